"""Meshes, query sets and the byte comparison that the tests of the per-lane walk queries share (test_closest_point.py, test_all_hits.py,
test_near.py, test_sphere_cast.py).  A plain module: nothing here is collected, and no test module imports another."""
import os

import numpy as np
import pytest

import scenes
from conftest import GOLDEN

MESH2K = os.path.join(GOLDEN, "mesh_2k.3d")
F = np.float32


def mesh_of(b):
    """(vertices, indices) of a builder in authoring order, copied"""
    d = b.desc()
    return (np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(F, copy=True),
            np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int32, copy=True))


def queries_of(points, max_distance=np.inf):
    q = np.zeros((len(points), 4), F)
    q[:, 0:3] = points
    q[:, 3] = max_distance
    return q


def mesh_scene(gx, v, idx, split=None):
    b = gx.SceneBuilder()
    b.add_mesh(np.ascontiguousarray(v, F), np.ascontiguousarray(idx, np.int32), b.MatteMaterial(scenes.WHITE, 60.0))
    if split:
        b.set_bvh_split_method(split)
    return b


def dragon(split=None):
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    if split:
        b.set_bvh_split_method(split)
    return b


def bound_of(v):
    return v.min(axis=0), v.max(axis=0)


def uniform_in(lo, hi, n, rng, scale=1.0):
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * scale
    return rng.uniform(c - h, c + h, (n, 3)).astype(F)


def surface_samples(v, idx, n, rng, jitter):
    t = idx[rng.integers(0, len(idx), n)]
    u = rng.uniform(0, 1, (n, 2))
    flip = u.sum(axis=1) > 1
    u[flip] = 1 - u[flip]
    p = v[t[:, 0]] + u[:, 0:1] * (v[t[:, 1]] - v[t[:, 0]]) + u[:, 1:2] * (v[t[:, 2]] - v[t[:, 0]])
    return (p + rng.uniform(-jitter, jitter, (n, 3))).astype(F)


def assert_same(got, want, what=""):
    """bytes of two arrays of records or counts"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} entries differ; first {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}")


def chain_scene(gx, n=36):
    """tests/test_ray_queries_device.py's chain, restated: n small triangles facing +x at x = 2^-k on the x axis.  The middle split peels
    one off per level, so the binary tree is a chain n - 1 deep."""
    v, idx = [], []
    for k in range(n):
        x, s = 2.0 ** -k, 0.3 * 2.0 ** -k
        v += [(x, -s, -s), (x, s, -s), (x, 0.0, 2 * s)]
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    b = gx.SceneBuilder()
    b.add_mesh(np.array(v, F), np.array(idx, np.int32), b.MatteMaterial(scenes.WHITE, 60.0))
    b.set_bvh_split_method("middle")
    return b


def binary_depth(scene):
    """the depth of the flattened binary tree (the root at 0), walked through scene.bvh(): an interior node's children are the next node
    and the node at its offset"""
    _, meta, _ = scene.bvh()
    depth, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        depth = max(depth, d)
        if meta[i, 1] == 0:
            todo += [(i + 1, d + 1), (int(meta[i, 0]), d + 1)]
    return depth


def concentric_mesh(rng):
    """130 nested triangles whose bounds share one centre (no split separates them: one leaf over 127 primitives) and 50 others"""
    v = []
    for k in range(130):
        s = 0.5 + 0.01 * k
        v += [(-s, -s, -s), (s, -s, s), (-s, s, s)]
    for k in range(50):
        c = rng.uniform(-4, 4, 3)
        v += [tuple(c + rng.uniform(-0.3, 0.3, 3)) for _ in range(3)]
    return np.array(v, F), np.arange(3 * 180, dtype=np.int32).reshape(-1, 3)


def sliver_mesh(rng, n=240):
    """long thin triangles through one region: every box overlaps most others, so leaves are large and boxes say little"""
    a = rng.uniform(-2, 2, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = np.stack([a - 3 * d, a + 3 * d, a + 3 * d + rng.normal(0, 1e-3, (n, 3))], axis=1).reshape(-1, 3)
    return v.astype(F), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


FAN_D = 1.5   # the query's height over the apex: dist2 = 2.25 and max_distance = 1.5 gives r2 = 2.25 exactly


def fan_mesh(rng, copies=1, others=0):
    """12 triangles around the apex (0, 0, 0), a cone that opens towards -z, in shuffled authoring order with randomly rotated corner
    order; `copies` of the fan (coincident triangles); `others` small triangles at least 2 FAN_D from the query (0, 0, FAN_D), shuffled
    in between.  Returns (v, idx, the fan's authoring indices ascending)."""
    ang = 2 * np.pi * np.arange(12) / 12
    ring = np.stack([np.cos(ang), np.sin(ang), np.full(12, -0.75)], axis=1)
    v = np.concatenate([[(0.0, 0.0, 0.0)], ring])
    tris = [np.roll((0, 1 + i, 1 + (i + 1) % 12), rng.integers(0, 3)) for i in range(12)] * copies
    is_fan = [True] * len(tris)
    for _ in range(others):
        while True:
            c = rng.uniform(-9, 9, 3)
            if np.linalg.norm(c - (0, 0, FAN_D)) >= 2 * FAN_D + 0.5:
                break
        base = len(v)
        v = np.concatenate([v, c + rng.uniform(-0.25, 0.25, (3, 3))])
        tris.append(np.array((base, base + 1, base + 2)))
        is_fan.append(False)
    perm = rng.permutation(len(tris))
    idx = np.array([tris[j] for j in perm], np.int32)
    return v.astype(F), idx, np.flatnonzero(np.array(is_fan)[perm])


@pytest.fixture(params=["caller_order", "binned"])
def order(request):
    """Both ways a call takes its point queries to the walk: in caller order (batches below 65536 queries) and binned by Morton key
    first, which GNXR_CLOSEST_BIN_MIN=1 asks of every batch.  Records and counts must not notice."""
    if request.param == "binned":
        os.environ["GNXR_CLOSEST_BIN_MIN"] = "1"
    yield request.param
    os.environ.pop("GNXR_CLOSEST_BIN_MIN", None)
