"""Closest-point queries (include/gnxr.h, "Closest-point queries"): the numpy restatement (tests/closest_reference.py) on hand-made cases and
the lower-bound property that makes the walk's pruning exact, then gnxr_closest_point_device / gnxr_closest_point on the GPU against the
restatement's brute force over all triangles.  Every comparison of records is on their bytes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import closest_reference as cr
import scenes
from query_cases import (assert_same, binary_depth, bound_of, chain_scene, concentric_mesh, dragon, mesh_of, mesh_scene, order, queries_of,  # noqa: F401
                         surface_samples, uniform_in)

ERR_INVALID = -1
F = np.float32
INF = F(np.inf)


# ---------------------------------------------------------------- helpers
def device_records(scene, queries, **kw):
    res = scene.closest_point(torch.from_numpy(np.array(queries, F)).cuda(), **kw)
    torch.cuda.synchronize()
    return res.records.cpu().numpy().view(cr.RECORD).reshape(-1)


def same_bytes(x, y):
    return x.dtype.itemsize == y.dtype.itemsize and len(x) == len(y) and x.tobytes() == y.tobytes()


_dragon_cache = {}


def dragon_case():
    """the 2 k mesh in its Cornell box, its query set and the brute force over it: computed once, shared, never written"""
    if not _dragon_cache:
        v, idx = mesh_of(dragon())
        rng = np.random.default_rng(21)
        lo, hi = bound_of(v)
        pts = np.concatenate([uniform_in(lo, hi, 2048, rng), surface_samples(v, idx, 2048, rng, 1e-3)])
        q = queries_of(pts)
        want = cr.closest_points(v, idx, q)
        for x in (v, idx, q, want):
            x.setflags(write=False)
        _dragon_cache.update(v=v, idx=idx, q=q, want=want)
    return _dragon_cache


_deep_tree_cache = []


def deep_tree_case(gx):
    """(queries, brute force) of chain_scene(36): points on and around the x axis beyond the smallest triangle, and some anywhere; computed
    once, shared, never written"""
    if not _deep_tree_cache:
        v, idx = mesh_of(chain_scene(gx))
        rng = np.random.default_rng(8)
        x = (2.0 ** -35) * rng.uniform(-2, 1, 4096)
        pts = np.stack([x, rng.normal(0, 2.0 ** -36, 4096), rng.normal(0, 2.0 ** -36, 4096)], axis=1).astype(F)
        pts[:64, 1:] = 0   # exactly on the axis
        pts = np.concatenate([pts, uniform_in(*bound_of(v), 512, rng, 1.5)])
        q = queries_of(pts)
        want = cr.closest_points(v, idx, q)
        q.setflags(write=False)
        want.setflags(write=False)
        _deep_tree_cache.extend([q, want])
    return _deep_tree_cache


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_closest_point_device", "gnxr_closest_point_counted_device", "gnxr_closest_point"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.PointQuery) == 16 and C.sizeof(gx._abi.ClosestPoint) == 32
    assert gx.CLOSEST_DTYPE == cr.RECORD
    assert gx._abi.GNXR_ABI_VERSION == 5 and gx._abi.PointQuery not in gx._abi.ABI_STRUCTS and gx._abi.ClosestPoint not in gx._abi.ABI_STRUCTS


def test_restatement_exact_cases():
    """Triangle (0,0,0), (4,0,0), (0,4,0) and points with small integer coordinates: every value is exactly representable."""
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F)
    idx = np.array([(0, 1, 2)], np.int32)
    cases = [   # q, p, b1, b2, feature, dist2
        ((1, 1, 3), (1, 1, 0), 0.25, 0.25, 0, 9),       # over the face
        ((1, 1, 0), (1, 1, 0), 0.25, 0.25, 0, 0),       # on the face
        ((-1, -2, 2), (0, 0, 0), 0, 0, 4, 9),           # beyond vertex a
        ((6, -1, 0), (4, 0, 0), 1, 0, 5, 5),            # beyond vertex b
        ((-1, 7, 1), (0, 4, 0), 0, 1, 6, 11),           # beyond vertex c
        ((2, -3, 0), (2, 0, 0), 0.5, 0, 1, 9),          # beyond edge ab
        ((-2, 1, 1), (0, 1, 0), 0, 0.25, 2, 5),         # beyond edge ac
        ((4, 4, 0), (2, 2, 0), 0.5, 0.5, 3, 8),         # beyond edge bc
        ((3, 3, 1), (2, 2, 0), 0.5, 0.5, 3, 3),
    ]
    q = queries_of(np.array([c[0] for c in cases], F))
    rec = cr.closest_points(v, idx, q)
    for r, (_, p, b1, b2, feature, dist2) in zip(rec, cases):
        assert r["prim"] == 0 and tuple(r["p"]) == p and r["b1"] == b1 and r["b2"] == b2 and r["feature"] == feature and r["dist2"] == dist2
    assert sorted(set(rec["feature"])) == [0, 1, 2, 3, 4, 5, 6]
    # the radius: dist2 <= max_distance^2 counts, the rest has no winner and a zero record; bad queries have none either
    q = queries_of(np.array([(1, 1, 3)] * 6 + [(np.nan, 0, 0)], F), [3, 2.999, np.inf, -1, np.nan, 0, np.inf])
    rec = cr.closest_points(v, idx, q)
    assert list(rec["prim"]) == [0, -1, 0, -1, -1, -1, -1]
    assert all(r.tobytes() == np.array([(-1, 0, (0, 0, 0), 0, 0, 0)], cr.RECORD).tobytes() for r in rec[rec["prim"] < 0])
    # the tie rule: two copies of the triangle, the smaller authoring index wins
    rec, tied = cr.closest_points(v, np.array([(0, 1, 2), (0, 1, 2)], np.int32), queries_of(np.array([(1, 1, 3)], F)), ties=True)
    assert rec["prim"][0] == 0 and tied[0] == 2


def test_box_distance_is_a_lower_bound_on_bits():
    """The claim that makes the skip rule exact: in fp32, the distance to any box that encloses a triangle's vertices is at most the
    triangle's dist2, and a wider box is never farther than a tighter one.  10^6 seeded cases; a third translated by 1000, a third scaled by
    2^-20.  Zero exceptions."""
    rng = np.random.default_rng(2024)
    n = 1_000_000
    tri = rng.uniform(-1, 1, (n, 3, 3)) * rng.choice([1.0, 0.1, 1e-3], (n, 1, 1))   # large to sliver-sized triangles
    q = rng.uniform(-2, 2, (n, 3))
    on = rng.integers(0, 4, n) == 0   # a quarter of the points close to the triangle's plane region
    w = rng.dirichlet((1, 1, 1), n)
    q[on] = (np.einsum("nk,nkc->nc", w, tri) + rng.normal(0, 1e-4, (n, 3)))[on]
    kind = np.arange(n) % 3
    shift = np.where(kind == 1, 1000.0, 0.0)[:, None]
    scale = np.where(kind == 2, 2.0 ** -20, 1.0)[:, None]
    a, b, c = ((tri[:, k] + shift) * scale for k in range(3))
    q = (q + shift) * scale
    a, b, c, q = (x.astype(F) for x in (a, b, c, q))
    dist2, p, _, _, _ = cr.closest_on_triangle(a, b, c, q)
    lo, hi = cr.triangle_bounds(a, b, c)
    grow = (rng.uniform(0, 1, (2, n, 3)) * rng.choice([0.0, 1e-6, 1e-2, 1.0], (2, n, 1)) * (scale + shift * 1e-3)).astype(F)
    lo_w, hi_w = lo - grow[0], hi + grow[1]
    assert (lo_w <= lo).all() and (hi_w >= hi).all()
    tight, wide = cr.box_dist2(lo, hi, q), cr.box_dist2(lo_w, hi_w, q)
    ok = ~np.isnan(dist2)
    assert ok.mean() > 0.99
    assert ((p >= lo) & (p <= hi))[ok].all()
    assert (tight[ok] <= dist2[ok]).all(), int((tight[ok] > dist2[ok]).sum())
    assert (wide <= tight).all(), int((wide > tight).sum())
    assert (tight > 0).mean() > 0.5 and (tight[ok] == dist2[ok]).any()   # the bound is not vacuous: it is often positive and sometimes met


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0 and n < 0 are refused before anything is looked at (the handle is a dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    for fn in (L.gnxr_closest_point_device, lambda s, q, n, o, st: L.gnxr_closest_point_counted_device(s, q, n, o, p, st)):
        assert fn(None, p, 1, p, None) == ERR_INVALID
        assert fn(None, p, 0, p, None) == ERR_INVALID
        assert fn(p, None, 4, p, None) == ERR_INVALID
        assert fn(p, p, 4, None, None) == ERR_INVALID
        assert fn(p, p, -1, p, None) == ERR_INVALID
    assert L.gnxr_closest_point_counted_device(p, p, 4, p, None, None) == ERR_INVALID
    assert L.gnxr_closest_point(None, C.cast(p, C.POINTER(gx._abi.PointQuery)), 1, C.cast(p, C.POINTER(gx._abi.ClosestPoint))) == ERR_INVALID
    assert L.gnxr_closest_point(p, None, 1, C.cast(p, C.POINTER(gx._abi.ClosestPoint))) == ERR_INVALID
    assert L.gnxr_closest_point(p, C.cast(p, C.POINTER(gx._abi.PointQuery)), -1, C.cast(p, C.POINTER(gx._abi.ClosestPoint))) == ERR_INVALID


def test_python_refuses_other_inputs_before_the_library(gx):
    """The cases tests/test_python_refusals.py exercises for intersect: only contiguous float32 (n, 3) / (n, 4) tensors on the scene's device
    pass; everything else raises before a library call (the handle is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    bad = [np.zeros((4, 3), F), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 5)), torch.zeros((3, 4)).t(), torch.zeros((4, 6))[:, ::2],
           torch.zeros(12), "points", None, torch.zeros((4, 3)), torch.zeros((4, 4))]
    for b in bad:
        with pytest.raises(ValueError):
            s.closest_point(b)
    with pytest.raises(ValueError):
        s.closest_point(torch.zeros((4, 4)), max_distance=1.0)


# ---------------------------------------------------------------- GPU


def cornell_points(v, idx):
    """uniform in 1.5 x the bound; on vertices, edge midpoints and face centroids; those pushed off along the geometric normal"""
    rng = np.random.default_rng(5)
    a, b, c = (v[idx[:, k]] for k in range(3))
    on = np.concatenate([a, b, c, F(0.5) * (a + b), F(0.5) * (a + c), F(0.5) * (b + c), (a + b + c) / F(3)]).astype(F)
    nrm = np.cross(b - a, c - a)
    nrm = np.tile((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F), (7, 1))
    special = np.concatenate([on] + [(on + F(h) * nrm).astype(F) for h in (2.0 ** -20, 2.0 ** -10, 1.0)])
    lo, hi = bound_of(v)
    return np.concatenate([uniform_in(lo, hi, 4096 - len(special), rng, 1.5), special]), len(on)


@pytest.mark.gpu
def test_cornell(gpu):
    b = scenes.cornell()
    v, idx = mesh_of(b)
    pts, n_on = cornell_points(v, idx)
    assert len(pts) == 4096
    q = queries_of(pts)
    want, tied = cr.closest_points(v, idx, q, ties=True)
    assert (tied[-4 * n_on:] > 1).sum() >= 100   # the tie rule is under test: shared vertices and edges
    assert (want["prim"] >= 0).all() and len(set(want["feature"])) == 7
    scene = gpu.Scene(b)
    assert_same(device_records(scene, q), want)
    # the host entry point walks the same way
    assert_same(scene.ClosestPoint(q).view(cr.RECORD), want)
    # points as (n, 3) with the default radius
    res = scene.closest_point(torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    assert_same(res.records.cpu().numpy().view(cr.RECORD).reshape(-1), want)
    assert (res.prim.cpu().numpy() == want["prim"]).all() and (res.feature.cpu().numpy() == want["feature"]).all()
    assert (res.point.cpu().numpy() == want["p"]).all() and (res.b1b2.cpu().numpy()[:, 1] == want["b2"]).all() and (res.dist2.cpu().numpy() == want["dist2"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65535, 65536, (1 << 22) + 257])
def test_binning_sizes(gpu, n):
    """From 65536 queries on a call bins them by Morton key, 2^22 per launch: one below, the first binned size, and one launch and a bit
    (the points repeat a set of 8192, so the brute force stays small)."""
    b = scenes.cornell()
    v, idx = mesh_of(b)
    rng = np.random.default_rng(n)
    base = queries_of(uniform_in(*bound_of(v), 8192, rng, 1.5), rng.choice([np.inf, 0.5, 0.1], 8192))
    base_want = cr.closest_points(v, idx, base, chunk=2048)
    pick = rng.integers(0, 8192, n)
    assert_same(device_records(gpu.Scene(b), base[pick]), base_want[pick])


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts"])
def test_split_methods(gpu, split, order):
    """the records do not depend on the tree: every split method gives the brute force's bytes (and so the four runs are identical)"""
    case = dragon_case()
    scene = gpu.Scene(dragon(split))
    assert_same(device_records(scene, case["q"]), case["want"])


@pytest.mark.gpu
def test_translated_mesh(gpu, order):
    """The 2 k mesh at (1000, 1000, 1000), where an ulp is 6e-5: boxes and closest points round coarsely, and a skip rule without an epsilon
    holds only because the closest point is clamped into the triangle's bounds."""
    v, idx = mesh_of(dragon())
    idx = idx[:len(idx) - 12]   # the mesh without the box and its light
    used = np.unique(idx)
    v = (v[used] + F(1000)).astype(F)
    idx = np.searchsorted(used, idx).astype(np.int32)
    rng = np.random.default_rng(22)
    lo, hi = bound_of(v)
    q = queries_of(np.concatenate([uniform_in(lo, hi, 2048, rng), surface_samples(v, idx, 2048, rng, 1e-3)]))
    want, tied = cr.closest_points(v, idx, q, ties=True)
    assert (tied > 1).sum() > 100   # at this magnitude distances collide: the tie rule decides many winners
    for split in ("sah", "hlbvh"):
        assert_same(device_records(gpu.Scene(mesh_scene(gpu, v, idx, split)), q), want)


@pytest.mark.gpu
def test_radius(gpu, order):
    """max_distance per point from the brute-force answer: sqrt(dist2) one ulp down and up, 0, +inf, -1 and NaN"""
    case = dragon_case()
    v, idx, q0, free = case["v"], case["idx"], case["q"], case["want"]
    root = np.sqrt(free["dist2"])
    choice = np.arange(len(q0)) % 6
    md = np.select([choice == 0, choice == 1, choice == 2, choice == 3, choice == 4],
                   [np.nextafter(root, F(0)), np.nextafter(root, INF), F(0), INF, F(-1)], F(np.nan)).astype(F)
    q = queries_of(q0[:, 0:3], md)
    want = cr.closest_points(v, idx, q)
    down, up = want[choice == 0], want[choice == 1]
    assert (down["prim"] == -1).any() and (up["prim"] >= 0).all()   # rejected by one ulp; accepted one ulp up
    assert (want["prim"][choice >= 4] == -1).all() and same_bytes(want[choice == 3], free[choice == 3])
    scene = gpu.Scene(dragon())
    assert_same(device_records(scene, q), want)
    # the same radii as a tensor beside (n, 3) points, and one number for all
    res = scene.closest_point(torch.from_numpy(q[:, 0:3].copy()).cuda(), max_distance=torch.from_numpy(md).cuda())
    one = scene.closest_point(torch.from_numpy(q[:, 0:3].copy()).cuda(), max_distance=0.05)
    torch.cuda.synchronize()
    assert_same(res.records.cpu().numpy().view(cr.RECORD).reshape(-1), want)
    assert_same(one.records.cpu().numpy().view(cr.RECORD).reshape(-1), cr.closest_points(v, idx, queries_of(q[:, 0:3], 0.05)))


@pytest.mark.gpu
def test_deep_tree(gpu, order):
    """chain_scene(36): from points on the x axis beyond the smallest triangle the walk descends the whole chain with a sibling on its stack
    per level.  Run with the default LDS levels, where the tree's need exceeds them (the global spill carries the rest), and forced onto 2
    LDS levels through GNXR_CLOSEST_LDS_LEVELS, the launch's knob."""
    q, want = deep_tree_case(gpu)
    assert (want["prim"] >= 30).sum() > 3000
    scene = gpu.Scene(chain_scene(gpu))
    assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
    assert_same(device_records(scene, q), want)
    os.environ["GNXR_CLOSEST_LDS_LEVELS"] = "2"
    try:
        assert_same(device_records(scene, q), want)
        assert_same(device_records(gpu.Scene(dragon()), dragon_case()["q"]), dragon_case()["want"])
    finally:
        del os.environ["GNXR_CLOSEST_LDS_LEVELS"]


@pytest.mark.gpu
def test_deep_binary_tree_spills(gpu, order):
    """test_deep_tree's chain and points on a scene kept on the binary tree by the creation switch, with 2 LDS levels: the binary walk,
    its LDS levels and its global spill together.  chain_scene(36) creates (its depth stays inside the 64-entry limit of scene creation)."""
    q, want = deep_tree_case(gpu)
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(chain_scene(gpu))
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    assert binary_depth(scene) + 2 > 2   # the walk's bound on this tree against the LDS levels below: the spill carries the rest
    os.environ["GNXR_CLOSEST_LDS_LEVELS"] = "2"
    try:
        assert_same(device_records(scene, q), want)
    finally:
        del os.environ["GNXR_CLOSEST_LDS_LEVELS"]


@pytest.mark.gpu
def test_off_the_wide_tree(gpu, order):
    rng = np.random.default_rng(9)
    v, idx = concentric_mesh(rng)
    q = queries_of(np.concatenate([uniform_in(*bound_of(v), 3072, rng, 1.2), surface_samples(v, idx, 1024, rng, 1e-3)]))
    want = cr.closest_points(v, idx, q)
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    _, meta, _ = scene.bvh()
    assert meta[:, 1].max() > 127   # a leaf the 4-wide encoding cannot hold: the scene is on the binary walk
    assert_same(device_records(scene, q), want)
    # and a scene kept on the binary tree by the creation switch
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        binary = gpu.Scene(dragon())
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    assert_same(device_records(binary, dragon_case()["q"]), dragon_case()["want"])


@pytest.mark.gpu
def test_degenerate_input(gpu, order):
    rng = np.random.default_rng(10)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    idx = np.arange(60, dtype=np.int32).reshape(-1, 3)
    v[3:6] = [(0, 0, 0), (0.5, 0.5, 0.5), (1, 1, 1)]          # zero area: three collinear vertices
    v[10] = v[9]                                               # two coincident vertices
    pts = np.concatenate([uniform_in(*bound_of(v), 3000, rng, 1.5), surface_samples(v, idx, 1000, rng, 1e-4),
                          np.linspace((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 64).astype(F)])   # along the collinear triangle
    bad = uniform_in(*bound_of(v), 32, rng)
    bad[0:8, 0] = np.nan; bad[8:12, 2] = np.nan
    bad[12:18, 0] = np.inf; bad[18:24, 1] = -np.inf; bad[24:28] = np.inf; bad[28:32, 2] = -np.inf
    q = queries_of(np.concatenate([pts, bad]))
    want = cr.closest_points(v, idx, q)
    assert (want["prim"][len(pts):len(pts) + 12] == -1).all() and (want["prim"][:len(pts)] >= 0).all()
    assert (want["prim"] == 1).any() or (want["prim"] == 3).any()
    assert_same(device_records(gpu.Scene(mesh_scene(gpu, v, idx)), q), want)


@pytest.mark.gpu
def test_live_scene(gpu, order):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    set_geometry with another triangle count -> the brute force over the new mesh"""
    case = dragon_case()
    b = dragon()
    v, idx = mesh_of(b)
    scene = gpu.Scene(b)
    assert_same(device_records(scene, case["q"]), case["want"])
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(0.15) * np.sin(F(5) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    scene.update_vertices(torch.from_numpy(v2[:n_mesh_v].copy()).cuda())
    want2 = cr.closest_points(v2, idx, case["q"])
    assert not same_bytes(want2, case["want"])
    assert_same(device_records(scene, case["q"]), want2)
    scene.rebuild_bvh()
    assert_same(device_records(scene, case["q"]), want2)
    rng = np.random.default_rng(11)
    v3 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v3[1::3] = v3[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    v3[2::3] = v3[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    idx3 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    scene.set_geometry(v3, idx3, np.zeros(300, np.int32), tri_light=tri_light)
    assert_same(device_records(scene, case["q"]), cr.closest_points(v3, idx3, case["q"]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_batch_sizes_and_out(gpu, n, order):
    case = dragon_case()
    scene = gpu.Scene(dragon())
    q = torch.from_numpy(case["q"][:n].copy()).cuda()
    out = torch.full((n, 8), 7.0, device="cuda")
    res = scene.closest_point(q, out=out)
    torch.cuda.synchronize()
    assert res.records is out and out.shape == (n, 8)
    assert_same(out.cpu().numpy().view(cr.RECORD).reshape(-1), case["want"][:n])
    assert len(scene.ClosestPoint(case["q"][:n])) == n
    with pytest.raises(ValueError):
        scene.closest_point(q, out=torch.zeros((n + 1, 8), device="cuda"))


@pytest.mark.gpu
def test_streams(gpu, order):
    """Queries written by torch on a side stream, answered there and reduced there with no synchronise in between; then two calls on two
    streams at once."""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    src = torch.from_numpy(case["q"].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q = src * 1.0
        res = scene.closest_point(q, stream=side)
        prim_sum = res.prim.to(torch.int64).sum()
    side.synchronize()
    assert int(prim_sum) == int(case["want"]["prim"].astype(np.int64).sum())
    assert_same(res.records.cpu().numpy().view(cr.RECORD).reshape(-1), case["want"])
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream()); sb.wait_stream(torch.cuda.current_stream())
    qa, qb = src[:3000].contiguous(), src[1000:].contiguous()
    torch.cuda.synchronize()
    ra, rb = scene.closest_point(qa, stream=sa), scene.closest_point(qb, stream=sb)
    torch.cuda.synchronize()
    assert_same(ra.records.cpu().numpy().view(cr.RECORD).reshape(-1), case["want"][:3000])
    assert_same(rb.records.cpu().numpy().view(cr.RECORD).reshape(-1), case["want"][1000:])


@pytest.mark.gpu
def test_refusals(gpu):
    """misaligned pointers, host memory, a negative n and an array that runs past its allocation give GNXR_ERR_INVALID with the front end's
    messages before anything is queued; wrong tensors raise ValueError; the scene still answers afterwards"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    L = gpu.lib()
    q = torch.from_numpy(case["q"].copy()).cuda()
    out = torch.zeros((len(q), 8), device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.gnxr_last_error().decode()
    assert L.gnxr_closest_point_device(scene._h, P(q, 4), 100, P(out), None) == ERR_INVALID and "d_queries is not 16-byte aligned" in err()
    assert L.gnxr_closest_point_device(scene._h, P(q), 100, P(out, 8), None) == ERR_INVALID and "d_out is not 16-byte aligned" in err()
    assert L.gnxr_closest_point_device(scene._h, P(q), -1, P(out), None) == ERR_INVALID
    host = np.zeros((100, 8), F)
    assert L.gnxr_closest_point_device(scene._h, C.c_void_p(host.ctypes.data), 100, P(out), None) == ERR_INVALID and "d_queries is not device memory" in err()
    assert L.gnxr_closest_point_device(scene._h, P(q), 100, C.c_void_p(host.ctypes.data), None) == ERR_INVALID and "d_out is not device memory" in err()
    lone = torch.zeros((64, 4), device="cuda")
    assert L.gnxr_closest_point_device(scene._h, P(lone), 1 << 20, P(out), None) == ERR_INVALID and "d_queries" in err()
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.gnxr_closest_point_counted_device(scene._h, P(q), 100, P(out), P(counts, 4), None) == ERR_INVALID and "d_counts" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (counts == 0).all()   # nothing was queued by the refused calls
    for bad in (q.double(), q.cpu(), q[:, :2].contiguous(), q.t(), case["q"]):
        with pytest.raises(ValueError):
            scene.closest_point(bad)
    with pytest.raises(ValueError):
        scene.closest_point(q[:, 0:3].contiguous(), max_distance=torch.zeros(5, device="cuda"))
    with pytest.raises(TypeError):
        scene.closest_point(q[:, 0:3].contiguous(), max_distance="far")
    assert_same(device_records(scene, case["q"]), case["want"])
    # the counting form: the same records, and counters that say the walk prunes
    res = scene.closest_point(q, counts=counts)
    torch.cuda.synchronize()
    assert_same(res.records.cpu().numpy().view(cr.RECORD).reshape(-1), case["want"])
    nodes, tris = (int(x) for x in counts.cpu())
    assert len(q) <= nodes and len(q) <= tris < len(q) * len(case["idx"]) // 4
