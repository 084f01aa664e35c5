"""The device HLBVH build (csrc/hlbvh_build.hip.h, csrc/api_hlbvh.hip.h) against a plain reference, beyond one sort tile.

tests/hlbvh_reference.py restates BVHAccel::HLBVHBuild in sequential numpy float32.  The CPU tests here pin that restatement to three
dumps of the compiled reference (bvh_hlbvh.npz mesh2k / smooth, one tile each; bvh_hlbvh_6k.npz, three tiles) and check it against
itself on every generated input; the GPU tests then require the device's flattened tree and primitive order to EQUAL the reference's
on inputs sized to reach each path of the build (kTile = 2048 primitives per sort block):

  tiny        n = 1, 2, 3; 3 triangles on one centroid      U == 1 (no internal kernel), T == 1, the root is a leaf
  tile edge   n = 2047, 2048, 2049, 4097                    n_tiles 1 -> 2 -> 3, ragged last tile, first non-zero cross-tile offsets
  stability   6000 triangles on 200 centroids               leaves of ~30 whose order only a stable sort gets right, across chunks and tiles
  uniform70k  n = 70 000                                    35 tiles: 64 * 35 histogram words = a second scan tile; all 4096 treelets
  clustered   n = 20 000, 8 clusters + outliers             few deep treelets, many empty SAH buckets
  flat        n = 3000 on a plane / on a line               the hi > lo guards of the Morton kernel, a split axis chosen among zero extents
  dump 6k     the 6 k golden                                device == compiled reference above one tile
  large       n = 2 200 000                                 1075 tile sums: the carry loop of k_scan_sums (vectorised checks only)
  refusal     65 536 triangles on one centroid + 100        the checked error, and a correct build right after it

Every comparison is exact: meta and order equal, bounds equal as numbers and bit-equal wherever non-zero (np.minimum and fminf may
pick different zeros of a +0 / -0 pair; tests/test_scene_update.py grants this build the same).  After the uniform70k and the clustered
comparison 20 000 rays go through Scene.Intersect and through the oracle walking its OWN SAH tree: the closest hit does not depend on
the tree, so a primitive both (equal) HLBVH trees lost would show; 20 000 more are aimed at triangles (aimed_rays), since random rays
hardly meet the clustered case.  The stability case holds triangles through one point, where `prim`
can be ambiguous between two of them at equal t: no ray check there.

Figures per case (n_tiles = ceil(n / 2048), U = distinct codes = leaves, T = treelets; `PYTHONPATH=. python tests/test_hlbvh_build.py`
prints them) and the seconds the reference takes on one CPU core, which dominate each test:

  case          n        n_tiles  U       T     nodes    largest leaf  reference s
  tiny1         1        1        1       1     1        1             0.00
  tiny2         2        1        2       2     3        1             0.00
  tiny3         3        1        3       3     5        1             0.00
  tiny3shared   3        1        1       1     1        3             0.00
  uniform2047   2047     1        2047    1599  4093     1             0.8
  uniform2048   2048     1        2048    1598  4095     1             0.8
  uniform2049   2049     2        2049    1613  4097     1             0.7
  uniform4097   4097     3        4097    2610  8193     1             1.2
  stability     6000     3        200     194   399      46            0.1
  uniform70000  70000    35       69998   4096  139995   2             2.1
  clustered     20000    10       17739   32    35477    5             0.1
  flat_plane    3000     2        2988    256   5975     2             0.1
  flat_line     3000     2        1024    16    2047     3             0.0
  dump 6k       5772     3        5750    -     11499    -             0.2
  large         2200000  1075     -       -     -        -             (no reference tree)
"""
import functools
import os
import time

import numpy as np
import pytest

import hlbvh_reference as hr
import oracle_lib as ol
import scenes
from conftest import GOLDEN, golden

K_TILE = 2048


# ---------------------------------------------------------------- comparison
def same_bounds(a, b):
    """equal as numbers, and bit-equal wherever the value is not a zero"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, b) and bool(((a.view(np.uint32) == b.view(np.uint32)) | (a == 0)).all())


def first_difference(got, want):
    """None when the trees are the same under the rule above, else a sentence naming the first differing order index / node"""
    (gb, gm, go), (wb, wm, wo) = got, want
    if len(go) != len(wo) or not (go == wo).all():
        i = int(np.flatnonzero(go[:min(len(go), len(wo))] != wo[:min(len(go), len(wo))])[0]) if len(go) == len(wo) else -1
        return f"order differs: lengths {len(go)} / {len(wo)}, first at index {i}" + (f" (tile {i // K_TILE}): {go[i]} != {wo[i]}" if i >= 0 else "")
    if gm.shape != wm.shape:
        return f"node counts differ: {len(gm)} / {len(wm)}"
    if not (gm == wm).all():
        i = int(np.flatnonzero((gm != wm).any(axis=1))[0])
        return f"meta differs first at node {i}: {gm[i].tolist()} != {wm[i].tolist()}"
    if not same_bounds(gb, wb):
        bad = ~(((gb.view(np.uint32) == wb.view(np.uint32)) | ((gb == 0) & (wb == 0))).all(axis=1))
        i = int(np.flatnonzero(bad)[0])
        return f"bounds differ first at node {i} (meta {gm[i].tolist()}): {gb[i].tolist()} != {wb[i].tolist()}"
    return None


def desc_arrays(b):
    d = b.desc()
    return (np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).copy(), np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).copy())


def self_check(tree, verts, idx):
    """what any HLBVH tree over these primitives satisfies, whatever its shape"""
    bounds, meta, order = tree
    n = len(idx)
    assert np.array_equal(np.sort(order), np.arange(n))
    leaf = meta[:, 1] > 0
    lv = meta[leaf][np.argsort(meta[leaf, 0], kind="stable")]
    assert lv[0, 0] == 0 and np.array_equal(lv[:-1, 0] + lv[:-1, 1], lv[1:, 0]) and lv[-1, 0] + lv[-1, 1] == n      # the leaves tile [0, n)
    assert len(meta) == 2 * int(leaf.sum()) - 1
    inner = np.flatnonzero(~leaf)
    c0, c1 = inner + 1, meta[inner, 0]
    assert (c1 > c0).all() and (c1 < len(meta)).all()
    assert same_bounds(bounds[inner, :3], np.minimum(bounds[c0, :3], bounds[c1, :3])) and same_bounds(bounds[inner, 3:], np.maximum(bounds[c0, 3:], bounds[c1, 3:]))
    plo, phi, _ = hr.primitive_boxes(verts, idx)
    assert same_bounds(bounds[0], np.concatenate([plo.min(axis=0), phi.max(axis=0)]))
    # every leaf's box is the union of its primitives' boxes
    starts = meta[leaf, 0]
    o = np.argsort(starts)
    assert same_bounds(bounds[leaf][o, :3], np.minimum.reduceat(plo[order], starts[o], axis=0)) and same_bounds(bounds[leaf][o, 3:], np.maximum.reduceat(phi[order], starts[o], axis=0))


# ---------------------------------------------------------------- inputs (every triangle from a seeded generator)
def soup(centres, rng, size=0.02):
    """one small triangle around each centre: (vertices [3n, 3], indices [n, 3])"""
    n = len(centres)
    v = (centres[:, None, :] + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def around(centres, rng):
    """triangles whose boxes are centred EXACTLY on `centres` (multiples of 1/64) with half extents of 1..63 / 1024 per axis and one of
    eight orientations: lo, hi and .5f * lo + .5f * hi are exact in float32, so triangles of one centre share centroid and Morton code"""
    n = len(centres)
    h = rng.integers(1, 64, (n, 3)) / 1024.0
    s = rng.choice([-1.0, 1.0], (n, 3))
    v2 = np.stack([-s[:, 0] * h[:, 0], s[:, 1] * h[:, 1], rng.integers(-8, 9, n) / 8.0 * h[:, 2]], 1)
    v = np.stack([centres - s * h, centres + s * h, centres + v2], 1).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def uniform(n, seed):
    rng = np.random.default_rng(seed)
    return soup(rng.uniform(-2.0, 2.0, (n, 3)), rng)


def grid_centres(k, rng):
    """k distinct points with coordinates that are multiples of 1/64 in [-2, 2]"""
    cells = rng.choice(257 ** 3, k, replace=False)
    return np.stack([cells % 257, cells // 257 % 257, cells // (257 * 257)], 1) / 64.0 - 2.0


def make_case(name):
    if name.startswith("tiny"):
        rng = np.random.default_rng(100)
        if name == "tiny3shared":
            return around(np.repeat(grid_centres(1, rng), 3, axis=0), rng)
        return soup(rng.uniform(-2.0, 2.0, (int(name[4:]), 3)), rng)
    if name.startswith("uniform"):
        n = int(name[7:])
        return uniform(n, 200 + n % 97)
    if name == "stability":
        rng = np.random.default_rng(300)
        return around(grid_centres(200, rng)[rng.integers(0, 200, 6000)], rng)
    if name == "clustered":
        rng = np.random.default_rng(400)
        mid = rng.uniform(-1.5, 1.5, (8, 3))
        c = mid[rng.integers(0, 8, 19990)] + rng.normal(0.0, 0.02, (19990, 3))
        return soup(np.concatenate([c, rng.uniform(-2.0, 2.0, (10, 3))]), rng, size=0.01)      # the ten outliers set the bounds
    if name in ("flat_plane", "flat_line"):
        rng = np.random.default_rng(500)
        c = np.zeros((3000, 3))
        c[:, 0] = rng.permutation(3000) / 1024.0 - 1.5          # exact in float32, like the boxes of around()
        if name == "flat_plane":
            c[:, 1] = rng.integers(-128, 129, 3000) / 64.0
        c[:, 2] = 0.25
        return around(c, rng)
    if name == "oversized":
        rng = np.random.default_rng(700)
        g = grid_centres(101, rng)
        return around(np.concatenate([np.repeat(g[:1], 65536, axis=0), g[1:]]), rng)
    raise KeyError(name)


TINY = ["tiny1", "tiny2", "tiny3", "tiny3shared"]
TILE_EDGE = ["uniform2047", "uniform2048", "uniform2049", "uniform4097"]
CASES = TINY + TILE_EDGE + ["stability", "uniform70000", "clustered", "flat_plane", "flat_line"]
RAY_CASES = ("uniform70000", "clustered")


def builder(gx, name):
    v, i = make_case(name)
    b = gx.SceneBuilder()
    b.add_mesh(v, i, b.MatteMaterial(scenes.WHITE, 60.0))
    b.set_bvh_split_method("hlbvh")
    return b


@functools.lru_cache(maxsize=None)
def reference_tree(name):
    """computed once per session and shared (read-only) by the CPU and the GPU tests of a case"""
    import gnxraytracer_amd as gx
    v, i = desc_arrays(builder(gx, name))
    tree = hr.hlbvh_reference(v, i)
    for a in tree:
        a.setflags(write=False)
    return tree


def figures(name, tree, n):
    _, meta, _ = tree
    codes = np.unique(hr.morton_codes(hr.primitive_boxes(*make_case(name))[2]))
    return (f"{name}: n={n} n_tiles={(n + K_TILE - 1) // K_TILE} nodes={len(meta)} U={int((meta[:, 1] > 0).sum())} "
            f"T={len(np.unique(codes >> hr.TREELET_SHIFT))} largest leaf={int(meta[:, 1].max())}")


def dump_scene(name):
    if name == "6k":
        b = scenes.dragon_cornell(6000, "glass+metal", mesh_path=scenes.synthetic_mesh_path(6000))
        g = golden("bvh_hlbvh_6k.npz")
        want = (g["bounds"], g["meta"], g["order"])
    else:
        b = scenes.smooth_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr")) if name == "smooth" else \
            scenes.dragon_cornell(2000, "glass+metal", mesh_path=os.path.join(GOLDEN, "mesh_2k.3d"))
        g = golden("bvh_hlbvh.npz")
        want = (g[name + "_bounds"], g[name + "_meta"], g[name + "_order"])
    b.set_bvh_split_method("hlbvh")
    return b, want


# ---------------------------------------------------------------- CPU: the reference against the compiled reference and against itself
@pytest.mark.parametrize("name", ["mesh2k", "smooth", "6k"])
def test_reference_reproduces_the_compiled_reference(gx, name):
    """tests/hlbvh_reference.py gives the LinearBVHNode[] and primitive order the compiled reference dumped for the same scene: the two
    one-tile dumps of test_hlbvh_build_matches_reference and the 6 k dump (5772 primitives with the box: three tiles)."""
    b, want = dump_scene(name)
    v, i = desc_arrays(b)
    assert len(i) == len(want[2])
    if name == "6k":
        assert (len(i) + K_TILE - 1) // K_TILE == 3
    tree = hr.hlbvh_reference(v, i)
    assert first_difference(tree, want) is None, first_difference(tree, want)
    self_check(tree, v, i)


@pytest.mark.parametrize("name", CASES)
def test_reference_is_consistent(gx, name):
    """order is a permutation, the leaves tile [0, n), interior boxes are the unions of their children, leaf boxes those of their
    primitives, the root box is the scene's; and the case reaches what it is there for"""
    b = builder(gx, name)
    v, i = desc_arrays(b)
    tree = reference_tree(name)
    self_check(tree, v, i)
    _, meta, _ = tree
    n, U = len(i), int((meta[:, 1] > 0).sum())
    codes = np.unique(hr.morton_codes(hr.primitive_boxes(v, i)[2]))
    T = len(np.unique(codes >> hr.TREELET_SHIFT))
    print(figures(name, tree, n))
    assert U == len(codes)
    if name == "tiny3shared":
        assert (n, U, len(meta)) == (3, 1, 1) and meta[0].tolist() == [0, 3, 0]
    if name == "uniform70000":
        assert (n + K_TILE - 1) // K_TILE == 35 and T == 4096
    if name == "stability":
        assert U == 200 and meta[:, 1].max() >= 30
    if name == "clustered":
        assert T < 200          # a few treelets hold nearly everything
    if name == "flat_line":
        assert len(np.unique(codes & 0x36db6db6)) == 1          # no y or z bit set: codes from one axis only


def test_reference_refuses_an_oversized_leaf(gx):
    """65 536 primitives with one Morton code make a leaf LinearBVHNode::nPrimitives (uint16_t) cannot count"""
    v, i = desc_arrays(builder(gx, "oversized"))
    assert len(i) == 65636
    with pytest.raises(ValueError, match="65535"):
        hr.hlbvh_reference(v, i)


# ---------------------------------------------------------------- GPU: the device tree equals the reference tree
def device_tree(gpu, b):
    scene = gpu.Scene(b)
    return scene, scene.bvh()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_tree_equals_reference(gpu, name):
    b = builder(gpu, name)
    scene, got = device_tree(gpu, b)
    diff = first_difference(got, reference_tree(name))
    assert diff is None, f"{name}: {diff}"
    if name in RAY_CASES:
        want_scene = ol.OracleScene(_with_sah(gpu, name))
        for kind, rays in (("random", scenes.random_rays(20000)), ("aimed", aimed_rays(name, 20000))):
            hits, want = scene.Intersect(rays), want_scene.Intersect(rays)
            hit = want["prim"] >= 0
            print(f"{name}: {int(hit.sum())} of {len(rays)} {kind} rays hit")
            if kind == "aimed":
                assert hit.sum() >= 0.99 * len(rays)
            assert np.array_equal(hits["prim"], want["prim"]), kind
            assert np.array_equal(hits["t"][hit].view(np.uint32), want["t"][hit].view(np.uint32)), kind


def aimed_rays(name, n):
    """rays from scenes.random_rays' origins through the barycentre of a randomly chosen triangle each.  The random rays of the issue
    hardly meet the clustered case's triangles (8 clusters a few hundredths wide in a box of 4: a few dozen of 20 000 hit), so these make
    the comparison say something there: a ray through a triangle's barycentre hits that triangle or one in front of it unless the
    triangle is thinner than the rounding of the direction (size 1e-2 against 1e-7), hence the 99 % the test asks for."""
    v, i = make_case(name)
    rng = np.random.default_rng(900)
    target = v[i[rng.integers(0, len(i), n)]].astype(np.float64).mean(axis=1)
    o = scenes.random_rays(n, seed=1)[:, :3]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return scenes.gx.make_rays(o, d.astype(np.float32))


def _with_sah(gx, name):
    b = builder(gx, name)
    b.set_bvh_split_method("sah")
    return b


@pytest.mark.gpu
def test_device_tree_equals_the_6k_dump(gpu):
    """device == compiled reference above one tile (5772 primitives, 3 tiles)"""
    b, want = dump_scene("6k")
    _, got = device_tree(gpu, b)
    diff = first_difference(got, want)
    assert diff is None, diff


@pytest.mark.gpu
def test_device_large_sort_and_runs(gpu):
    """n = 2 200 000: the head-flag scan has 1075 tile sums, so k_scan_sums takes a second loop iteration with a carry.  The full
    reference tree is too slow here; what is compared is vectorised: the order against the stable argsort of the reference Morton codes,
    the leaves against the runs of equal codes, the root box against the scene bounds, the node count against 2 U - 1."""
    v, i = make_case("uniform2200000")
    b = gpu.SceneBuilder()
    b.add_mesh(v, i, b.MatteMaterial(scenes.WHITE, 60.0))
    b.set_bvh_split_method("hlbvh")
    n = len(i)
    assert (n + K_TILE - 1) // K_TILE == 1075
    t0 = time.perf_counter()
    _, (bounds, meta, order) = device_tree(gpu, b)
    print(f"large: scene creation + export {time.perf_counter() - t0:.2f} s")
    plo, phi, cen = hr.primitive_boxes(v, i)
    codes = hr.morton_codes(cen)
    want_order = np.argsort(codes, kind="stable")
    bad = np.flatnonzero(order != want_order)
    assert len(bad) == 0, f"order differs at {len(bad)} places, first at index {bad[0]} (tile {bad[0] // K_TILE})"
    _, ustart = hr.code_runs(codes[want_order])
    runs = np.stack([ustart, np.diff(np.append(ustart, n))], 1)
    leaf = meta[:, 1] > 0
    got = meta[leaf, :2]
    assert np.array_equal(got[np.argsort(got[:, 0], kind="stable")], runs)
    assert same_bounds(bounds[0], np.concatenate([plo.min(axis=0), phi.max(axis=0)]))
    assert len(meta) == 2 * len(ustart) - 1


@pytest.mark.gpu
def test_oversized_leaf_is_refused_and_the_next_build_is_right(gpu):
    """65 536 triangles on one centroid: gnxr_scene_create returns the library's checked error (no device fault), and the next scene of
    the process builds the reference's tree"""
    b = builder(gpu, "oversized")
    with pytest.raises(gpu.GnxrError, match="a leaf exceeds 65535 primitives"):
        gpu.Scene(b)
    _, got = device_tree(gpu, builder(gpu, "uniform2049"))
    diff = first_difference(got, reference_tree("uniform2049"))
    assert diff is None, diff


if __name__ == "__main__":
    import gnxraytracer_amd as gx
    for case in CASES:
        t0 = time.perf_counter()
        tree = reference_tree(case)
        print(figures(case, tree, len(tree[2])), f"reference {time.perf_counter() - t0:.2f} s")
