"""Neighbour queries (include/gnxr.h, "Neighbour queries"): the numpy restatement (tests/near_reference.py) on hand-made cases, the refusals
of the C calls and of the Python methods without a device, then gnxr_near_device / gnxr_near on the GPU in both modes against the
restatement's brute force over all triangles.  Every comparison of records and counts is on their bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import closest_reference as cr
import near_reference as nr
import scenes
from conftest import ROOT
from query_cases import (FAN_D, assert_same, bound_of, chain_scene, concentric_mesh, dragon, fan_mesh, mesh_of, mesh_scene, order, queries_of,  # noqa: F401
                         sliver_mesh, surface_samples, uniform_in)

ERR_INVALID = -1
F = np.float32
INF = F(np.inf)
EMPTY = nr.empty_slots(1)[0]


# ---------------------------------------------------------------- helpers
def device_lists(scene, queries, K, nearest, **kw):
    """(records (n, K) of nr.RECORD, counts) of one device call on ready-made (n, 4) records"""
    q = torch.from_numpy(np.array(queries, F)).cuda()
    res = scene.nearest(q, K, **kw) if nearest else scene.within(q, None, K, **kw)
    torch.cuda.synchronize()
    return res.records.cpu().numpy().view(nr.RECORD).reshape(len(q), K), res.count.cpu().numpy()


def check_both_modes(scene, v, idx, q, Ks, want=None):
    """both modes of the device against the brute force for every K of `Ks`; `want`: {K: near_lists(...)} computed before"""
    for K in Ks:
        rec, count_all, count_nearest = want[K] if want else nr.near_lists(v, idx, q, K)
        got, cnt = device_lists(scene, q, K, False)
        assert_same(cnt, count_all, f"ALL K={K} counts")
        assert_same(got, rec, f"ALL K={K}")
        if K > 0:
            got, cnt = device_lists(scene, q, K, True)
            assert_same(cnt, count_nearest, f"NEAREST K={K} counts")
            assert_same(got, rec, f"NEAREST K={K}")


_dragon_cache = {}
DRAGON_KS = (0, 1, 8, 32)


def dragon_case():
    """the 2 k mesh in its Cornell box, 1024 queries with per-query radii and the brute force for DRAGON_KS: computed once, shared, never
    written (1024 x 2012 pairs)"""
    if not _dragon_cache:
        v, idx = mesh_of(dragon())
        rng = np.random.default_rng(31)
        lo, hi = bound_of(v)
        pts = np.concatenate([uniform_in(lo, hi, 512, rng), surface_samples(v, idx, 512, rng, 1e-3)])
        q = queries_of(pts, rng.choice([0.02, 0.1, 0.3, 1.0, np.inf], len(pts)))
        rec, count, _ = nr.near_lists(v, idx, q, max(DRAGON_KS))   # the cut is the only thing K changes
        want = {K: (np.ascontiguousarray(rec[:, :K]), count, np.minimum(count, K).astype(np.int32)) for K in DRAGON_KS}
        for x in (v, idx, q) + tuple(a for w in want.values() for a in w):
            x.setflags(write=False)
        _dragon_cache.update(v=v, idx=idx, q=q, want=want)
    return _dragon_cache


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_near_device", "gnxr_near_counted_device", "gnxr_near"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.PointQuery) == 16 and C.sizeof(gx._abi.ClosestPoint) == 32 and nr.RECORD.itemsize == 32
    assert gx.CLOSEST_DTYPE == nr.RECORD
    assert gx.NEAR_MAX == 32 == nr.NEAR_MAX and (gx._abi.NEAR_ALL, gx._abi.NEAR_NEAREST) == (0, 1)
    assert gx._abi.GNXR_ABI_VERSION == 5 and gx._abi.PointQuery not in gx._abi.ABI_STRUCTS and gx._abi.ClosestPoint not in gx._abi.ABI_STRUCTS
    assert gx.NearLists._fields == ("count", "records", "prim", "dist2", "p", "b1", "b2", "feature")


def test_restatement_exact_cases():
    """Triangle (0,0,0), (4,0,0), (0,4,0) and points with small integer coordinates: every value is exactly representable."""
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F)
    one = np.array([(0, 1, 2)], np.int32)
    # face, edge and vertex distances: (1, 1, 3) is 3 over the face, (2, -3, 0) is 3 beyond edge ab, (-1, -2, 2) is 3 beyond vertex a
    for p, feature, closest in (((1, 1, 3), 0, (1, 1, 0)), ((2, -3, 0), 1, (2, 0, 0)), ((-1, -2, 2), 4, (0, 0, 0))):
        root = F(3)
        md = [root, np.nextafter(root, F(0)), np.nextafter(root, INF), INF, F(0), F(-1), F(np.nan)]
        rec, count, count_nearest = nr.near_lists(v, one, queries_of(np.array([p] * len(md), F), md), 2)
        # exactly at sqrt(dist2): near; one ulp below: not; one ulp above: near
        assert list(count) == [1, 0, 1, 1, 0, 0, 0] and list(count_nearest) == list(count)
        for r, c in zip(rec, count):
            assert r[1].tobytes() == EMPTY.tobytes()
            if c:
                assert r[0]["prim"] == 0 and r[0]["dist2"] == 9 and tuple(r[0]["p"]) == closest and r[0]["feature"] == feature
            else:
                assert r[0].tobytes() == EMPTY.tobytes()
    # the record is closest_points' record
    q = queries_of(np.array([(1, 1, 3), (6, -1, 0), (4, 4, 0)], F))
    assert nr.near_lists(v, one, q, 1)[0][:, 0].tobytes() == cr.closest_points(v, one, q).tobytes()
    # order and cut: three copies of the triangle and one farther; bit-equal dist2 in authoring order, the count never clamped
    v2 = np.concatenate([v, v + F((0, 0, -1))])
    idx = np.array([(3, 4, 5), (0, 1, 2), (1, 2, 0), (0, 1, 2)], np.int32)
    q = queries_of(np.array([(1, 1, 3)], F), [5.0])
    for K in (0, 1, 2, 3, 4, 6):
        rec, count, count_nearest = nr.near_lists(v2, idx, q, K)
        assert count[0] == 4 and count_nearest[0] == min(4, K) and rec.shape == (1, K)
        assert list(rec["prim"][0]) == [1, 2, 3, 0, -1, -1][:K] and list(rec["dist2"][0]) == [9, 9, 9, 16, INF, INF][:K]
    assert nr.near_lists(v2, idx, queries_of(np.array([(1, 1, 3)], F), [3.5]), 4)[1][0] == 3   # the radius cuts the farther one
    # a bad query point, and no triangles
    rec, count, _ = nr.near_lists(v2, idx, queries_of(np.array([(np.nan, 1, 3)], F)), 2)
    assert count[0] == 0 and all(r.tobytes() == EMPTY.tobytes() for r in rec[0])
    rec, count, _ = nr.near_lists(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), q, 2)
    assert count[0] == 0 and all(r.tobytes() == EMPTY.tobytes() for r in rec[0])
    assert EMPTY["prim"] == -1 and EMPTY["dist2"] == INF and not EMPTY["p"].any() and EMPTY["b1"] == 0 and EMPTY["b2"] == 0 and EMPTY["feature"] == 0


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0, n < 0, max_near out of range for the mode, records that do not go with max_near and unknown
    flag bits are refused before anything is looked at (the handle is a dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    ALL, NEAREST = gx._abi.NEAR_ALL, gx._abi.NEAR_NEAREST
    for fn in (L.gnxr_near_device, lambda s, q, n, k, f, o, c, st: L.gnxr_near_counted_device(s, q, n, k, f, o, c, p, st)):
        assert fn(None, p, 1, 1, ALL, p, p, None) == ERR_INVALID
        assert fn(None, p, 0, 1, ALL, p, p, None) == ERR_INVALID
        assert fn(p, None, 4, 1, ALL, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 1, ALL, None, p, None) == ERR_INVALID       # records missing with max_near > 0
        assert fn(p, p, 4, 1, ALL, p, None, None) == ERR_INVALID
        assert fn(p, p, 4, 0, ALL, p, p, None) == ERR_INVALID          # records set with max_near == 0
        assert fn(p, p, -1, 1, ALL, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 33, ALL, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, -1, ALL, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 33, NEAREST, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 0, NEAREST, None, p, None) == ERR_INVALID   # K = 0 is not a mode of NEAREST
        assert "GNXR_NEAR_NEAREST" in L.gnxr_last_error().decode()
        assert fn(p, p, 0, 33, ALL, p, p, None) == ERR_INVALID         # n == 0 is a no-op only for good arguments
        for flags in (2, 3, 4, 1 << 31):
            assert fn(p, p, 4, 1, flags, p, p, None) == ERR_INVALID
            assert "flags" in L.gnxr_last_error().decode()
    assert L.gnxr_near_counted_device(p, p, 4, 1, ALL, p, p, None, None) == ERR_INVALID
    Q, R, I = (lambda x: C.cast(x, C.POINTER(gx._abi.PointQuery))), (lambda x: C.cast(x, C.POINTER(gx._abi.ClosestPoint))), (lambda x: C.cast(x, C.POINTER(C.c_int32)))
    assert L.gnxr_near(None, Q(p), 1, 1, ALL, R(p), I(p)) == ERR_INVALID
    assert L.gnxr_near(p, None, 1, 1, ALL, R(p), I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 1, ALL, None, I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 1, ALL, R(p), None) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 0, ALL, R(p), I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), -1, 1, ALL, R(p), I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 33, ALL, R(p), I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 0, NEAREST, None, I(p)) == ERR_INVALID
    assert L.gnxr_near(p, Q(p), 1, 1, 2, R(p), I(p)) == ERR_INVALID


def test_python_refuses_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 3) / (n, 4) tensors on the scene's device pass, K is an integer in the mode's range, the radius takes
    closest_point's forms and the launch keywords are `stream` and `counts`; everything else raises before a library call (the handle is
    empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    bad = [np.zeros((4, 3), F), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 5)), torch.zeros((3, 4)).t(), torch.zeros((4, 6))[:, ::2],
           torch.zeros(12), "points", None, torch.zeros((4, 3)), torch.zeros((4, 4))]
    for b in bad:
        with pytest.raises(ValueError):
            s.within(b, None, 4)
        with pytest.raises(ValueError):
            s.count_within(b, None)
        with pytest.raises(ValueError):
            s.nearest(b, 4)
    for call in (lambda: s.within(torch.zeros((4, 4)), 1.0, 4), lambda: s.count_within(torch.zeros((4, 4)), 1.0), lambda: s.nearest(torch.zeros((4, 4)), 4, 1.0)):
        with pytest.raises(ValueError, match="ready-made"):
            call()
    for k in (33, -1):
        with pytest.raises(ValueError):
            s.within(torch.zeros((4, 4)), None, k)
    for k in (33, 0, -1):
        with pytest.raises(ValueError):
            s.nearest(torch.zeros((4, 4)), k)
    for k in (1.5, "4", None, True):
        with pytest.raises(TypeError):
            s.within(torch.zeros((4, 4)), None, k)
        with pytest.raises(TypeError):
            s.nearest(torch.zeros((4, 4)), k)
    for method, args in ((s.within, (torch.zeros((4, 4)), None, 4)), (s.count_within, (torch.zeros((4, 4)), None)), (s.nearest, (torch.zeros((4, 4)), 4))):
        with pytest.raises(ValueError, match="unexpected arguments"):
            method(*args, streams=None)


def test_no_scratch(gx):
    """tools/kernel_regs.py: every instantiation of k_near (wide / binary; ALL with a list, ALL count-only, NEAREST; timed / counting) runs
    without scratch and without spilled VGPRs -- the list lives in the output row, not in a private array"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels(gx.LIB_PATH) if "k_near<" in k["name"]]
    assert len(ks) == 12, [k["name"] for k in ks]
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in ks), ks


# ---------------------------------------------------------------- GPU
def cornell_case():
    """384 points on, near and far from the walls with per-query radii (12 triangles: the brute force is tiny)"""
    b = scenes.cornell()
    v, idx = mesh_of(b)
    rng = np.random.default_rng(41)
    lo, hi = bound_of(v)
    a, bb, c = (v[idx[:, k]] for k in range(3))
    on = np.concatenate([a, bb, c, F(0.5) * (a + bb), (a + bb + c) / F(3)]).astype(F)                       # 60: vertices, edge midpoints, centroids
    pts = np.concatenate([on, surface_samples(v, idx, 100, rng, 1e-3), uniform_in(lo, hi, 124, rng), uniform_in(lo, hi, 100, rng, 3.0)])
    extent = float((hi - lo).max())
    md = rng.choice([0.0, 0.02 * extent, 0.3 * extent, 0.75 * extent, 4 * extent, np.inf], len(pts), p=[0.1, 0.2, 0.15, 0.2, 0.2, 0.15]).astype(F)
    return b, v, idx, queries_of(pts, md)


@pytest.mark.gpu
def test_cornell(gpu, order):
    b, v, idx, q = cornell_case()
    assert len(q) == 384
    want = {K: nr.near_lists(v, idx, q, K) for K in (0, 1, 4, 32)}
    count = want[4][1]
    assert (count > 4).mean() >= 0.25 and (count == 0).mean() >= 0.1 and (count == len(idx)).any()   # lists that overflow, empty ones, everything
    scene = gpu.Scene(b)
    check_both_modes(scene, v, idx, q, (0, 1, 4, 32), want)
    # (n, 3) points with the radius as a tensor, as a number and as None
    pts, md = torch.from_numpy(q[:, 0:3].copy()).cuda(), torch.from_numpy(q[:, 3].copy()).cuda()
    res = scene.within(pts, md, 4)
    near = scene.nearest(pts, 4, max_distance=md)
    only_count = scene.count_within(pts, md)
    one = scene.within(pts, 2.5, 4)
    free = scene.nearest(pts, 4)
    torch.cuda.synchronize()
    as_rec = lambda r: r.records.cpu().numpy().view(nr.RECORD).reshape(len(q), -1)
    assert_same(as_rec(res), want[4][0]); assert_same(res.count.cpu().numpy(), want[4][1])
    assert_same(as_rec(near), want[4][0]); assert_same(near.count.cpu().numpy(), want[4][2])
    assert_same(only_count.cpu().numpy(), want[4][1])
    assert_same(as_rec(one), nr.near_lists(v, idx, queries_of(q[:, 0:3], 2.5), 4)[0])
    assert_same(as_rec(free), nr.near_lists(v, idx, queries_of(q[:, 0:3]), 4)[0])
    # the named views are the records' fields
    w = want[4][0]
    for name in ("prim", "dist2", "p", "b1", "b2", "feature"):
        assert_same(getattr(res, name).cpu().numpy(), w[name], name)


@pytest.mark.gpu
@pytest.mark.parametrize("copies,others", [(1, 0), (2, 0), (1, 3000)])
def test_tie_cut(gpu, order, copies, others):
    """All triangles of the fan are at one bit-equal dist2 from the query beyond the apex: the list must hold the smallest authoring
    indices, in both modes, for K below, at and above the size of the tie group -- with coincident triangles (two copies) and with the
    group spread over several leaves of a tree of 3000 other triangles, where entering a box with bd2 == the K-th dist2 is what decides."""
    v, idx, fan = fan_mesh(np.random.default_rng(50 + copies + others), copies, others)
    q = queries_of(np.array([(0, 0, FAN_D)] * 3 + [(0.25, -0.5, FAN_D + 1)], F), [np.inf, FAN_D, 2 * FAN_D, np.inf])
    dist2, _, _, _, feature = cr.closest_on_triangle(v[idx[fan, 0]], v[idx[fan, 1]], v[idx[fan, 2]], q[0, 0:3])
    assert len(fan) == 12 * copies and (dist2.view(np.uint32) == F(FAN_D * FAN_D).view(np.uint32)).all() and sorted(set(feature)) == [4, 5, 6]
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    for K in (1, 3, 11, 12, 13):
        rec, count_all, count_nearest = nr.near_lists(v, idx, q, K)
        assert list(rec["prim"][1][:min(K, len(fan))]) == list(fan[:K]) and count_all[1] == len(fan)   # radius FAN_D: the fan and nothing else
        assert list(rec["prim"][0][:min(K, len(fan))]) == list(fan[:K])
        for nearest in (False, True):
            got, cnt = device_lists(scene, q, K, nearest)
            assert_same(got, rec, f"K={K} nearest={nearest}")
            assert_same(cnt, count_nearest if nearest else count_all, f"K={K} nearest={nearest} counts")


@pytest.mark.gpu
def test_mode_equivalence(gpu, order):
    case = dragon_case()
    scene = gpu.Scene(dragon())
    q = torch.from_numpy(case["q"].copy()).cuda()
    for K in (1, 8, 32):
        work_all, work_nearest = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        a = scene.within(q, None, K, counts=work_all)
        b = scene.nearest(q, K, counts=work_nearest)
        torch.cuda.synchronize()
        assert_same(b.records.cpu().numpy(), a.records.cpu().numpy(), f"K={K}")
        assert_same(b.count.cpu().numpy(), np.minimum(a.count.cpu().numpy(), K).astype(np.int32), f"K={K} counts")
        assert_same(a.count.cpu().numpy(), case["want"][K][1]); assert_same(a.records.cpu().numpy().view(nr.RECORD).reshape(len(q), K), case["want"][K][0])
        nodes_all, tris_all = (int(x) for x in work_all.cpu())
        nodes_nearest, tris_nearest = (int(x) for x in work_nearest.cpu())
        assert len(q) <= nodes_nearest <= nodes_all, (K, nodes_nearest, nodes_all)   # NEAREST's bound is never above r2
        assert tris_nearest <= tris_all
    # nearest(points, 1) is closest_point wherever that has a winner
    one = scene.nearest(q, 1)
    cp = scene.closest_point(q)
    torch.cuda.synchronize()
    got, want = one.records.cpu().numpy().view(nr.RECORD).reshape(-1), cp.records.cpu().numpy().view(cr.RECORD).reshape(-1)
    has = want["prim"] >= 0
    assert has.any() and (~has).any()
    assert_same(got[has], want[has])
    assert (got["prim"][~has] == -1).all() and all(r.tobytes() == EMPTY.tobytes() for r in got[~has])
    assert_same(one.count.cpu().numpy(), has.astype(np.int32))


@pytest.mark.gpu
def test_radius_on_the_ulp(gpu, order):
    """Ready-made records whose max_distance squares to a tie group's dist2 exactly, and the next float below: the count changes by
    exactly the size of the group (the fan's 12 triangles at dist2 = 2.25 = 1.5^2, among 3000 others)."""
    v, idx, fan = fan_mesh(np.random.default_rng(60), 1, 3000)
    at, below = F(FAN_D), np.nextafter(F(FAN_D), F(0))
    assert at * at == F(2.25) and below * below < F(2.25)
    q = queries_of(np.array([(0, 0, FAN_D)] * 2, F), [at, below])
    rec, count, _ = nr.near_lists(v, idx, q, 16)
    assert count[0] - count[1] == len(fan) == 12 and count[1] == 0
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    check_both_modes(scene, v, idx, q, (0, 16))
    # the same on the dragon: per query the radius at and one ulp below the root of its 5th dist2 where that root squares back exactly
    case = dragon_case()
    d5 = nr.near_lists(case["v"], case["idx"], queries_of(case["q"][:, 0:3]), 5)[0]["dist2"][:, 4]
    root = np.sqrt(d5)
    exact = root * root == d5
    assert exact.sum() >= 50
    pts = case["q"][exact, 0:3]
    q2 = np.concatenate([queries_of(pts, root[exact]), queries_of(pts, np.nextafter(root[exact], F(0)))])
    count2 = nr.near_lists(case["v"], case["idx"], q2, 0)[1]
    m = int(exact.sum())
    assert (count2[:m] >= 5).all() and (count2[m:] < count2[:m]).all()
    check_both_modes(gpu.Scene(dragon()), case["v"], case["idx"], q2, (0, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts"])
def test_split_methods(gpu, split, order):
    """records and counts do not depend on the tree: every split method gives the brute force's bytes (and so the four runs are identical)"""
    case = dragon_case()
    check_both_modes(gpu.Scene(dragon(split)), case["v"], case["idx"], case["q"], (0, 8), case["want"])


@pytest.mark.gpu
def test_off_the_wide_tree_and_large_leaves(gpu, order):
    rng = np.random.default_rng(9)
    v, idx = concentric_mesh(rng)
    pts = np.concatenate([uniform_in(*bound_of(v), 768, rng, 1.2), surface_samples(v, idx, 256, rng, 1e-3)])
    q = queries_of(pts, rng.choice([0.05, 0.5, 2.0, np.inf], len(pts)))
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    _, meta, _ = scene.bvh()
    assert meta[:, 1].max() > 127   # a leaf the 4-wide encoding cannot hold: the scene is on the binary walk
    check_both_modes(scene, v, idx, q, (0, 4, 32))
    # slivers: boxes that say little, leaves of many triangles
    v, idx = sliver_mesh(rng)
    pts = np.concatenate([uniform_in(*bound_of(v), 768, rng), surface_samples(v, idx, 256, rng, 1e-3)])
    q = queries_of(pts, rng.choice([0.05, 0.5, 2.0, np.inf], len(pts)))
    check_both_modes(gpu.Scene(mesh_scene(gpu, v, idx)), v, idx, q, (0, 4, 32))
    # a scene kept on the binary tree by the creation switch
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        binary = gpu.Scene(dragon())
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    case = dragon_case()
    check_both_modes(binary, case["v"], case["idx"], case["q"], (0, 8), case["want"])


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_deep_tree_spills(gpu, order, binary):
    """chain_scene(36): from points beyond the smallest triangle the walk descends the whole chain with a sibling on its stack per level.
    With the default LDS levels on the 4-wide tree, where the tree's need exceeds them, and forced onto 2 LDS levels through
    GNXR_NEAR_LDS_LEVELS on the 4-wide and on the binary tree: the LDS levels and the global spill together, with both entry sizes."""
    b = chain_scene(gpu)
    v, idx = mesh_of(b)
    rng = np.random.default_rng(8)
    x = (2.0 ** -35) * rng.uniform(-2, 1, 1024)
    pts = np.stack([x, rng.normal(0, 2.0 ** -36, 1024), rng.normal(0, 2.0 ** -36, 1024)], axis=1).astype(F)
    pts = np.concatenate([pts, uniform_in(*bound_of(v), 512, rng, 1.5)])
    q = queries_of(pts, rng.choice([2.0 ** -30, 2.0 ** -8, 0.25, np.inf], len(pts)))
    want = {K: nr.near_lists(v, idx, q, K) for K in (0, 3, 32)}
    assert (want[32][1] == 36).sum() > 100 and (want[32][1] > 32).sum() > 100
    if binary:
        os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(b)
    finally:
        os.environ.pop("GNXR_BINARY_BVH", None)
    if not binary:
        assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
        check_both_modes(scene, v, idx, q, (0, 3, 32), want)
    os.environ["GNXR_NEAR_LDS_LEVELS"] = "2"
    try:
        check_both_modes(scene, v, idx, q, (0, 3, 32), want)
    finally:
        del os.environ["GNXR_NEAR_LDS_LEVELS"]


@pytest.mark.gpu
def test_live_scene(gpu, order):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    SkinnedMesh.pose -> the brute force over the vertices it holds; set_geometry with another triangle count -> over the new mesh"""
    case = dragon_case()
    b = dragon()
    v, idx = mesh_of(b)
    q = case["q"][::2]
    scene = gpu.Scene(b)
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(0.15) * np.sin(F(5) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    scene.update_vertices(torch.from_numpy(v2[:n_mesh_v].copy()).cuda())
    want2 = {K: nr.near_lists(v2, idx, q, K) for K in (0, 8)}
    assert want2[8][0].tobytes() != nr.near_lists(v, idx, q, 8)[0].tobytes()
    check_both_modes(scene, v2, idx, q, (0, 8), want2)
    scene.rebuild_bvh()
    check_both_modes(scene, v2, idx, q, (0, 8), want2)
    # two bones that blend along the mesh's height
    rest = v2[:n_mesh_v]
    h = (rest[:, 1] - rest[:, 1].min()) / (rest[:, 1].max() - rest[:, 1].min())
    bw = np.stack([h, 1 - h, np.zeros(n_mesh_v), np.zeros(n_mesh_v)], 1).astype(F)
    bi = np.tile(np.array([0, 1, 0, 0], np.int32), (n_mesh_v, 1))
    ca, sa = np.cos(0.6), np.sin(0.6)
    bones = np.stack([np.array([[ca, 0, sa, 0.1], [0, 1, 0, 0.2], [-sa, 0, ca, 0]]), np.eye(3, 4)]).astype(F)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sk = gpu.SkinnedMesh(scene, v2, dev(rest), dev(bi), dev(bw), first_vertex=0, normals=False)
    sk.pose(dev(bones))
    torch.cuda.synchronize()
    v3 = sk.vertices.cpu().numpy()
    assert v3.tobytes() != v2.tobytes() and v3[n_mesh_v:].tobytes() == v2[n_mesh_v:].tobytes()
    check_both_modes(scene, v3, idx, q, (0, 8))
    rng = np.random.default_rng(11)
    v4 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v4[1::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    v4[2::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    idx4 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    scene.set_geometry(v4, idx4, np.zeros(300, np.int32), tri_light=tri_light)
    check_both_modes(scene, v4, idx4, q, (0, 8))


@pytest.mark.gpu
def test_degenerate_input(gpu, order):
    rng = np.random.default_rng(10)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    idx = np.arange(60, dtype=np.int32).reshape(-1, 3)
    v[3:6] = [(0, 0, 0), (0.5, 0.5, 0.5), (1, 1, 1)]          # zero area: three collinear vertices
    v[10] = v[9]                                               # two coincident vertices
    v[12:15] = v[12]                                           # zero area: one point
    pts = np.concatenate([uniform_in(*bound_of(v), 700, rng, 1.5), surface_samples(v, idx, 200, rng, 1e-4),
                          np.linspace((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 64).astype(F)])   # along the collinear triangle
    bad = uniform_in(*bound_of(v), 32, rng)
    bad[0:8, 0] = np.nan; bad[8:12, 2] = np.nan
    bad[12:18, 0] = np.inf; bad[18:24, 1] = -np.inf; bad[24:28] = np.inf; bad[28:32, 2] = -np.inf
    md = rng.choice([0.3, 1.0, np.inf], len(pts) + len(bad)).astype(F)
    md[:40] = [-1, np.nan, 0, -0.0] * 10                      # negative, NaN and zero radius (and -0: not < 0, r2 = 0)
    q = queries_of(np.concatenate([pts, bad]), md)
    want = nr.near_lists(v, idx, q, 32)
    assert (want[1][len(pts):len(pts) + 12] == 0).all() and (want[1][0:40:4] == 0).all() and (want[1][1:40:4] == 0).all()
    assert (want[1] == 20).any() or (want[1] == 19).any()
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    check_both_modes(scene, v, idx, q, (0, 5, 32))
    # a point ON a triangle with radius 0 finds it
    on = queries_of(v[idx[:, 0]], 0.0)
    assert (nr.near_lists(v, idx, on, 1)[1] >= 1).all()
    check_both_modes(scene, v, idx, on, (0, 2))
    # Every scene has a triangle: scene creation refuses a description without one (the restatement's answer without triangles, counts 0
    # and empty slots, is asserted in test_restatement_exact_cases; the library has no such path) ...
    b = gpu.SceneBuilder()
    b.AddSphere((0, 0, 0), 1.0, b.MatteMaterial(scenes.WHITE, 60.0))
    b.AddSkyLight()
    with pytest.raises(gpu.GnxrError, match="no geometry"):
        gpu.Scene(b)
    # ... and a sphere beside triangles is not considered: points on and inside the sphere of cornell_sphere get the walls' answer
    b = scenes.cornell_sphere("matte", center=(0.6, -1.5, 0.2), radius=1.0)
    v, idx = mesh_of(b)
    d = rng.normal(0, 1, (256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (np.array((0.6, -1.5, 0.2)) + d * rng.choice([0.0, 0.5, 1.0, 1.0 + 1e-4], (256, 1))).astype(F)
    ball = gpu.Scene(b)
    assert ball.n_triangles == len(idx)
    check_both_modes(ball, v, idx, queries_of(pts, rng.choice([0.25, 1.0, np.inf], len(pts))), (0, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_batch_sizes_and_out(gpu, n, order):
    case = dragon_case()
    scene = gpu.Scene(dragon())
    q = torch.from_numpy(case["q"][:n].copy()).cuda()
    rec, count_all, count_nearest = (x[:n] for x in case["want"][8])
    for nearest in (False, True):
        out = torch.full((n, 8, 8), 7.0, device="cuda")
        counts_out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        res = scene.nearest(q, 8, out=out, counts_out=counts_out) if nearest else scene.within(q, None, 8, out=out, counts_out=counts_out)
        torch.cuda.synchronize()
        assert res.records is out and res.count is counts_out and out.shape == (n, 8, 8)
        assert_same(out.cpu().numpy().view(nr.RECORD).reshape(n, 8), rec)
        assert_same(counts_out.cpu().numpy(), count_nearest if nearest else count_all)
        # the host-array form equals the device form
        h_rec, h_cnt = scene.Near(case["q"][:n], 8, nearest=nearest)
        assert_same(h_rec.view(nr.RECORD), rec); assert_same(h_cnt, count_nearest if nearest else count_all)
    h_rec, h_cnt = scene.Near(case["q"][:n], 0)
    assert h_rec.shape == (n, 0) and (h_cnt == count_all).all()
    assert scene.count_within(q, None).shape == (n,)
    with pytest.raises(ValueError):
        scene.within(q, None, 8, out=torch.zeros((n + 1, 8, 8), device="cuda"))
    with pytest.raises(ValueError):
        scene.nearest(q, 8, counts_out=torch.zeros((n,), dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
def test_stream(gpu, order):
    """Queries written by torch on a side stream, answered there and reduced there with no synchronise in between"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    src = torch.from_numpy(case["q"].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q = src * 1.0
        res = scene.within(q, None, 8, stream=side)
        near = scene.nearest(q, 8, stream=side)
        total = res.count.to(torch.int64).sum() + near.prim.to(torch.int64).sum()
    side.synchronize()
    rec, count_all, _ = case["want"][8]
    assert int(total) == int(count_all.astype(np.int64).sum() + rec["prim"].astype(np.int64).sum())
    assert_same(res.records.cpu().numpy().view(nr.RECORD).reshape(len(q), 8), rec)
    assert_same(near.records.cpu().numpy().view(nr.RECORD).reshape(len(q), 8), rec)


@pytest.mark.gpu
def test_one_binned_batch(gpu):
    """65536 queries, the first size a call bins by itself, against the same call in caller order (binning switched off), and the brute
    force on a 512-query subset (512 x 2012 pairs)."""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    rng = np.random.default_rng(70)
    pts = np.concatenate([uniform_in(*bound_of(case["v"]), 32768, rng), surface_samples(case["v"], case["idx"], 32768, rng, 1e-2)])
    q_host = queries_of(pts, rng.choice([0.05, 0.2, 0.6, np.inf], len(pts)))
    q = torch.from_numpy(q_host).cuda()
    binned = [scene.within(q, None, 8), scene.nearest(q, 8)]
    torch.cuda.synchronize()
    os.environ["GNXR_CLOSEST_BIN_MIN"] = str(1 << 62)
    try:
        plain = [scene.within(q, None, 8), scene.nearest(q, 8)]
        torch.cuda.synchronize()
    finally:
        del os.environ["GNXR_CLOSEST_BIN_MIN"]
    for a, b in zip(binned, plain):
        assert torch.equal(a.records.view(torch.int32), b.records.view(torch.int32)) and torch.equal(a.count, b.count)
    pick = rng.choice(len(q_host), 512, replace=False)
    rec, count_all, count_nearest = nr.near_lists(case["v"], case["idx"], q_host[pick], 8)
    for res, cnt in zip(binned, (count_all, count_nearest)):
        assert_same(res.records.cpu().numpy().view(nr.RECORD).reshape(len(q_host), 8)[pick], rec)
        assert_same(res.count.cpu().numpy()[pick], cnt)


@pytest.mark.gpu
def test_second_binned_launch(gpu):
    """2^22 + 257 queries: a binned call walks 2^22 per launch, so the second launch starts at query 2^22 and its rows at 2^22 K.  The
    queries tile cornell_case's 384 and the expectation tiles their brute force; both stay on the device (the records are 268 MB) and
    are compared there, on bits."""
    b, v, idx, q = cornell_case()
    n, K = (1 << 22) + 257, 2
    rec, count, _ = nr.near_lists(v, idx, q, K)
    tile = torch.arange(n, device="cuda") % len(q)
    want_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(len(q), K, 8)).cuda()[tile]
    want_count = torch.from_numpy(count).cuda()[tile]
    res = gpu.Scene(b).within(torch.from_numpy(q).cuda()[tile], None, K)
    torch.cuda.synchronize()
    assert res.records.shape == (n, K, 8) and torch.equal(res.records.view(torch.int32), want_rec)
    assert res.count.dtype == torch.int32 and torch.equal(res.count, want_count)


@pytest.mark.gpu
def test_refusals(gpu):
    """K out of range per mode, misaligned pointers, host memory, a negative n, unknown flags and an array that runs past its allocation
    give GNXR_ERR_INVALID with a message before anything is queued; wrong tensors and keywords raise; the scene still answers afterwards"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    L = gpu.lib()
    q = torch.from_numpy(case["q"].copy()).cuda()
    out = torch.zeros((len(q), 8, 8), device="cuda")
    cnt = torch.zeros(len(q), dtype=torch.int32, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.gnxr_last_error().decode()
    near = lambda *a: L.gnxr_near_device(scene._h, *a)
    assert near(P(q, 4), 100, 8, 0, P(out), P(cnt), None) == ERR_INVALID and "d_queries is not 16-byte aligned" in err()
    assert near(P(q), 100, 8, 0, P(out, 8), P(cnt), None) == ERR_INVALID and "d_out is not 16-byte aligned" in err()
    assert near(P(q), 100, 8, 0, P(out), P(cnt, 2), None) == ERR_INVALID and "d_counts is not 4-byte aligned" in err()
    assert near(P(q), -1, 8, 0, P(out), P(cnt), None) == ERR_INVALID
    assert near(P(q), 100, 33, 0, P(out), P(cnt), None) == ERR_INVALID and "max_near" in err()
    assert near(P(q), 100, 0, 1, None, P(cnt), None) == ERR_INVALID and "max_near" in err()
    assert near(P(q), 100, 0, 0, P(out), P(cnt), None) == ERR_INVALID and "count-only" in err()
    assert near(P(q), 100, 8, 2, P(out), P(cnt), None) == ERR_INVALID and "flags" in err()
    host = np.zeros((100, 64), F)
    assert near(C.c_void_p(host.ctypes.data), 100, 8, 0, P(out), P(cnt), None) == ERR_INVALID and "d_queries is not device memory" in err()
    assert near(P(q), 100, 8, 0, C.c_void_p(host.ctypes.data), P(cnt), None) == ERR_INVALID and "d_out is not device memory" in err()
    assert near(P(q), 100, 8, 0, P(out), C.c_void_p(host.ctypes.data), None) == ERR_INVALID and "d_counts is not device memory" in err()
    lone = torch.zeros((64, 4), device="cuda")
    assert near(P(lone), 1 << 20, 8, 0, P(out), P(cnt), None) == ERR_INVALID and "d_queries" in err()
    many = torch.zeros((1 << 20, 4), device="cuda")
    assert near(P(many), 1 << 20, 8, 0, P(out), P(cnt), None) == ERR_INVALID and "d_out" in err()   # 2^20 rows of 8 records: far past out's allocation
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.gnxr_near_counted_device(scene._h, P(q), 100, 8, 0, P(out), P(cnt), P(work, 4), None) == ERR_INVALID and "d_work" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (cnt == 0).all() and (work == 0).all()   # nothing was queued by the refused calls
    for bad in (q.double(), q.cpu(), q[:, :2].contiguous(), q.t(), case["q"]):
        with pytest.raises(ValueError):
            scene.within(bad, None, 8)
        with pytest.raises(ValueError):
            scene.nearest(bad, 8)
    p3 = q[:, 0:3].contiguous()
    with pytest.raises(ValueError):
        scene.within(p3, torch.zeros(5, device="cuda"), 8)
    with pytest.raises(TypeError):
        scene.within(p3, "far", 8)
    for k in (33, -1):
        with pytest.raises(ValueError):
            scene.within(q, None, k)
    for k in (33, 0):
        with pytest.raises(ValueError):
            scene.nearest(q, k)
    with pytest.raises(ValueError, match="unexpected arguments"):
        scene.nearest(q, 8, streams=None)
    with pytest.raises(ValueError):
        scene.within(q, None, 8, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    check_both_modes(scene, case["v"], case["idx"], case["q"], (8,), case["want"])
