"""Triangle overlap queries (include/gnxr.h, "Triangle overlap queries"): the numpy restatement (tests/overlap_tri_reference.py) on hand-made
exact cases and against an independent float64 separating-axis check, the refusals of the C calls and of the Python methods without a
device, then gnxr_overlap_tri_device / gnxr_overlap_tri, Scene.overlap_triangles and Scene.self_intersections on the GPU against the
restatement's brute force over all triangles.  Every comparison of rows, CSR lists and counts is on their bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import overlap_reference as orf
import overlap_tri_reference as otr
from conftest import ROOT
from overlap_tri_cases import ALL_PAIRS, LONE_SEPARATOR, ONE, check_mix, pairs_by_triangle, self_case, tri_case
from query_cases import assert_same, bound_of, chain_scene, dragon, fan_mesh, mesh_of, mesh_scene

ERR_INVALID = -1
F = np.float32
CANARY = -7
SKIP, SELF = 1, 2


# ---------------------------------------------------------------- helpers
def dev(x):
    return torch.from_numpy(np.array(x)).cuda()   # a copy: the shared cases are read-only


def device_rows(scene, queries, K, **kw):
    res = scene.overlap_triangles(dev(np.array(queries, F)), K, **kw)
    torch.cuda.synchronize()
    return res.prims.cpu().numpy(), res.count.cpu().numpy()


def device_csr(scene, queries, **kw):
    res = scene.overlap_triangles(dev(np.array(queries, F)), **kw)
    torch.cuda.synchronize()
    return res.offsets.cpu().numpy(), res.prims.cpu().numpy(), res.count.cpu().numpy()


def check_result(res, m, K, what):
    """an OverlapLists (K an integer) or OverlapCSR (K None) against the restatement's matrix `m`"""
    torch.cuda.synchronize()
    assert_same(res.count.cpu().numpy(), orf.counts_of(m), f"{what} K={K} counts")
    if K is not None:
        assert_same(res.prims.cpu().numpy(), orf.rows_of(m, K), f"{what} K={K}")
    else:
        want_offsets, want_prims = orf.csr_of(m)
        assert_same(res.offsets.cpu().numpy(), want_offsets, f"{what} CSR offsets")
        assert_same(res.prims.cpu().numpy(), want_prims, f"{what} CSR")


def check_all_forms(scene, m, queries, Ks=(0, 1, 8, 32), what="", **kw):
    """rows mode for every K of `Ks` and the CSR form against the restatement's matrix `m`"""
    d = dev(np.array(queries, F))
    for K in (*Ks, None):
        check_result(scene.overlap_triangles(d, K, **kw), m, K, what)


def check_self(scene, m, Ks=(4,), what=""):
    for K in (*Ks, None):
        check_result(scene.self_intersections(K), m, K, f"{what} self")


def raw_call(gx, scene, tris, n, flags, max_prims, offsets, prims, counts, work=None, stream=None):
    """gnxr_overlap_tri[_counted]_device on tensors, as the C ABI takes them"""
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L = gx.lib()
    if work is None:
        return L.gnxr_overlap_tri_device(scene._h, P(tris), n, flags, max_prims, P(offsets), P(prims), P(counts), stream)
    return L.gnxr_overlap_tri_counted_device(scene._h, P(tris), n, flags, max_prims, P(offsets), P(prims), P(counts), P(work), stream)


def binary_scene(gx, b):
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        return gx.Scene(b)
    finally:
        os.environ.pop("GNXR_BINARY_BVH", None)


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_overlap_tri_device", "gnxr_overlap_tri_counted_device", "gnxr_overlap_tri"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.TriQuery) == 48
    assert gx._abi.GNXR_ABI_VERSION == 5 and gx.lib().gnxr_abi_version() == 5 and gx._abi.TriQuery not in gx._abi.ABI_STRUCTS
    assert (gx.OVERLAP_TRI_SKIP_SHARED, gx.OVERLAP_TRI_SELF) == (1, 2) == (otr.SKIP_SHARED, otr.SELF)
    hdr = open(os.path.join(ROOT, "include", "gnxr.h")).read()
    assert "#define GNXR_OVERLAP_TRI_SKIP_SHARED 1u" in hdr and "#define GNXR_OVERLAP_TRI_SELF        2u" in hdr


@pytest.mark.parametrize("case", ALL_PAIRS, ids=[c[0] for c in ALL_PAIRS])
def test_restatement_exact_cases(case):
    """Pairs of triangles of small integer coordinates: contacts (a vertex on a face, an edge through a face, coplanar pairs touching in a
    point and nested), the same one ulp apart and one ulp past, disjoint pairs inside each other's bounds, points, segments and
    non-finite queries (tests/overlap_tri_cases.py has the arithmetic of each)."""
    _, q, tri, want = case
    m = otr.overlap_matrix(np.array(tri, F), ONE, otr.tri_records(np.array([q], F)))
    assert m.shape == (1, 1) and int(m[0, 0]) == want
    assert list(orf.counts_of(m)) == [want] and list(orf.rows_of(m, 2)[0]) == ([0, -1] if want else [-1, -1])


@pytest.mark.parametrize("case", LONE_SEPARATOR, ids=[c[0] for c in LONE_SEPARATOR])
def test_each_axis_group_is_a_lone_separator(case):
    """one pair per group of step 5's axes that ONLY that group separates, and that the bounds test lets through: an implementation that
    drops the group reports the pair"""
    group, q, tri = case
    sep = otr.groups_separate(q, tri)
    assert sep == tuple(g == group for g in otr.GROUPS), sep
    q, tri = np.array(q, F), np.array(tri, F)
    assert (tri.min(axis=0) <= q.max(axis=0)).all() and (tri.max(axis=0) >= q.min(axis=0)).all()
    assert not otr.overlap_matrix(tri, ONE, otr.tri_records(q[None])).any()


def test_restatement_order_cuts_and_skip():
    """three coincident copies of one triangle and one other: the prims ascend, a short row holds the smallest, the count is never
    clamped; with the skip rule a triangle queried against a scene that holds itself and its edge neighbours reports none of them, and
    the one that only crosses it stays; a query with a coordinate that is not finite reports nothing"""
    tri = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F)
    v = np.concatenate([tri, tri + F((0, 0, 1))])
    idx = np.array([(3, 4, 5), (0, 1, 2), (1, 2, 0), (2, 0, 1)], np.int32)
    queries = otr.tri_records(np.array([[(1, 1, -1), (1, 1, 0.5), (2, 1, 0.5)], [(1, 1, -1), (1, 1, 2), (2, 1, 2)], [(1, 1, -1), (1, np.inf, 2), (2, 1, 2)]], F))
    m = otr.overlap_matrix(v, idx, queries)
    assert list(orf.counts_of(m)) == [3, 4, 0]
    for K in (0, 1, 2, 3, 4, 6):
        rows = orf.rows_of(m, K)
        assert rows.shape == (3, K) and list(rows[0]) == [1, 2, 3, -1, -1, -1][:K] and list(rows[1]) == [0, 1, 2, 3, -1, -1][:K] and list(rows[2]) == [-1] * K
    offsets, prims = orf.csr_of(m)
    assert list(offsets) == [0, 3, 7, 7] and list(prims) == [1, 2, 3, 0, 1, 2, 3]
    offsets, prims = orf.csr_of(m[:2], np.array([1, 3, 9]), np.full(10, CANARY, np.int32))
    assert list(prims) == [CANARY, 1, 2, 0, 1, 2, 3, -1, -1, CANARY]
    assert not otr.overlap_matrix(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), queries).size
    # a strip of four triangles in z = 0 -- 1 shares an edge with 0 and 2 and a vertex with 3 --, triangle 4 that stands across the edge
    # of 0 and 1, and triangle 5 that touches 1 in the vertex (0, 2, 0) alone, which it holds as a duplicate with -0
    sv = np.array([(0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 0), (4, 0, 0), (4, 2, 0), (1, 1, -1), (1, 1, 1), (1.5, 1.5, 1), (-0.0, 2, 0), (-2, 2, 0), (0, 4, 0)], F)
    sidx = np.array([(0, 1, 2), (1, 3, 2), (1, 4, 3), (4, 5, 3), (6, 7, 8), (9, 10, 11)], np.int32)
    own = otr.tri_records(sv[sidx])
    assert list(np.flatnonzero(otr.overlap_matrix(sv, sidx, own[1:2])[0])) == [0, 1, 2, 3, 4, 5]
    assert list(np.flatnonzero(otr.overlap_matrix(sv, sidx, own[1:2], skip_shared=True)[0])) == [4]
    assert_same(otr.pairs_of(otr.self_matrix(sv, sidx)), np.array([(0, 4), (1, 4)], np.int32))


def test_float64_margin():
    """An independent check that knows only geometry: the separating-axis test of two triangles in float64 on normalised axes, on the
    vertices as they stand (otr.sat_gap64).  A pair the fp32 definition reports must not be separated by more than the margin, a pair
    it rejects must not overlap by more than the margin on every axis.  Measured on the 2 k-triangle mesh with these 1024 mixed
    query triangles (2 019 328 pairs, 150 309 of them past the bounds test, 7 352 overlapping): the largest float64 gap at which the
    two disagree is 0 -- they disagree nowhere: the largest gap of a reported pair is -3.1e-6, the smallest of a rejected one
    +2.7e-8 (3.1e-9 of the scene's diagonal 8.66: a point query that rounding moved off the face it was sampled on, rejected in both
    precisions).  Allowed: 4 x that = 0 of the scene's diagonal, i.e. the two must agree on every pair of the set.  The set must also
    be a mix: more than 0.2 of the queries touch nothing, more than 0.03 touch over 32 triangles, more than 0.1 between 1 and 7
    (measured 0.43 / 0.063 / 0.38)."""
    case = tri_case()
    v, idx, queries, m = case["v"], case["idx"], case["queries"], case["m"]
    check_mix(case["count"])
    margin = 4 * 0.0 * float(np.linalg.norm(np.subtract(*bound_of(v)[::-1])))
    # pairs apart along a coordinate axis need no arithmetic in either precision: the comparisons are exact.  The others go to float64.
    tri = v[idx].astype(np.float64)
    qlo, qhi = (x.astype(np.float64) for x in otr.query_bounds(queries))
    near = otr.tri_valid(queries)[:, None] & ((tri.min(axis=1)[None] <= qhi[:, None]) & (tri.max(axis=1)[None] >= qlo[:, None])).all(axis=2)
    assert not (m & ~near).any()
    qi, ti = np.nonzero(near)
    gap = otr.sat_gap64(v, idx, queries, qi, ti)
    said = m[qi, ti]
    print(f"pairs {m.size}, past the bounds test {len(qi)}, overlapping {int(said.sum())}, smallest |gap| {np.abs(gap).min():.3e}, "
          f"largest gap of a reported pair {gap[said].max():.3e}, smallest of a rejected one {gap[~said].min():.3e}")
    assert (gap[said] <= margin).all()
    assert (gap[~said] >= -margin).all()


def test_self_case_folds():
    """the deformation of the self-intersection tests folds between 5 % and 60 % of the 2 k scene's triangles through others, by the
    restatement; the rows of the result are cut at K = 4 somewhere"""
    s, idx = self_case(), tri_case()["idx"]
    involved = (s["bent"].any(axis=0) | s["bent"].any(axis=1)).mean()
    print(f"at rest {int(s['rest'].sum())} directed pairs, deformed {int(s['bent'].sum())}, involved {involved:.3f}")
    assert 0.05 < involved < 0.6 and s["bent"].sum(axis=1).max() > 4 and s["bent"].shape == (len(idx), len(idx))


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0, n < 0, an unknown flag bit, SELF with a triangle array, max_prims out of range, rows that
    do not go with max_prims and a max_prims that does not go with the offsets are refused before anything is looked at (the handle is
    a dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    err = lambda: L.gnxr_last_error().decode()
    for fn in (L.gnxr_overlap_tri_device, lambda s, t, n, f, k, o, r, c, st: L.gnxr_overlap_tri_counted_device(s, t, n, f, k, o, r, c, p, st)):
        for flags in (0, SKIP):
            assert fn(None, p, 1, flags, 1, None, p, p, None) == ERR_INVALID
            assert fn(None, p, 0, flags, 1, None, p, p, None) == ERR_INVALID
            assert fn(p, None, 4, flags, 1, None, p, p, None) == ERR_INVALID      # queries missing without SELF
            assert fn(p, p, 4, flags, 1, None, None, p, None) == ERR_INVALID      # rows missing with max_prims > 0
            assert fn(p, p, 4, flags, 1, None, p, None, None) == ERR_INVALID
            assert fn(p, p, 4, flags, 0, None, p, p, None) == ERR_INVALID and "count-only" in err()
            assert fn(p, p, -1, flags, 1, None, p, p, None) == ERR_INVALID
            assert fn(p, p, 4, flags, 33, None, p, p, None) == ERR_INVALID and "max_prims" in err()
            assert fn(p, p, 4, flags, -2, None, p, p, None) == ERR_INVALID and "max_prims" in err()
            assert fn(p, p, 4, flags, -1, None, p, p, None) == ERR_INVALID and "CSR" in err()      # -1 without offsets
            for k in (0, 1, 32, -2):
                assert fn(p, p, 4, flags, k, p, p, p, None) == ERR_INVALID and "CSR" in err()      # offsets with anything but -1
            assert fn(p, p, 4, flags, -1, p, None, p, None) == ERR_INVALID                         # CSR rows without an array
            assert fn(p, p, 0, flags, 33, None, p, p, None) == ERR_INVALID                         # n == 0 is a no-op only for good arguments
        for flags in (4, 8, 1 << 31, 7):
            assert fn(p, p, 4, flags, 1, None, p, p, None) == ERR_INVALID and "flags" in err()
            assert fn(p, p, 0, flags, 1, None, p, p, None) == ERR_INVALID and "flags" in err()
        for flags in (SELF, SELF | SKIP):
            assert fn(p, p, 4, flags, 1, None, p, p, None) == ERR_INVALID and "SELF" in err() and "NULL" in err()
            assert fn(p, None, 4, flags, 1, None, p, None, None) == ERR_INVALID   # SELF needs no queries, but counts
    assert L.gnxr_overlap_tri_counted_device(p, p, 4, 0, 1, None, p, p, None, None) == ERR_INVALID
    T, I, O = (lambda x: C.cast(x, C.POINTER(gx._abi.TriQuery))), (lambda x: C.cast(x, C.POINTER(C.c_int32))), (lambda x: C.cast(x, C.POINTER(C.c_int64)))
    assert L.gnxr_overlap_tri(None, T(p), 1, 0, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, None, 1, 0, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, 1, None, None, I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, 1, None, I(p), None) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, 0, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), -1, 0, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, 33, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, -1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 0, 4, O(p), I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_tri(p, T(p), 1, 4, 1, None, I(p), I(p)) == ERR_INVALID and "flags" in err()
    assert L.gnxr_overlap_tri(p, T(p), 1, SELF, 1, None, I(p), I(p)) == ERR_INVALID and "SELF" in err()
    off = (C.c_int64 * 3)(4, 2, 8)
    assert L.gnxr_overlap_tri(p, T(p), 2, 0, -1, off, I(p), I(p)) == ERR_INVALID and "ascend" in err()
    off = (C.c_int64 * 3)(-1, 2, 8)
    assert L.gnxr_overlap_tri(p, T(p), 2, 0, -1, off, I(p), I(p)) == ERR_INVALID and "negative" in err()


def test_python_refuses_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 12) records, (n, 3, 3) or (n, 9) corners or a (vertices, indices) pair on the scene's device pass,
    max_prims is None or an integer in range, the launch keywords are `stream` and `counts`, pairs go with the complete lists;
    everything else raises before a library call (the handle is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_triangles = None, 0, 4
    bad = [np.zeros((4, 12), F), torch.zeros((4, 12), dtype=torch.float64), torch.zeros((4, 5)), torch.zeros((12, 4)).t(), torch.zeros((4, 24))[:, ::2],
           torch.zeros(12), "tris", None, torch.zeros((4, 12)), torch.zeros((4, 3, 3)), torch.zeros((4, 9)), torch.zeros((4, 3)),
           (torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)), (np.zeros((4, 3), F), np.zeros((2, 3), np.int32))]
    for b in bad:
        for call in (lambda: s.overlap_triangles(b, 4), lambda: s.overlap_triangles(b), lambda: s.count_overlapping_triangles(b), lambda: s.overlap_triangles(b, 4, True)):
            with pytest.raises(ValueError, match="overlap_triangles|count_overlapping_triangles"):
                call()
    for b in bad[:8] + [torch.zeros((4, 12)), torch.zeros((4, 3))]:
        with pytest.raises(ValueError, match="triangle_queries"):
            gx.triangle_queries(b)
    with pytest.raises(ValueError, match="triangle_queries: vertices"):
        gx.triangle_queries(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="triangle_queries: unexpected arguments"):
        gx.triangle_queries(torch.zeros((4, 9)), streams=None)
    for k in (33, -1):
        with pytest.raises(ValueError, match="overlap_triangles: max_prims"):
            s.overlap_triangles(torch.zeros((4, 12)), k)
        with pytest.raises(ValueError, match="self_intersections: max_prims"):
            s.self_intersections(k)
    for k in (1.5, "4", True):
        with pytest.raises(TypeError, match="overlap_triangles: max_prims"):
            s.overlap_triangles(torch.zeros((4, 12)), k)
    with pytest.raises(ValueError, match="overlap_triangles: .*out must be None"):
        s.overlap_triangles(torch.zeros((4, 12)), None, out=torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="self_intersections: pairs"):
        s.self_intersections(4, pairs=True)
    for method, args in ((s.overlap_triangles, (torch.zeros((4, 12)), 4)), (s.count_overlapping_triangles, (torch.zeros((4, 12)),)), (s.self_intersections, ())):
        with pytest.raises(ValueError, match="unexpected arguments"):
            method(*args, streams=None)


def test_no_scratch(gx):
    """tools/kernel_regs.py: every instantiation of k_overlap_tri (wide / binary; count-only / rows; timed / counting; caller's queries /
    the scene's own) runs without scratch and without spilled VGPRs -- the list lives in the output row, the query in registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels(gx.LIB_PATH) if "k_overlap_tri<" in k["name"]]
    assert len(ks) == 16, [k["name"] for k in ks]
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in ks), ks


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_one_pair_scenes(gpu):
    """every hand-made pair on the device, in rows mode at K = 0, 1 and 2 and in CSR mode"""
    for tri, (queries, want, names) in pairs_by_triangle().items():
        v = np.array(tri, F)
        m = otr.overlap_matrix(v, ONE, queries)
        assert list(orf.counts_of(m)) == list(want), names
        check_all_forms(gpu.Scene(mesh_scene(gpu, v, ONE)), m, queries, (0, 1, 2), str(tri))


@pytest.mark.gpu
def test_tie_fan(gpu):
    """Twelve triangles round one vertex, among 300 others, and the point-triangle on that vertex: all twelve touch it.  Rows mode cuts to
    the smallest prims; CSR rows that are exact, short, over-long and out of order hold the smallest prims, then -1, and nothing outside
    a row is written (canaries before, behind and, for a call on the middle row alone, in the neighbouring rows).  With the skip rule
    the same query shares the apex with all twelve and reports none."""
    v, idx, fan = fan_mesh(np.random.default_rng(50), 1, 300)
    queries = otr.tri_records(np.zeros((4, 3, 3), F))
    m = otr.overlap_matrix(v, idx, queries)
    assert list(orf.counts_of(m)) == [12] * 4 and list(np.flatnonzero(m[0])) == list(fan) and (np.diff(fan) > 0).all()
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    check_all_forms(scene, m, queries, (0, 5, 12, 13, 32))
    assert list(device_rows(scene, queries, 5)[0][0]) == list(fan[:5])
    d_tris = dev(queries)
    offsets = np.array([3, 15, 20, 40, 36], np.int64)   # exact, short (5), over-long (20), out of order (nothing)
    prims = torch.full((44,), CANARY, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert raw_call(gpu, scene, d_tris, 4, 0, -1, dev(offsets), prims, counts) == 0
    torch.cuda.synchronize()
    want = orf.csr_of(m, offsets, np.full(44, CANARY, np.int32))[1]
    assert list(want[:3]) == [CANARY] * 3 and list(want[3:15]) == list(fan) and list(want[15:20]) == list(fan[:5]) and list(want[32:40]) == [-1] * 8 and list(want[40:]) == [CANARY] * 4
    assert_same(prims.cpu().numpy(), want)
    assert_same(counts.cpu().numpy(), orf.counts_of(m))
    # the middle row alone: its neighbours keep their canaries
    prims.fill_(CANARY)
    d_offsets = dev(offsets)
    assert raw_call(gpu, scene, d_tris[1:2], 1, 0, -1, d_offsets[1:3], prims, counts[1:2]) == 0
    torch.cuda.synchronize()
    got = prims.cpu().numpy()
    assert list(got[15:20]) == list(fan[:5]) and (got[:15] == CANARY).all() and (got[20:] == CANARY).all()
    none = otr.overlap_matrix(v, idx, queries, skip_shared=True)
    assert not none.any()
    check_all_forms(scene, none, queries, (0, 5), "skip_shared", skip_shared=True)


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts", "binary"])
def test_mesh_2k(gpu, split):
    """the margin test's 1024 query triangles against the 2 k mesh: lists and counts do not depend on the tree -- every split method,
    and the binary tree of a scene kept off the 4-wide one, give the brute force's bytes"""
    case = tri_case()
    check_mix(case["count"])
    scene = binary_scene(gpu, dragon()) if split == "binary" else gpu.Scene(dragon(split))
    check_all_forms(scene, case["m"], case["queries"], (0, 1, 8, 32), split)


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_the_walk_is_the_box_walk(gpu, binary):
    """Inside the tree the bounds test alone is applied: the counted form's nodes visited and triangles taken to step 2 equal those of
    gnxr_overlap_box_counted_device on the boxes [qlo, qhi], exactly, on the 4-wide and on the binary tree"""
    case = tri_case()
    check_mix(case["count"])
    scene = binary_scene(gpu, dragon()) if binary else gpu.Scene(dragon())
    queries = case["queries"]
    qlo, qhi = otr.query_bounds(queries)
    ok = otr.tri_valid(queries)
    assert ok.all()   # a box of a non-finite query would be refused by the box rule as well, but on other grounds
    work_t, work_b = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
    count = scene.count_overlapping_triangles(dev(queries), counts=work_t)
    in_box = scene.count_in_box(dev(orf.box_records(qlo, qhi)), counts=work_b)
    torch.cuda.synchronize()
    assert_same(count.cpu().numpy(), case["count"])
    assert (in_box >= count).all()
    nodes, tris = (int(x) for x in work_t.cpu())
    print(f"nodes {nodes}, triangles {tris}, in the boxes {int(in_box.sum())}, overlapping {int(count.sum())}")
    assert nodes > len(queries) and tris >= int(in_box.sum())
    assert [nodes, tris] == [int(x) for x in work_b.cpu()]


@pytest.mark.gpu
def test_self_intersections(gpu):
    """The 2 k scene at rest and under a sine deformation through update_vertices that folds a third of it through itself:
    self_intersections equals the brute force with the skip rule on bytes, in rows (K = 4) and CSR; it equals, on bytes,
    overlap_triangles of the scene's own triangles in authoring order with skip_shared=True; pairs=True is the upper triangle of
    m | m.T; so does the host form, and the binary tree"""
    case, s = tri_case(), self_case()
    v, idx = case["v"], case["idx"]
    involved = (s["bent"].any(axis=0) | s["bent"].any(axis=1)).mean()
    assert 0.05 < involved < 0.6
    scene = gpu.Scene(dragon())
    check_self(scene, s["rest"], (4,), "at rest")
    assert_same(scene.self_intersections(pairs=True).cpu().numpy(), otr.pairs_of(s["rest"]))
    scene.update_vertices(dev(s["v2"][:s["n_mesh_v"]]))
    check_self(scene, s["bent"], (0, 4), "deformed")
    own = gpu.triangle_queries(dev(s["v2"]), dev(idx))
    assert_same(own.cpu().numpy(), otr.tri_records(s["v2"][idx]))
    for K in (4, None):
        a, b = scene.self_intersections(K), scene.overlap_triangles(own, K, skip_shared=True)
        torch.cuda.synchronize()
        assert_same(a.count.cpu().numpy(), b.count.cpu().numpy()); assert_same(a.prims.cpu().numpy(), b.prims.cpu().numpy())
    pairs = scene.self_intersections(pairs=True)
    torch.cuda.synchronize()
    want = otr.pairs_of(s["bent"])
    assert pairs.dtype == torch.int32 and len(want) > 100
    assert_same(pairs.cpu().numpy(), want)
    h_prims, h_count, h_offsets = scene.OverlapTriangles(None, None, flags=SELF)
    want_offsets, want_prims = orf.csr_of(s["bent"])
    assert_same(h_prims, want_prims); assert_same(h_count, orf.counts_of(s["bent"])); assert_same(h_offsets, want_offsets)
    h_rows, h_count = scene.OverlapTriangles(None, 4, flags=SELF | SKIP)
    assert_same(h_rows, orf.rows_of(s["bent"], 4))
    two = binary_scene(gpu, dragon())
    two.update_vertices(dev(s["v2"][:s["n_mesh_v"]]))
    check_self(two, s["bent"], (4,), "binary")


@pytest.mark.gpu
def test_live_scene(gpu):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    SkinnedMesh.pose -> the brute force over the vertices it holds; set_geometry with another triangle count -> over the new mesh, the
    SELF call's n is the new count and the old one is refused.  The general call and self_intersections, each time."""
    case, s = tri_case(), self_case()
    b = dragon()
    v, idx = mesh_of(b)
    queries = case["queries"][::2]
    scene = gpu.Scene(b)
    v2, n_mesh_v = s["v2"], s["n_mesh_v"]
    scene.update_vertices(dev(v2[:n_mesh_v]))
    m2 = otr.overlap_matrix(v2, idx, queries)
    assert (m2 != case["m"][::2]).any()
    check_all_forms(scene, m2, queries, (0, 8), "update_vertices")
    check_self(scene, s["bent"], (4,), "update_vertices")
    scene.rebuild_bvh()
    check_all_forms(scene, m2, queries, (0, 8), "rebuild_bvh")
    check_self(scene, s["bent"], (4,), "rebuild_bvh")
    rest = v2[:n_mesh_v]
    h = (rest[:, 1] - rest[:, 1].min()) / (rest[:, 1].max() - rest[:, 1].min())
    bw = np.stack([h, 1 - h, np.zeros(n_mesh_v), np.zeros(n_mesh_v)], 1).astype(F)
    bi = np.tile(np.array([0, 1, 0, 0], np.int32), (n_mesh_v, 1))
    ca, sa = np.cos(0.6), np.sin(0.6)
    bones = np.stack([np.array([[ca, 0, sa, 0.1], [0, 1, 0, 0.2], [-sa, 0, ca, 0]]), np.eye(3, 4)]).astype(F)
    sk = gpu.SkinnedMesh(scene, v2.copy(), dev(rest), dev(bi), dev(bw), first_vertex=0, normals=False)
    sk.pose(dev(bones))
    torch.cuda.synchronize()
    v3 = sk.vertices.cpu().numpy()
    assert v3.tobytes() != v2.tobytes()
    check_all_forms(scene, otr.overlap_matrix(v3, idx, queries), queries, (0, 8), "pose")
    check_self(scene, otr.self_matrix(v3, idx), (4,), "pose")
    rng = np.random.default_rng(11)
    v4 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v4[1::3] = v4[0::3] + rng.uniform(-0.6, 0.6, (300, 3)).astype(F)
    v4[2::3] = v4[0::3] + rng.uniform(-0.6, 0.6, (300, 3)).astype(F)
    idx4 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    old = scene.n_triangles
    scene.set_geometry(v4, idx4, np.zeros(300, np.int32), tri_light=tri_light)
    check_all_forms(scene, otr.overlap_matrix(v4, idx4, queries), queries, (0, 8), "set_geometry")
    m4 = otr.self_matrix(v4, idx4)
    assert scene.n_triangles == 300 != old and m4.any()
    check_self(scene, m4, (4,), "set_geometry")
    counts = torch.zeros(old, dtype=torch.int32, device="cuda")
    assert raw_call(gpu, scene, None, old, SELF, 0, None, None, counts) == ERR_INVALID and "300 triangles" in gpu.lib().gnxr_last_error().decode()
    assert raw_call(gpu, scene, None, 300, SELF, 0, None, None, counts) == 0
    torch.cuda.synchronize()
    assert_same(counts[:300].cpu().numpy(), orf.counts_of(m4))
    assert (counts[300:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_deep_tree_spills(gpu, binary):
    """chain_scene(36): a query round the small end of the chain makes the walk descend it with a sibling on its stack per level.  With
    the default LDS levels on the 4-wide tree, where the tree's need exceeds them, and forced onto 2 LDS levels through
    GNXR_OVERLAP_LDS_LEVELS on the 4-wide and on the binary tree: the LDS levels and the global spill together give the same bytes,
    for caller's queries and for the scene against itself."""
    b = chain_scene(gpu)
    v, idx = mesh_of(b)
    rng = np.random.default_rng(9)
    n = 1024
    ctr = np.zeros((n, 1, 3))
    ctr[:, 0, 0] = (2.0 ** -rng.integers(0, 36, n)) * rng.uniform(0.9, 1.1, n)
    extent = (2.0 ** -rng.integers(0, 38, (n, 1, 1))) * rng.uniform(0.5, 1.0, (n, 1, 1))
    corners = ctr + extent * rng.uniform(-1, 1, (n, 3, 3))
    # every seventh: a sliver inside the chain's cone (the triangle at x reaches 0.3 x off the axis) from x = 0.7 * 2^-j to beyond its
    # large end: it crosses the j + 1 largest triangles
    j = rng.integers(0, 40, len(corners[::7]))
    corners[::7] = np.array([(0, 0, 0), (1.1, 0.05, 0.05), (1.1, -0.05, 0.05)])
    corners[::7, 0, 0] = 0.7 * 2.0 ** -j
    queries = otr.tri_records(corners.astype(F))
    m = otr.overlap_matrix(v, idx, queries)
    count = orf.counts_of(m)
    assert list(count[::7]) == list(np.minimum(j + 1, 36))
    assert (count == 36).sum() > 10 and (count > 32).sum() > 15 and ((count > 0) & (count < 4)).sum() > 50 and (count == 0).sum() > 50
    ms = otr.self_matrix(v, idx)
    scene = binary_scene(gpu, b) if binary else gpu.Scene(b)
    if not binary:
        assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
        check_all_forms(scene, m, queries, (0, 3, 32), "default levels")
        check_self(scene, ms, (4,), "default levels")
    os.environ["GNXR_OVERLAP_LDS_LEVELS"] = "2"
    try:
        check_all_forms(scene, m, queries, (0, 3, 32), "2 LDS levels")
        check_self(scene, ms, (4,), "2 LDS levels")
    finally:
        del os.environ["GNXR_OVERLAP_LDS_LEVELS"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_entry_points(gpu, n):
    """the counted entry point gives the same lists and two positive counters; `out` and `counts_out` are used; corners and a (vertices,
    indices) pair pack into the same records; the host-array entry point agrees with the device one, in rows and CSR form; n == 0
    returns at once"""
    case = tri_case()
    scene = gpu.Scene(dragon())
    queries, m = case["queries"][:n], case["m"][:n]
    d_tris = dev(queries.copy())
    rows, count = orf.rows_of(m, 8), orf.counts_of(m)
    out = torch.full((n, 8), CANARY, dtype=torch.int32, device="cuda")
    counts_out = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    res = scene.overlap_triangles(d_tris, 8, out=out, counts_out=counts_out, counts=work)
    torch.cuda.synchronize()
    assert res.prims is out and res.count is counts_out
    assert_same(out.cpu().numpy(), rows); assert_same(counts_out.cpu().numpy(), count)
    nodes, tris = (int(x) for x in work.cpu())
    assert nodes >= n and tris >= int(count.sum()) and (n < 257 or tris > 0) and (n > 0 or nodes == 0)
    work.zero_()
    csr = scene.overlap_triangles(d_tris, counts=work)
    torch.cuda.synchronize()
    want_offsets, want_prims = orf.csr_of(m)
    assert_same(csr.offsets.cpu().numpy(), want_offsets); assert_same(csr.prims.cpu().numpy(), want_prims); assert_same(csr.count.cpu().numpy(), count)
    walks = 2 if count.sum() else 1   # the count-only walk and, unless every list is empty, the one that fills the rows
    assert int(work[0]) == walks * nodes and int(work[1]) == walks * tris
    corners = d_tris.view(n, 3, 4)[:, :, 0:3].contiguous()
    packed = torch.full((n, 12), 5.0, device="cuda")
    assert gpu.triangle_queries(corners, out=packed) is packed
    flat = gpu.triangle_queries(corners.view(n, 9))
    gathered = gpu.triangle_queries(corners.view(3 * n, 3), torch.arange(3 * n, device="cuda").view(n, 3))
    by_corners = scene.overlap_triangles(corners, 8)
    by_pair = scene.overlap_triangles((corners.view(3 * n, 3), torch.arange(3 * n, dtype=torch.int32, device="cuda").view(n, 3)), 8)
    only = scene.count_overlapping_triangles(corners.view(n, 9))
    torch.cuda.synchronize()
    for t in (packed, flat, gathered):
        assert_same(t.cpu().numpy(), queries)
    assert_same(by_corners.prims.cpu().numpy(), rows); assert_same(by_pair.prims.cpu().numpy(), rows); assert_same(only.cpu().numpy(), count)
    h_rows, h_count = scene.OverlapTriangles(queries, 8)
    assert_same(h_rows, rows); assert_same(h_count, count)
    h_rows, h_count = scene.OverlapTriangles(queries, 0)
    assert h_rows.shape == (n, 0); assert_same(h_count, count)
    h_prims, h_count, h_offsets = scene.OverlapTriangles(queries, None)
    assert_same(h_prims, want_prims); assert_same(h_count, count); assert_same(h_offsets, want_offsets)
    skipped = otr.overlap_matrix(case["v"], case["idx"], queries, skip_shared=True)
    h_rows, h_count = scene.OverlapTriangles(queries, 8, flags=SKIP)
    assert_same(h_rows, orf.rows_of(skipped, 8)); assert_same(h_count, orf.counts_of(skipped))
    with pytest.raises(ValueError):
        scene.overlap_triangles(d_tris, 8, out=torch.zeros((n + 1, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        scene.overlap_triangles(d_tris, 8, counts_out=torch.zeros((n,), dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
def test_stream(gpu):
    """Queries written by torch on a side stream, answered there and reduced there with no synchronise in between; the self call and its
    pairs on that stream as well"""
    case, s = tri_case(), self_case()
    scene = gpu.Scene(dragon())
    src = dev(case["queries"].copy())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tris = src * 1.0
        res = scene.overlap_triangles(tris, 8, stream=side)
        csr = scene.overlap_triangles(tris, stream=side)
        pairs = scene.self_intersections(pairs=True, stream=side)
        total = res.count.to(torch.int64).sum() + res.prims.to(torch.int64).sum() + csr.prims.to(torch.int64).sum() + pairs.numel()
    side.synchronize()
    rows, (_, prims) = orf.rows_of(case["m"], 8), orf.csr_of(case["m"])
    assert int(total) == int(case["count"].astype(np.int64).sum() + rows.astype(np.int64).sum() + prims.astype(np.int64).sum() + otr.pairs_of(s["rest"]).size)
    assert_same(res.prims.cpu().numpy(), rows); assert_same(csr.prims.cpu().numpy(), prims)


@pytest.mark.gpu
def test_refusals(gpu):
    """flags, the SELF arguments, misaligned pointers, host memory, a max_prims that does not go with the offsets and an array that runs
    past its allocation give GNXR_ERR_INVALID with a message before anything is queued; the scene still answers afterwards"""
    case = tri_case()
    scene = gpu.Scene(dragon())
    L = gpu.lib()
    nt = scene.n_triangles
    tris = dev(case["queries"].copy())
    out = torch.zeros((nt, 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nt, dtype=torch.int32, device="cuda")
    off = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
    P = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    err = lambda: L.gnxr_last_error().decode()
    call = lambda *a: L.gnxr_overlap_tri_device(scene._h, *a)
    assert call(P(tris), 100, 4, 8, None, P(out), P(cnt), None) == ERR_INVALID and "flags" in err()
    assert call(P(tris), nt, SELF, 8, None, P(out), P(cnt), None) == ERR_INVALID and "SELF" in err() and "NULL" in err()
    for n in (nt - 1, nt + 1, 1):
        assert call(None, n, SELF, 8, None, P(out), P(cnt), None) == ERR_INVALID and f"{nt} triangles" in err()
        assert call(None, n, SELF | SKIP, 0, None, None, P(cnt), None) == ERR_INVALID and f"{nt} triangles" in err()
    assert call(None, nt, SELF, 8, None, P(out, 2), P(cnt), None) == ERR_INVALID and "d_prims is not 4-byte aligned" in err()
    assert call(P(tris, 4), 100, 0, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_tris is not 16-byte aligned" in err()
    assert call(P(tris, 8), 100, 0, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_tris is not 16-byte aligned" in err()
    assert call(P(tris), 100, 0, 8, None, P(out, 2), P(cnt), None) == ERR_INVALID and "d_prims is not 4-byte aligned" in err()
    assert call(P(tris), 100, 0, 8, None, P(out), P(cnt, 2), None) == ERR_INVALID and "d_counts is not 4-byte aligned" in err()
    assert call(P(tris), 100, 0, -1, P(off, 4), P(out), P(cnt), None) == ERR_INVALID and "d_offsets is not 8-byte aligned" in err()
    assert call(P(tris), 100, 0, 8, P(off), P(out), P(cnt), None) == ERR_INVALID and "CSR" in err()
    assert call(P(tris), 100, 0, -1, None, P(out), P(cnt), None) == ERR_INVALID and "CSR" in err()
    assert call(P(tris), 100, 0, 33, None, P(out), P(cnt), None) == ERR_INVALID and "max_prims" in err()
    assert call(P(tris), 100, 0, 0, None, P(out), P(cnt), None) == ERR_INVALID and "count-only" in err()
    host = np.zeros((100, 64), F)
    H = C.c_void_p(host.ctypes.data)
    assert call(H, 100, 0, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_tris is not device memory" in err()
    assert call(P(tris), 100, 0, 8, None, H, P(cnt), None) == ERR_INVALID and "d_prims is not device memory" in err()
    assert call(P(tris), 100, 0, 8, None, P(out), H, None) == ERR_INVALID and "d_counts is not device memory" in err()
    assert call(P(tris), 100, 0, -1, H, P(out), P(cnt), None) == ERR_INVALID and "d_offsets is not device memory" in err()
    assert call(None, nt, SELF, 0, None, None, H, None) == ERR_INVALID and "d_counts is not device memory" in err()
    many = torch.zeros((1 << 20, 12), device="cuda")
    assert call(P(many), 1 << 20, 0, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_prims" in err()   # 2^20 rows of 8: far past out's allocation
    assert call(P(tris), 1 << 20, 0, 0, None, None, P(cnt), None) == ERR_INVALID and "d_tris" in err()      # 2^20 records from a 1024-record array
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.gnxr_overlap_tri_counted_device(scene._h, P(tris), 100, 0, 8, None, P(out), P(cnt), P(work, 4), None) == ERR_INVALID and "d_work" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (cnt == 0).all() and (work == 0).all()   # nothing was queued by the refused calls
    for bad in (tris.double(), tris.cpu(), tris[:, :5].contiguous(), tris.t(), case["queries"]):
        with pytest.raises(ValueError):
            scene.overlap_triangles(bad, 8)
    with pytest.raises(ValueError):
        scene.overlap_triangles(tris, 8, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    corners = torch.zeros((8, 3), device="cuda")
    for bad in (torch.zeros((2, 3), device="cuda"), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="triangle_queries: indices"):
            gpu.triangle_queries(corners, bad)
    assert_same(device_rows(scene, case["queries"], 8)[0], orf.rows_of(case["m"], 8))
