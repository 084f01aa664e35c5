"""Box overlap queries (include/gnxr.h, "Overlap queries"): the numpy restatement (tests/overlap_reference.py) on hand-made exact cases and
against an independent float64 separating-axis check, the refusals of the C calls and of the Python methods without a device, then
gnxr_overlap_box_device / gnxr_overlap_box and Scene.voxelize on the GPU against the restatement's brute force over all triangles.
Every comparison of rows, CSR lists and counts is on their bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import overlap_reference as orf
from conftest import ROOT
from overlap_cases import HAND_MADE, ONE, dragon_case, hand_made_by_triangle
from query_cases import assert_same, bound_of, chain_scene, dragon, fan_mesh, mesh_of, mesh_scene

ERR_INVALID = -1
F = np.float32
CANARY = -7


# ---------------------------------------------------------------- helpers
def device_rows(scene, boxes, K, **kw):
    res = scene.overlap_box(torch.from_numpy(np.array(boxes, F)).cuda(), None, K, **kw)
    torch.cuda.synchronize()
    return res.prims.cpu().numpy(), res.count.cpu().numpy()


def device_csr(scene, boxes, **kw):
    res = scene.overlap_box(torch.from_numpy(np.array(boxes, F)).cuda(), **kw)
    torch.cuda.synchronize()
    return res.offsets.cpu().numpy(), res.prims.cpu().numpy(), res.count.cpu().numpy()


def check_all_forms(scene, m, boxes, Ks=(0, 1, 8, 32), what=""):
    """rows mode for every K of `Ks` and the CSR form against the restatement's matrix `m`"""
    count = orf.counts_of(m)
    for K in Ks:
        got, cnt = device_rows(scene, boxes, K)
        assert_same(cnt, count, f"{what} K={K} counts")
        assert_same(got, orf.rows_of(m, K), f"{what} K={K}")
    offsets, prims, cnt = device_csr(scene, boxes)
    want_offsets, want_prims = orf.csr_of(m)
    assert_same(cnt, count, f"{what} CSR counts")
    assert_same(offsets, want_offsets, f"{what} CSR offsets")
    assert_same(prims, want_prims, f"{what} CSR")


def raw_call(gx, scene, boxes, max_prims, offsets, prims, counts, work=None, stream=None):
    """gnxr_overlap_box[_counted]_device on tensors, as the C ABI takes them"""
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L = gx.lib()
    if work is None:
        return L.gnxr_overlap_box_device(scene._h, P(boxes), len(boxes), max_prims, P(offsets), P(prims), P(counts), stream)
    return L.gnxr_overlap_box_counted_device(scene._h, P(boxes), len(boxes), max_prims, P(offsets), P(prims), P(counts), P(work), stream)


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_overlap_box_device", "gnxr_overlap_box_counted_device", "gnxr_overlap_box"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.BoxQuery) == 32
    assert gx.OVERLAP_MAX == 32 == orf.OVERLAP_MAX
    assert gx._abi.GNXR_ABI_VERSION == 5 and gx._abi.BoxQuery not in gx._abi.ABI_STRUCTS
    assert gx.OverlapLists._fields == ("count", "prims") and gx.OverlapCSR._fields == ("count", "offsets", "prims")


@pytest.mark.parametrize("case", HAND_MADE, ids=[c[0] for c in HAND_MADE])
def test_restatement_exact_cases(case):
    """Triangles of small integer coordinates; the boxes touch them in one point, miss by one ulp or reach one ulp into them, through a
    box axis, an edge axis and the plane (tests/overlap_cases.py has the arithmetic of each)."""
    _, tri, lo, hi, want = case
    boxes = orf.box_records(np.array([lo], F), np.array([hi], F))
    m = orf.overlap_matrix(np.array(tri, F), ONE, boxes)
    assert m.shape == (1, 1) and int(m[0, 0]) == want
    assert list(orf.counts_of(m)) == [want] and list(orf.rows_of(m, 2)[0]) == ([0, -1] if want else [-1, -1])


def test_restatement_order_and_cuts():
    """three coincident copies of one triangle and one other: the prims ascend, a short row (rows mode: K < count; CSR: capacity < count)
    holds the smallest, and the count is never clamped"""
    tri = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F)
    v = np.concatenate([tri, tri + F((0, 0, 1))])
    idx = np.array([(3, 4, 5), (0, 1, 2), (1, 2, 0), (2, 0, 1)], np.int32)
    boxes = orf.box_records(np.array([(1, 1, -0.5), (1, 1, -0.5)], F), np.array([(2, 2, 0.5), (2, 2, 1)], F))
    m = orf.overlap_matrix(v, idx, boxes)
    assert list(orf.counts_of(m)) == [3, 4]
    for K in (0, 1, 2, 3, 4, 6):
        rows = orf.rows_of(m, K)
        assert rows.shape == (2, K) and list(rows[0]) == [1, 2, 3, -1, -1, -1][:K] and list(rows[1]) == [0, 1, 2, 3, -1, -1][:K]
    offsets, prims = orf.csr_of(m)
    assert list(offsets) == [0, 3, 7] and list(prims) == [1, 2, 3, 0, 1, 2, 3]
    offsets, prims = orf.csr_of(m, np.array([1, 3, 9]), np.full(10, CANARY, np.int32))
    assert list(prims) == [CANARY, 1, 2, 0, 1, 2, 3, -1, -1, CANARY]
    assert list(orf.counts_of(m)) == [3, 4]   # whatever the rows hold
    assert not orf.overlap_matrix(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), boxes).size


def test_float64_margin():
    """An independent check that knows only geometry: a 13-axis separating-axis test in float64 on normalised axes (orf.sat_gap64).  A pair
    the fp32 definition reports must not be separated by more than the margin, a pair it rejects must not overlap by more than the
    margin on every axis.  Measured on the 2 k-triangle mesh with these 1024 mixed boxes (2 019 328 pairs, 155 665 of them past the
    bounds test, 153 984 overlapping): the largest float64 gap at which the two disagree is 0 -- they disagree nowhere; the pair nearest
    to contact has |gap| = 1.76e-5, 2.0e-6 of the scene's diagonal 8.66, far outside fp32 rounding, so this set does not reach the
    rounding of steps 4 and 5.  Allowed: 4 x that = 0 of the scene's diagonal, i.e. the two must agree on every pair of the set."""
    case = dragon_case()
    v, idx, boxes, m = case["v"], case["idx"], case["boxes"], case["m"]
    margin = 4 * 0.0 * float(np.linalg.norm(np.subtract(*bound_of(v)[::-1])))
    # pairs apart along a box axis need no arithmetic in either precision: the comparisons are exact.  The others go to the float64 test.
    tri = v[idx].astype(np.float64)
    b64 = boxes.astype(np.float64)
    near = orf.box_valid(boxes)[:, None] & ((tri.min(axis=1)[None] <= b64[:, None, 4:7]) & (tri.max(axis=1)[None] >= b64[:, None, 0:3])).all(axis=2)
    assert not (m & ~near).any()
    bi, ti = np.nonzero(near)
    gap = orf.sat_gap64(v, idx, boxes, bi, ti)
    said = m[bi, ti]
    print(f"pairs {m.size}, past the bounds test {len(bi)}, overlapping {int(said.sum())}, smallest |gap| {np.abs(gap).min():.3e}, "
          f"largest gap of a reported pair {gap[said].max():.3e}, smallest of a rejected one {gap[~said].min():.3e}")
    assert (gap[said] <= margin).all()
    assert (gap[~said] >= -margin).all()


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0, n < 0, max_prims out of range, rows that do not go with max_prims and a max_prims that
    does not go with the offsets are refused before anything is looked at (the handle is a dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    err = lambda: L.gnxr_last_error().decode()
    for fn in (L.gnxr_overlap_box_device, lambda s, b, n, k, o, r, c, st: L.gnxr_overlap_box_counted_device(s, b, n, k, o, r, c, p, st)):
        assert fn(None, p, 1, 1, None, p, p, None) == ERR_INVALID
        assert fn(None, p, 0, 1, None, p, p, None) == ERR_INVALID
        assert fn(p, None, 4, 1, None, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 1, None, None, p, None) == ERR_INVALID      # rows missing with max_prims > 0
        assert fn(p, p, 4, 1, None, p, None, None) == ERR_INVALID
        assert fn(p, p, 4, 0, None, p, p, None) == ERR_INVALID and "count-only" in err()
        assert fn(p, p, -1, 1, None, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 33, None, p, p, None) == ERR_INVALID and "max_prims" in err()
        assert fn(p, p, 4, -2, None, p, p, None) == ERR_INVALID and "max_prims" in err()
        assert fn(p, p, 4, -1, None, p, p, None) == ERR_INVALID and "CSR" in err()      # -1 without offsets
        for k in (0, 1, 32, -2):
            assert fn(p, p, 4, k, p, p, p, None) == ERR_INVALID and "CSR" in err()      # offsets with anything but -1
        assert fn(p, p, 4, -1, p, None, p, None) == ERR_INVALID                         # CSR rows without an array
        assert fn(p, p, 0, 33, None, p, p, None) == ERR_INVALID                         # n == 0 is a no-op only for good arguments
    assert L.gnxr_overlap_box_counted_device(p, p, 4, 1, None, p, p, None, None) == ERR_INVALID
    B, I, O = (lambda x: C.cast(x, C.POINTER(gx._abi.BoxQuery))), (lambda x: C.cast(x, C.POINTER(C.c_int32))), (lambda x: C.cast(x, C.POINTER(C.c_int64)))
    assert L.gnxr_overlap_box(None, B(p), 1, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, None, 1, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, 1, None, None, I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, 1, None, I(p), None) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, 0, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), -1, 1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, 33, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, -1, None, I(p), I(p)) == ERR_INVALID
    assert L.gnxr_overlap_box(p, B(p), 1, 4, O(p), I(p), I(p)) == ERR_INVALID
    off = (C.c_int64 * 3)(4, 2, 8)
    assert L.gnxr_overlap_box(p, B(p), 2, -1, off, I(p), I(p)) == ERR_INVALID and "ascend" in err()
    off = (C.c_int64 * 3)(-1, 2, 8)
    assert L.gnxr_overlap_box(p, B(p), 2, -1, off, I(p), I(p)) == ERR_INVALID and "negative" in err()


def test_python_refuses_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 3) pairs or (n, 8) records on the scene's device pass, max_prims is None or an integer in range, the
    launch keywords are `stream` and `counts`, a voxel grid is three numbers, a positive cell and three positive integers; everything
    else raises before a library call (the handle is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    bad = [np.zeros((4, 3), F), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 5)), torch.zeros((3, 4)).t(), torch.zeros((4, 6))[:, ::2],
           torch.zeros(12), "boxes", None, torch.zeros((4, 3)), torch.zeros((4, 8))]
    for b in bad:
        for call in (lambda: s.overlap_box(b, None, 4), lambda: s.overlap_box(b), lambda: s.count_in_box(b), lambda: s.overlap_box(b, b, 4)):
            with pytest.raises(ValueError, match="overlap_box|count_in_box"):
                call()
    with pytest.raises(ValueError, match="overlap_box: .*ready-made"):
        s.overlap_box(torch.zeros((4, 8)), torch.zeros((4, 3)), 4)
    with pytest.raises(ValueError, match="count_in_box: .*ready-made"):
        s.count_in_box(torch.zeros((4, 8)), torch.zeros((4, 3)))
    for k in (33, -1):
        with pytest.raises(ValueError, match="overlap_box: max_prims"):
            s.overlap_box(torch.zeros((4, 8)), None, k)
    for k in (1.5, "4", True):
        with pytest.raises(TypeError, match="overlap_box: max_prims"):
            s.overlap_box(torch.zeros((4, 8)), None, k)
    with pytest.raises(ValueError, match="overlap_box: .*out must be None"):
        s.overlap_box(torch.zeros((4, 8)), None, None, out=torch.zeros((4, 4), dtype=torch.int32))
    for method, args in ((s.overlap_box, (torch.zeros((4, 8)), None, 4)), (s.count_in_box, (torch.zeros((4, 8)),)), (s.voxelize, ((0, 0, 0), 1.0, (2, 2, 2)))):
        with pytest.raises(ValueError, match="unexpected arguments"):
            method(*args, streams=None)
    grids = [((0, 0), 1.0, (2, 2, 2)), ((0, 0, 0), 0.0, (2, 2, 2)), ((0, 0, 0), -1.0, (2, 2, 2)), ((0, 0, 0), (1, 1), (2, 2, 2)), ((0, 0, 0), 1.0, (2, 2)),
             ((0, 0, 0), 1.0, (2, 0, 2)), ((0, 0, 0), 1.0, (2, 2.5, 2)), ((0, np.nan, 0), 1.0, (2, 2, 2)), ((0, 0, 0), np.inf, (2, 2, 2)), ((0, 0, 0), 1.0, (2, 2, (1 << 24) + 1))]
    for g in grids:
        with pytest.raises((ValueError, TypeError), match="voxelize"):
            s.voxelize(*g)
        with pytest.raises((ValueError, TypeError), match="voxel_boxes"):
            gx.voxel_boxes(*g)
    with pytest.raises(ValueError, match="voxelize: fill"):
        s.voxelize((0, 0, 0), 1.0, (2, 2, 2), fill=True, counts=True)
    for chunk in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="voxelize: chunk"):
            s.voxelize((0, 0, 0), 1.0, (2, 2, 2), chunk=chunk)
    with pytest.raises(ValueError, match="voxel_boxes: unexpected arguments"):
        gx.voxel_boxes((0, 0, 0), 1.0, (2, 2, 2), streams=None)


def test_voxel_records_share_faces():
    """the restated grid: x fastest, and hi of a voxel is lo of its neighbour bit for bit, also where i * cell rounds"""
    boxes = orf.voxel_records((0.1, -0.7, 3.3), (0.3, 0.7, 0.11), (5, 4, 3)).reshape(3, 4, 5, 8)
    assert_same(boxes[:, :, 1:, 0], boxes[:, :, :-1, 4]); assert_same(boxes[:, 1:, :, 1], boxes[:, :-1, :, 5]); assert_same(boxes[1:, :, :, 2], boxes[:-1, :, :, 6])
    assert boxes[0, 0, 0, 0] == F(0.1) and boxes[0, 0, 1, 0] == F(1) * F(0.3) + F(0.1) and boxes[2, 3, 4, 6] == F(3) * F(0.11) + F(3.3)
    assert not boxes[..., 3].any() and not boxes[..., 7].any()


def test_no_scratch(gx):
    """tools/kernel_regs.py: every instantiation of k_overlap_box (wide / binary; count-only / rows; timed / counting) runs without scratch
    and without spilled VGPRs -- the list lives in the output row, not in a private array"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels(gx.LIB_PATH) if "k_overlap_box<" in k["name"]]
    assert len(ks) == 8, [k["name"] for k in ks]
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in ks), ks


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_one_triangle_scenes(gpu):
    """every hand-made case on the device, in rows mode at K = 0, 1 and 2 and in CSR mode"""
    for tri, (boxes, want, names) in hand_made_by_triangle().items():
        v = np.array(tri, F)
        m = orf.overlap_matrix(v, ONE, boxes)
        assert list(orf.counts_of(m)) == list(want), names
        check_all_forms(gpu.Scene(mesh_scene(gpu, v, ONE)), m, boxes, (0, 1, 2), str(tri))


@pytest.mark.gpu
def test_tie_fan(gpu):
    """Twelve triangles round one vertex, among 300 others, and a box that holds only that vertex: all twelve touch it.  Rows mode cuts to
    the smallest prims; CSR rows that are exact, short, over-long and out of order hold the smallest prims, then -1, and nothing outside
    a row is written (canaries before, behind and, for a call on the middle row alone, in the neighbouring rows)."""
    v, idx, fan = fan_mesh(np.random.default_rng(50), 1, 300)
    boxes = orf.box_records(np.full((4, 3), -0.125, F), np.full((4, 3), 0.125, F))
    m = orf.overlap_matrix(v, idx, boxes)
    assert list(orf.counts_of(m)) == [12] * 4 and list(np.flatnonzero(m[0])) == list(fan) and (np.diff(fan) > 0).all()
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    check_all_forms(scene, m, boxes, (0, 5, 12, 13, 32))
    assert list(device_rows(scene, boxes, 5)[0][0]) == list(fan[:5])
    d_boxes = torch.from_numpy(boxes).cuda()
    offsets = np.array([3, 15, 20, 40, 36], np.int64)   # exact, short (5), over-long (20), out of order (nothing)
    prims = torch.full((44,), CANARY, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert raw_call(gpu, scene, d_boxes, -1, torch.from_numpy(offsets).cuda(), prims, counts) == 0
    torch.cuda.synchronize()
    want = orf.csr_of(m, offsets, np.full(44, CANARY, np.int32))[1]
    assert list(want[:3]) == [CANARY] * 3 and list(want[3:15]) == list(fan) and list(want[15:20]) == list(fan[:5]) and list(want[32:40]) == [-1] * 8 and list(want[40:]) == [CANARY] * 4
    assert_same(prims.cpu().numpy(), want)
    assert_same(counts.cpu().numpy(), orf.counts_of(m))
    # the middle row alone: its neighbours keep their canaries
    prims.fill_(CANARY)
    d_offsets = torch.from_numpy(offsets).cuda()
    assert raw_call(gpu, scene, d_boxes[1:2], -1, d_offsets[1:3], prims, counts[1:2]) == 0
    torch.cuda.synchronize()
    got = prims.cpu().numpy()
    assert list(got[15:20]) == list(fan[:5]) and (got[:15] == CANARY).all() and (got[20:] == CANARY).all()


@pytest.mark.gpu
def test_whole_scene_box(gpu):
    case = dragon_case()
    lo, hi = bound_of(case["v"])
    boxes = orf.box_records(np.array([lo], F), np.array([hi], F))
    scene = gpu.Scene(dragon())
    offsets, prims, count = device_csr(scene, boxes)
    n = len(case["idx"])
    assert scene.n_triangles == n and list(count) == [n] and list(offsets) == [0, n]
    assert_same(prims, np.arange(n, dtype=np.int32))
    assert_same(device_rows(scene, boxes, 32)[0], np.arange(32, dtype=np.int32)[None])


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts", "binary"])
def test_mesh_2k(gpu, split):
    """1024 boxes of mixed size against the 2 k mesh: lists and counts do not depend on the tree -- every split method, and the binary
    tree of a scene kept off the 4-wide one, give the brute force's bytes"""
    case = dragon_case()
    count = case["count"]
    assert (count == 0).mean() > 0.2 and (count > 32).mean() > 0.2 and (count == len(case["idx"])).any() and ((count > 0) & (count < 8)).any()
    if split == "binary":
        os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(dragon(None if split == "binary" else split))
    finally:
        os.environ.pop("GNXR_BINARY_BVH", None)
    check_all_forms(scene, case["m"], case["boxes"], (0, 1, 8, 32), split)


@pytest.mark.gpu
def test_live_scene(gpu):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    SkinnedMesh.pose -> the brute force over the vertices it holds; set_geometry with another triangle count -> over the new mesh"""
    case = dragon_case()
    b = dragon()
    v, idx = mesh_of(b)
    boxes = case["boxes"][::2]
    scene = gpu.Scene(b)
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(0.15) * np.sin(F(5) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    scene.update_vertices(torch.from_numpy(v2[:n_mesh_v].copy()).cuda())
    m2 = orf.overlap_matrix(v2, idx, boxes)
    assert (m2 != case["m"][::2]).any()
    check_all_forms(scene, m2, boxes, (0, 8), "update_vertices")
    scene.rebuild_bvh()
    check_all_forms(scene, m2, boxes, (0, 8), "rebuild_bvh")
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
    assert v3.tobytes() != v2.tobytes()
    check_all_forms(scene, orf.overlap_matrix(v3, idx, boxes), boxes, (0, 8), "pose")
    rng = np.random.default_rng(11)
    v4 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v4[1::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    v4[2::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    idx4 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    scene.set_geometry(v4, idx4, np.zeros(300, np.int32), tri_light=tri_light)
    check_all_forms(scene, orf.overlap_matrix(v4, idx4, boxes), boxes, (0, 8), "set_geometry")


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_deep_tree_spills(gpu, binary):
    """chain_scene(36): a box round the small end of the chain makes the walk descend it with a sibling on its stack per level.  With the
    default LDS levels on the 4-wide tree, where the tree's need exceeds them, and forced onto 2 LDS levels through
    GNXR_OVERLAP_LDS_LEVELS on the 4-wide and on the binary tree: the LDS levels and the global spill together give the same bytes."""
    b = chain_scene(gpu)
    v, idx = mesh_of(b)
    rng = np.random.default_rng(8)
    n = 1024
    ctr = np.zeros((n, 3))
    ctr[:, 0] = (2.0 ** -rng.integers(0, 36, n)) * rng.uniform(0.9, 1.1, n)
    half = (2.0 ** -rng.integers(0, 38, (n, 1))) * rng.uniform(0.5, 1.0, (n, 3))
    half[::7] = 2.0
    boxes = orf.box_records((ctr - half).astype(F), (ctr + half).astype(F))
    m = orf.overlap_matrix(v, idx, boxes)
    count = orf.counts_of(m)
    assert (count == 36).sum() > 100 and (count > 32).sum() > 100 and ((count > 0) & (count < 4)).sum() > 50 and (count == 0).any()
    if binary:
        os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(b)
    finally:
        os.environ.pop("GNXR_BINARY_BVH", None)
    if not binary:
        assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
        check_all_forms(scene, m, boxes, (0, 3, 32), "default levels")
    os.environ["GNXR_OVERLAP_LDS_LEVELS"] = "2"
    try:
        check_all_forms(scene, m, boxes, (0, 3, 32), "2 LDS levels")
    finally:
        del os.environ["GNXR_OVERLAP_LDS_LEVELS"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_entry_points(gpu, n):
    """the counted entry point gives the same lists and two positive counters; `out` and `counts_out` are used; (n, 3) corners pack into
    the same records; the host-array entry point agrees with the device one, in rows and CSR form; n == 0 returns at once"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    boxes, m = case["boxes"][:n], case["m"][:n]
    d_boxes = torch.from_numpy(boxes.copy()).cuda()
    rows, count = orf.rows_of(m, 8), orf.counts_of(m)
    out = torch.full((n, 8), CANARY, dtype=torch.int32, device="cuda")
    counts_out = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    res = scene.overlap_box(d_boxes, None, 8, out=out, counts_out=counts_out, counts=work)
    torch.cuda.synchronize()
    assert res.prims is out and res.count is counts_out
    assert_same(out.cpu().numpy(), rows); assert_same(counts_out.cpu().numpy(), count)
    nodes, tris = (int(x) for x in work.cpu())
    assert nodes >= n and tris >= int(count.sum()) and (n < 257 or tris > 0) and (n > 0 or nodes == 0)
    work.zero_()
    csr = scene.overlap_box(d_boxes, counts=work)
    torch.cuda.synchronize()
    want_offsets, want_prims = orf.csr_of(m)
    assert_same(csr.offsets.cpu().numpy(), want_offsets); assert_same(csr.prims.cpu().numpy(), want_prims); assert_same(csr.count.cpu().numpy(), count)
    walks = 2 if count.sum() else 1   # the count-only walk and, unless every list is empty, the one that fills the rows
    assert int(work[0]) == walks * nodes and int(work[1]) == walks * tris
    pair = scene.overlap_box(d_boxes[:, 0:3].contiguous(), d_boxes[:, 4:7].contiguous(), 8)
    only = scene.count_in_box(d_boxes[:, 0:3].contiguous(), d_boxes[:, 4:7].contiguous())
    torch.cuda.synchronize()
    assert_same(pair.prims.cpu().numpy(), rows); assert_same(only.cpu().numpy(), count)
    h_rows, h_count = scene.OverlapBox(boxes, 8)
    assert_same(h_rows, rows); assert_same(h_count, count)
    h_rows, h_count = scene.OverlapBox(boxes, 0)
    assert h_rows.shape == (n, 0); assert_same(h_count, count)
    h_prims, h_count, h_offsets = scene.OverlapBox(boxes, None)
    assert_same(h_prims, want_prims); assert_same(h_count, count); assert_same(h_offsets, want_offsets)
    with pytest.raises(ValueError):
        scene.overlap_box(d_boxes, None, 8, out=torch.zeros((n + 1, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        scene.overlap_box(d_boxes, None, 8, counts_out=torch.zeros((n,), dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
def test_stream(gpu):
    """Boxes written by torch on a side stream, answered there and reduced there with no synchronise in between"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    src = torch.from_numpy(case["boxes"].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        boxes = src * 1.0
        res = scene.overlap_box(boxes, None, 8, stream=side)
        csr = scene.overlap_box(boxes, stream=side)
        total = res.count.to(torch.int64).sum() + res.prims.to(torch.int64).sum() + csr.prims.to(torch.int64).sum()
    side.synchronize()
    rows, (_, prims) = orf.rows_of(case["m"], 8), orf.csr_of(case["m"])
    assert int(total) == int(case["count"].astype(np.int64).sum() + rows.astype(np.int64).sum() + prims.astype(np.int64).sum())
    assert_same(res.prims.cpu().numpy(), rows); assert_same(csr.prims.cpu().numpy(), prims)


@pytest.mark.gpu
def test_refusals(gpu):
    """misaligned pointers, host memory, a max_prims that does not go with the offsets and an array that runs past its allocation give
    GNXR_ERR_INVALID with a message before anything is queued; the scene still answers afterwards"""
    case = dragon_case()
    scene = gpu.Scene(dragon())
    L = gpu.lib()
    boxes = torch.from_numpy(case["boxes"].copy()).cuda()
    out = torch.zeros((len(boxes), 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(len(boxes), dtype=torch.int32, device="cuda")
    off = torch.zeros(len(boxes) + 1, dtype=torch.int64, device="cuda")
    P = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    err = lambda: L.gnxr_last_error().decode()
    call = lambda *a: L.gnxr_overlap_box_device(scene._h, *a)
    assert call(P(boxes, 4), 100, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_boxes is not 16-byte aligned" in err()
    assert call(P(boxes), 100, 8, None, P(out, 2), P(cnt), None) == ERR_INVALID and "d_prims is not 4-byte aligned" in err()
    assert call(P(boxes), 100, 8, None, P(out), P(cnt, 2), None) == ERR_INVALID and "d_counts is not 4-byte aligned" in err()
    assert call(P(boxes), 100, -1, P(off, 4), P(out), P(cnt), None) == ERR_INVALID and "d_offsets is not 8-byte aligned" in err()
    assert call(P(boxes), 100, 8, P(off), P(out), P(cnt), None) == ERR_INVALID and "CSR" in err()
    assert call(P(boxes), 100, -1, None, P(out), P(cnt), None) == ERR_INVALID and "CSR" in err()
    assert call(P(boxes), 100, 33, None, P(out), P(cnt), None) == ERR_INVALID and "max_prims" in err()
    assert call(P(boxes), 100, 0, None, P(out), P(cnt), None) == ERR_INVALID and "count-only" in err()
    host = np.zeros((100, 64), F)
    H = C.c_void_p(host.ctypes.data)
    assert call(H, 100, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_boxes is not device memory" in err()
    assert call(P(boxes), 100, 8, None, H, P(cnt), None) == ERR_INVALID and "d_prims is not device memory" in err()
    assert call(P(boxes), 100, 8, None, P(out), H, None) == ERR_INVALID and "d_counts is not device memory" in err()
    assert call(P(boxes), 100, -1, H, P(out), P(cnt), None) == ERR_INVALID and "d_offsets is not device memory" in err()
    many = torch.zeros((1 << 20, 8), device="cuda")
    assert call(P(many), 1 << 20, 8, None, P(out), P(cnt), None) == ERR_INVALID and "d_prims" in err()   # 2^20 rows of 8: far past out's allocation
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.gnxr_overlap_box_counted_device(scene._h, P(boxes), 100, 8, None, P(out), P(cnt), P(work, 4), None) == ERR_INVALID and "d_work" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (cnt == 0).all() and (work == 0).all()   # nothing was queued by the refused calls
    for bad in (boxes.double(), boxes.cpu(), boxes[:, :5].contiguous(), boxes.t(), case["boxes"]):
        with pytest.raises(ValueError):
            scene.overlap_box(bad, None, 8)
    with pytest.raises(ValueError):
        scene.overlap_box(boxes[:, 0:3].contiguous(), boxes[:5, 4:7].contiguous(), 8)
    with pytest.raises(ValueError):
        scene.overlap_box(boxes, None, 8, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert_same(device_rows(scene, case["boxes"], 8)[0], orf.rows_of(case["m"], 8))


def cube_mesh(lo, hi):
    """a closed box of twelve triangles"""
    x = np.array([[(lo, hi)[(i >> k) & 1] for k in range(3)] for i in range(8)], F)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return x, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


@pytest.mark.gpu
def test_voxelize(gpu):
    """voxelize equals the chain voxel_boxes -> count_in_box (-> contains) of public calls on bits, in one chunk and in several, and the
    restatement over the restated grid; a triangle lying exactly in the face two voxels share sets both; fill sets the inside of a closed
    mesh"""
    def check(scene, v, idx, origin, cell, dims, chunk):
        boxes = gpu.voxel_boxes(origin, cell, dims)
        want = orf.voxel_records(origin, cell, dims)
        assert_same(boxes.cpu().numpy(), want)
        count = scene.count_in_box(boxes)
        grid = scene.voxelize(origin, cell, dims)
        pieces = scene.voxelize(origin, cell, dims, chunk=chunk)
        numbers = scene.voxelize(origin, cell, dims, counts=True, chunk=chunk)
        torch.cuda.synchronize()
        shape = (dims[2], dims[1], dims[0])
        assert grid.dtype == torch.bool and tuple(grid.shape) == shape and numbers.dtype == torch.int32 and tuple(numbers.shape) == shape
        assert torch.equal(grid, (count > 0).view(shape)) and torch.equal(pieces, grid) and torch.equal(numbers, count.view(shape))
        ref = orf.counts_of(orf.overlap_matrix(v, idx, want)).reshape(shape)
        assert_same(numbers.cpu().numpy(), ref)
        return grid.cpu().numpy()

    # one triangle in the plane x = 0.5 = 2 * 0.25, the face voxels ix = 1 and ix = 2 share: both are set, and nothing else
    v = np.array([(0.5, 0.05, 0.05), (0.5, 0.2, 0.05), (0.5, 0.05, 0.2)], F)
    one = np.array([(0, 1, 2)], np.int32)
    scene = gpu.Scene(mesh_scene(gpu, v, one))
    grid = check(scene, v, one, (0, 0, 0), 0.25, (4, 4, 4), 7)
    assert grid.sum() == 2 and grid[0, 0, 1] and grid[0, 0, 2]
    # a 16^3 grid over a one-triangle scene, with a cell that does not divide anything
    tri = np.array([(0.1, 0.2, 0.3), (0.9, 0.4, 0.2), (0.3, 0.8, 0.9)], F)
    grid = check(gpu.Scene(mesh_scene(gpu, tri, one)), tri, one, (-0.05, 0.03, 0.01), (0.07, 0.06, 0.065), (16, 16, 16), 1000)
    assert 16 < grid.sum() < 16 * 16 * 4
    # a 32^3 grid over the 2 k mesh
    case = dragon_case()
    lo, hi = bound_of(case["v"])
    grid = check(gpu.Scene(dragon()), case["v"], case["idx"], tuple(lo - 0.01), tuple((hi - lo + 0.02) / 32), (32, 32, 32), 10000)
    assert grid.any() and not grid[1:-1, 1:-1, 1:-1].all()   # surfaces, and air inside the Cornell box
    # a closed cube: fill sets what lies inside, and equals the chain with contains of the voxel centres
    cv, cidx = cube_mesh(0.21, 0.83)
    cube = gpu.Scene(mesh_scene(gpu, cv, cidx))
    shell = cube.voxelize((0, 0, 0), 0.125, (8, 8, 8))
    solid = cube.voxelize((0, 0, 0), 0.125, (8, 8, 8), fill=True, chunk=100)
    boxes = gpu.voxel_boxes((0, 0, 0), 0.125, (8, 8, 8))
    inside = cube.contains((0.5 * boxes[:, 0:3] + 0.5 * boxes[:, 4:7]).contiguous()) != 0
    torch.cuda.synchronize()
    assert torch.equal(solid, shell | inside.view(8, 8, 8))
    assert not shell[3:5, 3:5, 3:5].any() and solid[3:5, 3:5, 3:5].all() and (solid | ~shell).all() and not solid[0].any() and not solid[:, :, 7].any()
