"""Temporal accumulation (include/gnxr.h, "Temporal accumulation"): gnxr_camera_matrices against camera rays, the numpy restatement
(tests/temporal_reference.py) against closed forms, the refusals -- then on the GPU temporal_accumulate against the restatement on
seeded inputs that reach every branch, Scene.motion against the chain ray generation -> Scene.intersect -> reprojection, a static
frame, moved vertices, a disocclusion, and TemporalAccumulator against the chain of public calls.  Comparisons are on bits unless a
test says why not."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import gnxraytracer_amd
import oracle_lib as ol
import scenes
import temporal_reference as tr
from conftest import ROOT

ERR_INVALID, ERR_NO_DEVICE = -1, -2
f32 = np.float32
NAMES = ("gnxr_camera_matrices", "gnxr_motion_device", "gnxr_temporal_accumulate_device")
DEV = "cuda:0"


def cameras(gx):
    """a perspective and an orthographic camera in front of the Cornell box, each with the camera of the frame before: moved and turned
    by a few degrees"""
    return {"perspective": (gx.camera(eye=(0.3, 0.2, 5.0), look=(0.1, 0.0, 0.0), fov=80.0), gx.camera(eye=(0.0, 0.1, 5.2), look=(-0.2, 0.1, 0.0), up=(0.05, 1, 0), fov=80.0)),
            "orthographic": (gx.camera(eye=(0.2, 0.1, 5.0), look=(0.1, 0.0, 0.0), orthographic=True),
                             gx.camera(eye=(0.0, 0.0, 5.0), look=(-0.2, 0.05, 0.0), up=(0.04, 1, 0), orthographic=True))}


# ---------------------------------------------------------------- CPU: the ABI
def test_temporal_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(gx.lib(), name) and name in gx._abi.PROTOTYPES, name
    # no record joins gnxr_abi_sizeof's list, the version stays
    assert gx.lib().gnxr_abi_version() == 5 and gx.lib().gnxr_abi_sizeof(13) > 0 and gx.lib().gnxr_abi_sizeof(14) == -1
    A = gx._abi
    assert C.sizeof(A.MotionParams) == 16 and C.sizeof(A.MotionBuffers) == 32 and C.sizeof(A.TemporalParams) == 28 and C.sizeof(A.TemporalBuffers) == 88
    assert re.search(r"struct gnxr_motion_params\s*\{ int32_t struct_size, width, height, n_views; \}", hdr)
    assert re.search(r"struct gnxr_temporal_params \{ int32_t struct_size, width, height, n_views, max_history;\s*float depth_tol, normal_cos; \}", hdr)
    for name in ("camera_matrices", "temporal_accumulate", "TemporalAccumulator"):
        assert callable(getattr(gx, name))
    assert callable(gx.Scene.motion)


# ---------------------------------------------------------------- CPU: gnxr_camera_matrices
def round_trip(gx, cam, W, H, camera_rays, sample_halton):
    """points on camera rays project back to the film position of their sample; r2c and c2w give those rays on bits"""
    rng = np.random.default_rng([20261020, W, H, int(cam.orthographic)])
    n = 300
    px, py, s = rng.integers(0, W, n).astype(np.int32), rng.integers(0, H, n).astype(np.int32), rng.integers(0, 64, n).astype(np.int64)
    o, d = camera_rays(cam, W, H, px, py, s)
    fx, fy = (sample_halton(W, H, px, py, s, np.full(n, k, np.int32)) for k in (0, 1))
    m = gx.camera_matrices(cam, W, H)
    assert all(m[k].shape == (4, 4) and m[k].dtype == f32 for k in ("r2c", "c2w", "w2r"))
    w = m["w2r"].reshape(16)
    worst = 0.0
    for t in (f32(1), f32(4)):
        X, Y, Z = (o[:, k] + t * d[:, k] for k in range(3))
        row = lambda k: (w[4 * k] * X + w[4 * k + 1] * Y) + (w[4 * k + 2] * Z + w[4 * k + 3])
        xr, yr, ww = row(0), row(1), row(3)
        assert (ww > 0).all()
        xq, yq = np.where(ww == 1, xr, xr / ww), np.where(ww == 1, yr, yr / ww)
        worst = max(worst, float(np.abs(xq - (px + fx.astype(np.float64))).max()), float(np.abs(yq - (py + fy.astype(np.float64))).max()))
    print(f"camera_matrices round trip {W}x{H} ortho={cam.orthographic}: worst {worst:.3e} pixel")
    assert worst <= 1 / 64
    ro, rd = tr.camera_ray(m["r2c"], m["c2w"], bool(cam.orthographic), px.astype(f32) + fx, py.astype(f32) + fy)
    assert tr.biteq(rd, d) and tr.biteq(ro, o)


@pytest.mark.parametrize("size", [(37, 23), (16, 48)])
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_camera_matrices_round_trip(gx, kind, size):
    """the rays and film samples are the CPU oracle's (the library's own need a device: the GPU form of this test takes those)"""
    round_trip(gx, cameras(gx)[kind][0], size[0], size[1], ol.oracle_camera_rays, ol.oracle_halton)


def test_camera_matrices_refusals_and_null_outputs(gx):
    L = gx.lib()
    cam = gx.camera()
    m = np.zeros(16, f32)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    assert L.gnxr_camera_matrices(None, 8, 8, fp, fp, fp) == ERR_INVALID
    assert L.gnxr_camera_matrices(C.byref(cam), 0, 8, fp, fp, fp) == ERR_INVALID and L.gnxr_camera_matrices(C.byref(cam), 8, 0, fp, fp, fp) == ERR_INVALID
    assert L.gnxr_camera_matrices(C.byref(cam), 8, 8, None, None, None) == 0
    assert L.gnxr_camera_matrices(C.byref(cam), 8, 8, None, None, fp) == 0 and tr.biteq(m.reshape(4, 4), gx.camera_matrices(cam, 8, 8)["w2r"])
    with pytest.raises(ValueError):
        gx.camera_matrices("camera", 8, 8)


# ---------------------------------------------------------------- CPU: the restatement against closed forms
def identity_inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    motion = np.stack([xx + 0.5, yy + 0.5, np.full((H, W), 2.0), np.ones((H, W))], -1).astype(f32)[None]
    guide = np.tile(np.array([0, 0, 1, 2], f32), (1, H, W, 1))
    prim = rng.integers(-1, 3, (1, H, W)).astype(np.int32)
    return rng, motion, guide, prim


@pytest.mark.parametrize("M", [1, 4, 32])
def test_restated_accumulate_is_the_running_mean_up_to_max_history(M):
    """identity motion is one tap of weight 1: after k frames N = min(k, M) and, while k <= M, the colour is the fp32 recurrence
    H = H + (1 / k) * (c - H) -- the definition's alpha = 1 / N' times the difference, not a division by k"""
    rng, motion, guide, prim = identity_inputs(5, 7, 11)
    hist, Hc = None, None
    for k in range(1, 7):
        c = rng.random((1, 5, 7, 4)).astype(f32)
        oc, os_ = tr.accumulate(c, motion, guide, prim, hist, M, 0.05, 0.9)
        hist = {"color": oc, "stat": os_, "guide": guide, "prim": prim}
        assert (os_[..., 2] == min(k, M)).all()
        alpha = f32(1) / f32(min(k, M))
        Hc = c[..., :3] if k == 1 else Hc + alpha * (c[..., :3] - Hc)
        assert tr.biteq(oc[..., :3], Hc) and tr.biteq(oc[..., 3], c[..., 3])
        if k == 1:
            l = tr.lum(c[..., 0], c[..., 1], c[..., 2])
            assert tr.biteq(os_, np.stack([l, l * l, np.ones_like(l), np.zeros_like(l)], -1))
        assert (os_[..., 3] >= 0).all()


def test_restated_first_frame_never_reads_history():
    rng, motion, guide, prim = identity_inputs(3, 4, 5)
    c = rng.random((1, 3, 4, 4)).astype(f32)
    want = tr.accumulate(c, motion, guide, prim, None, 8, 0.05, 0.9)
    wild = np.full_like(motion, np.nan)
    wild[..., 3] = 1
    got = tr.accumulate(c, wild, np.full_like(guide, np.inf), prim, None, 8, 0.05, 0.9)
    assert tr.biteq(got[0], want[0]) and tr.biteq(got[1], want[1]) and tr.biteq(want[0], c) and (want[1][..., 2] == 1).all()
    # and with a history whose flag is 0 everywhere the same
    hist = {"color": c * 3, "stat": np.ones_like(c), "guide": guide, "prim": prim}
    motion[..., 3] = 0
    got = tr.accumulate(c, motion, guide, prim, hist, 8, 0.05, 0.9)
    assert tr.biteq(got[0], want[0]) and tr.biteq(got[1], want[1])


def test_restated_two_taps_weigh_by_their_share_and_drop_the_other_surface():
    """x' = 1.75 puts 0.75 / 0.25 on pixels 1 and 2 of a 4 x 1 row; with pixel 2 on another primitive only pixel 1 counts"""
    z = lambda *v: np.array(v, f32)
    hist = {"color": np.zeros((1, 1, 4, 4), f32), "stat": np.zeros((1, 1, 4, 4), f32), "guide": np.tile(z(0, 0, 1, 2), (1, 1, 4, 1)), "prim": np.zeros((1, 1, 4), np.int32)}
    hist["color"][0, 0, :, 0] = (8, 16, 32, 64)
    hist["stat"][0, 0, :, 2] = (1, 2, 4, 8)
    color = np.zeros((1, 1, 4, 4), f32)
    motion = np.tile(z(1.75, 0.5, 2, 1), (1, 1, 4, 1))
    guide = np.tile(z(0, 0, 1, 2), (1, 1, 4, 1))
    prim = np.zeros((1, 1, 4), np.int32)
    oc, os_ = tr.accumulate(color, motion, guide, prim, hist, 32, 0.05, 0.9)
    H = f32(0.75) * f32(16) + f32(0.25) * f32(32)            # 20, N = 2.5 -> N' = 3.5
    assert os_[0, 0, 0, 2] == f32(3.5) and oc[0, 0, 0, 0] == H + (f32(1) / f32(3.5)) * (f32(0) - H)
    hist["prim"][0, 0, 2] = 7
    oc, os_ = tr.accumulate(color, motion, guide, prim, hist, 32, 0.05, 0.9)
    assert os_[0, 0, 0, 2] == f32(3) and oc[0, 0, 0, 0] == f32(16) + (f32(1) / f32(3)) * (f32(0) - f32(16))


# ---------------------------------------------------------------- CPU: the refusals
def dummy_args():
    """host memory that passes every argument check and a 16-byte aligned address inside it (also the handle, which must not be touched)"""
    buf = (C.c_float * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    return buf, base


def test_temporal_calls_refuse_malformed_arguments_before_any_device(gx):
    L, A = gx.lib(), gx._abi
    buf, base = dummy_args()
    vp = C.c_void_p
    p, odd2, dummy = vp(base), vp(base + 2), vp(base)
    err = lambda: L.gnxr_last_error()
    cam = gx.camera()
    cams = (gx.Camera * 2)(cam, cam)

    def motion(scene=dummy, params=None, cameras=cams, prev=cams, pv=None, bufs=None, W=8, H=8, V=2, psize=16, bsize=32, ch=(base, base + 4096, base + 8192)):
        pp = params if params is not None else A.MotionParams(psize, W, H, V)
        bb = bufs if bufs is not None else A.MotionBuffers(bsize, 0, *[vp(c) if c else None for c in ch])
        return L.gnxr_motion_device(scene, C.byref(pp) if pp else None, cameras, prev, pv, C.byref(bb) if bb else None, None)

    assert motion(scene=None) == ERR_INVALID and b"null" in err()
    assert L.gnxr_motion_device(dummy, None, cams, cams, None, C.byref(A.MotionBuffers(32, 0, p, p, p)), None) == ERR_INVALID
    assert L.gnxr_motion_device(dummy, C.byref(A.MotionParams(16, 8, 8, 2)), cams, cams, None, None, None) == ERR_INVALID
    assert motion(prev=None) == ERR_INVALID and b"null" in err()
    assert motion(psize=20) == ERR_INVALID and b"struct_size" in err()
    assert motion(bsize=24) == ERR_INVALID and b"struct_size" in err()
    assert motion(ch=(0, 0, 0)) == ERR_INVALID and b"channel" in err()
    assert motion(cameras=None) == ERR_INVALID and b"null cameras" in err()
    assert motion(W=0) == ERR_INVALID and motion(H=0) == ERR_INVALID and motion(V=-1) == ERR_INVALID
    assert motion(ch=(base + 4, 0, 0)) == ERR_INVALID and b"aligned" in err()
    assert motion(ch=(0, base + 8, 0)) == ERR_INVALID and b"aligned" in err()
    assert motion(ch=(0, 0, base + 2)) == ERR_INVALID and b"aligned" in err()
    assert motion(pv=odd2) == ERR_INVALID and b"aligned" in err()
    assert motion(W=32768, H=32768) == ERR_INVALID and b"path indexing" in err()
    assert motion(V=0) == 0 and motion(V=0, cameras=None) == 0                 # a no-op, the handle untouched

    def accumulate(params=None, io=None, W=8, H=8, V=1, M=32, tol=0.05, cosn=0.9, psize=28, bsize=88, ptrs=None, **named):
        names = ("d_color", "d_motion", "d_guide", "d_prim", "d_hist_color", "d_hist_stat", "d_hist_guide", "d_hist_prim", "d_out_color", "d_out_stat")
        at = {k: base + 1024 * i for i, k in enumerate(names)}                 # 1024 bytes apart: 64 pixels of 16 bytes
        at.update(named)
        pp = A.TemporalParams(psize, W, H, V, M, tol, cosn)
        bb = A.TemporalBuffers(bsize, 0, *[vp(at[k]) if at[k] else None for k in names])
        return L.gnxr_temporal_accumulate_device(C.byref(pp), C.byref(bb), None)

    ok_io = A.TemporalBuffers(88, 0, *[vp(base + 1024 * i) for i in range(10)])
    assert L.gnxr_temporal_accumulate_device(None, C.byref(ok_io), None) == ERR_INVALID and b"null" in err()
    assert L.gnxr_temporal_accumulate_device(C.byref(A.TemporalParams(28, 8, 8, 1, 32, 0.05, 0.9)), None, None) == ERR_INVALID
    for k in ("d_color", "d_motion", "d_guide", "d_prim", "d_out_color", "d_out_stat"):
        assert accumulate(**{k: 0}) == ERR_INVALID and b"required" in err(), k
    assert accumulate(psize=32) == ERR_INVALID and b"struct_size" in err()
    assert accumulate(bsize=80) == ERR_INVALID and b"struct_size" in err()
    for k in ("d_hist_color", "d_hist_stat", "d_hist_guide", "d_hist_prim"):
        assert accumulate(**{k: 0}) == ERR_INVALID and b"history" in err(), k
    assert accumulate(W=0) == ERR_INVALID and accumulate(H=0) == ERR_INVALID and accumulate(V=-1) == ERR_INVALID
    assert accumulate(M=0) == ERR_INVALID and b"max_history" in err()
    assert accumulate(tol=-0.1) == ERR_INVALID and accumulate(tol=float("nan")) == ERR_INVALID and b"depth_tol" in err()
    assert accumulate(cosn=float("nan")) == ERR_INVALID
    for k in ("d_color", "d_motion", "d_guide", "d_hist_color", "d_hist_stat", "d_hist_guide", "d_out_color", "d_out_stat"):
        assert accumulate(**{k: base + 16 * 1024 + 4}) == ERR_INVALID and b"16-byte aligned" in err(), k
    for k in ("d_prim", "d_hist_prim"):
        assert accumulate(**{k: base + 16 * 1024 + 2}) == ERR_INVALID and b"4-byte aligned" in err(), k
    # an output overlaps no input (the gather reads neighbours), nor the other output: the same address and a partial overlap
    for k in ("d_color", "d_motion", "d_guide", "d_prim", "d_hist_color", "d_hist_stat", "d_hist_guide", "d_hist_prim"):
        src = base + 1024 * ("d_color", "d_motion", "d_guide", "d_prim", "d_hist_color", "d_hist_stat", "d_hist_guide", "d_hist_prim").index(k)
        assert accumulate(d_out_color=src) == ERR_INVALID and b"overlaps" in err(), k
    assert accumulate(d_out_stat=base + 1024 * 4 + 512) == ERR_INVALID and b"overlaps" in err()
    assert accumulate(d_out_stat=base + 1024 * 8 + 16) == ERR_INVALID and b"overlaps" in err()
    assert accumulate(W=32768, H=32768, V=2) == ERR_INVALID and b"path indexing" in err()
    assert accumulate(V=0) == 0
    # arguments that pass every check need the runtime: no CPU fallback
    if not torch.cuda.is_available():
        assert motion() == ERR_NO_DEVICE and accumulate() == ERR_NO_DEVICE
        assert accumulate(d_hist_color=0, d_hist_stat=0, d_hist_guide=0, d_hist_prim=0) == ERR_NO_DEVICE
    del buf


# ---------------------------------------------------------------- GPU helpers
def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


NORMALS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], f32)
PERP = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 0]], f32)     # a unit vector perpendicular to each of NORMALS
CASES = ("centre", "snap", "fraction", "border", "wild", "flag0", "other_prim", "depth_in", "depth_out", "normal_in", "normal_out")
TOL, COSN = 0.05, 0.9


def accumulate_inputs(V, H, W):
    """seeded inputs of temporal_accumulate that reach every branch of the definition: a history in blocks of 3 x 3 pixels of one
    primitive (-1 among them), and for every pixel a case of CASES that aims it at a place of the history and takes its own primitive,
    normal and expected depth from what lies there, moved just inside or outside a tolerance where the case says so"""
    rng = np.random.default_rng([20261020, V, H, W])
    vv, yy, xx = np.mgrid[0:V, 0:H, 0:W]
    hp = ((xx // 3 + 2 * (yy // 3) + vv) % 5 - 1).astype(np.int32)
    hit = hp >= 0
    hn = np.where(hit[..., None], NORMALS[hp % 4], 0).astype(f32)
    ht = np.where(hit, 2 + 0.01 * xx + 0.02 * yy + 0.5 * vv, 0).astype(f32)
    hN = np.where(rng.random((V, H, W)) < 0.05, 0, rng.integers(1, 41, (V, H, W))).astype(f32)
    hc = (2 * rng.random((V, H, W, 4))).astype(f32)
    m1 = rng.random((V, H, W)).astype(f32)
    hs = np.stack([m1, m1 * m1 + f32(0.1) * rng.random((V, H, W)).astype(f32), hN, np.zeros((V, H, W), f32)], -1).astype(f32)
    wild = np.array([np.nan, np.inf, -np.inf], f32)
    for arr, chans in ((hc, 3), (hs, 2)):
        bad = rng.random((V, H, W)) < 0.02
        arr[bad, rng.integers(0, chans, int(bad.sum()))] = wild[rng.integers(0, 3, int(bad.sum()))]
    case = rng.integers(0, len(CASES), (V, H, W))
    name = np.array(CASES)[case]
    tx = xx + rng.integers(-2, 3, (V, H, W)).astype(np.float64)
    ty = yy + rng.integers(-2, 3, (V, H, W)).astype(np.float64)
    snap = name == "snap"
    tx, ty = tx + snap * rng.uniform(-1 / 300, 1 / 300, (V, H, W)), ty + snap * rng.uniform(-1 / 300, 1 / 300, (V, H, W))
    frac = name == "fraction"
    tx, ty = np.where(frac, xx + rng.uniform(-3, 3, (V, H, W)), tx), np.where(frac, yy + rng.uniform(-3, 3, (V, H, W)), ty)
    border = name == "border"      # within one pixel outside a border: left / right, or top / bottom
    side = rng.integers(0, 4, (V, H, W))
    u = rng.uniform(0, 1, (V, H, W))
    tx = np.where(border & (side == 0), -1 + u, np.where(border & (side == 1), W - 1 + u, tx))
    ty = np.where(border & (side == 2), -1 + u, np.where(border & (side == 3), H - 1 + u, ty))
    # what lies at the aim: the nearest pixel of the history inside the image
    qx, qy = np.clip(np.rint(tx), 0, W - 1).astype(int), np.clip(np.rint(ty), 0, H - 1).astype(int)
    prim = hp[vv, qy, qx].copy()
    n = hn[vv, qy, qx].copy()
    t = ht[vv, qy, qx].copy()
    prim[name == "other_prim"] += 1
    t = np.where(name == "depth_in", t / f32(1 + TOL * 0.95), np.where(name == "depth_out", t / f32(1 + TOL * 1.05), t)).astype(f32)
    ang = np.where(name == "normal_in", np.arccos(COSN) - 0.01, np.where(name == "normal_out", np.arccos(COSN) + 0.01, 0.0))
    perp = np.where((prim >= 0)[..., None], PERP[hp[vv, qy, qx] % 4], 0)
    n = (np.cos(ang)[..., None] * n + np.sin(ang)[..., None] * perp).astype(f32)
    motion = np.stack([tx + 0.5, ty + 0.5, t, np.ones((V, H, W))], -1).astype(f32)
    w = name == "wild"
    wild4 = np.array([np.nan, np.inf, -np.inf, 1e30], f32)
    motion[w, rng.integers(0, 3, int(w.sum()))] = wild4[rng.integers(0, 4, int(w.sum()))]
    motion[name == "flag0", 3] = 0
    color = (2 * rng.random((V, H, W, 4))).astype(f32)
    bad = rng.random((V, H, W)) < 0.03
    color[bad, rng.integers(0, 3, int(bad.sum()))] = wild[rng.integers(0, 3, int(bad.sum()))]
    guide = np.concatenate([n, t[..., None]], -1).astype(f32)
    cross = None
    if V > 1 and W > 2:
        # a pixel on view 0's last row aimed half a pixel below it: the lower taps are outside the image -- in memory, view 1's first
        # row, which is made to look like the same surface in another colour
        x = W // 2
        cross = (0, H - 1, x)
        hp[0, H - 1, x - 1:x + 2] = 2; hn[0, H - 1, x - 1:x + 2] = NORMALS[2]; ht[0, H - 1, x - 1:x + 2] = 3; hs[0, H - 1, x - 1:x + 2] = (0.5, 0.3, 4, 0.05); hc[0, H - 1, x - 1:x + 2] = 1
        hp[1, 0, x - 1:x + 2] = 2; hn[1, 0, x - 1:x + 2] = NORMALS[2]; ht[1, 0, x - 1:x + 2] = 3; hs[1, 0, x - 1:x + 2] = (0.5, 0.3, 4, 0.05); hc[1, 0, x - 1:x + 2] = 100
        prim[cross] = 2; guide[cross] = (*NORMALS[2], 3); motion[cross] = (x + 0.5, H, 3, 1); color[cross] = 1
    hist = {"color": hc, "stat": hs, "guide": np.concatenate([hn, ht[..., None]], -1).astype(f32), "prim": hp}
    return {"color": color, "motion": motion, "guide": guide, "prim": prim.astype(np.int32), "history": hist, "cross": cross}


BRANCHES = ("flag0", "out_of_range", "snapped", "fractional", "one_tap", "four_taps", "miss_pair", "tap_outside", "tap_zero_length", "tap_prim", "tap_nonfinite",
            "tap_depth", "tap_normal", "close_depth", "close_normal", "blend", "first", "keep_history", "nothing", "clamped")


def test_accumulate_inputs_reach_every_branch_by_the_restatement_alone():
    """before any device is involved: every branch of the definition is taken by at least one pixel of the seeded inputs of the two
    larger sizes, and the pixel on a view's last row that aims below it has its lower taps outside the image"""
    for V, H, W, M in ((2, 23, 37, 32), (1, 64, 64, 1)):
        a = accumulate_inputs(V, H, W)
        br = {}
        oc, _ = tr.accumulate(a["color"], a["motion"], a["guide"], a["prim"], a["history"], M, TOL, COSN, branches=br)
        missing = [k for k in BRANCHES if not br[k].any()]
        assert not missing, (V, H, W, missing)
        wild = a["motion"][..., :2]
        for bad in (np.isnan(wild).any(-1), np.isposinf(wild).any(-1), np.isneginf(wild).any(-1), (wild == f32(1e30)).any(-1)):
            assert (bad & (a["motion"][..., 3] != 0)).any() and (br["out_of_range"] | ~bad | (a["motion"][..., 3] == 0)).all()
        if a["cross"]:
            assert br["tap_outside"][a["cross"]] and br["blend"][a["cross"]] and oc[a["cross"]][0] == 1      # view 1's 100 stays out


# ---------------------------------------------------------------- GPU 1: accumulate against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("V,H,W,M,first", [(2, 23, 37, 32, False), (1, 64, 64, 1, False), (1, 64, 64, 32, False), (1, 1, 1, 32, False), (2, 23, 37, 32, True), (1, 1, 1, 1, True)])
def test_accumulate_equals_the_restatement_on_bits(gpu, V, H, W, M, first):
    a = accumulate_inputs(V, H, W)
    hist = None if first else a["history"]
    want_c, want_s = tr.accumulate(a["color"], a["motion"], a["guide"], a["prim"], hist, M, TOL, COSN)
    dh = None if first else {k: dev(v) for k, v in hist.items()}
    got = gpu.temporal_accumulate(dev(a["color"]), dev(a["motion"]), dev(a["guide"]), dev(a["prim"]), history=dh, max_history=M, depth_tol=TOL, normal_cos=COSN)
    gc, gs = host(got["color"]), host(got["stat"])
    diff = (gc.view(np.int32) != want_c.view(np.int32)).any(-1) | (gs.view(np.int32) != want_s.view(np.int32)).any(-1)
    print(f"accumulate {V}x{H}x{W} M={M} first={first}: {int(diff.sum())} of {diff.size} pixels differ")
    assert not diff.any(), np.argwhere(diff)[:8]
    assert got["guide"].data_ptr() == dev(a["guide"]).data_ptr() or tr.biteq(host(got["guide"]), a["guide"])
    assert (host(got["prim"]) == a["prim"]).all()
    # 3-dimensional tensors are one view
    if V == 1:
        g3 = gpu.temporal_accumulate(dev(a["color"][0]), dev(a["motion"][0]), dev(a["guide"][0]), dev(a["prim"][0]),
                                     history=None if first else {k: dev(v[0]) for k, v in hist.items()}, max_history=M, depth_tol=TOL, normal_cos=COSN)
        assert tuple(g3["color"].shape) == (H, W, 4) and tr.biteq(host(g3["color"]), want_c[0]) and tr.biteq(host(g3["stat"]), want_s[0])


@pytest.mark.gpu
def test_accumulate_python_checks_and_device_refusals(gpu):
    a = accumulate_inputs(1, 5, 6)
    c, m, g, p = dev(a["color"]), dev(a["motion"]), dev(a["guide"]), dev(a["prim"])
    ok = gpu.temporal_accumulate(c, m, g, p)
    for bad in (dict(color=c.cpu()), dict(color=c[..., :3]), dict(motion=m[:, :4]), dict(prim=p.float()), dict(guide=g.double()), dict(max_history=0), dict(depth_tol=-1.0),
                dict(normal_cos=float("nan")), dict(history={"color": c}), dict(history=dict(ok, prim=p.float())), dict(out={"colour": c}), dict(out={"color": c[0]})):
        kw = dict(color=c, motion=m, guide=g, prim=p)
        kw.update(bad)
        with pytest.raises(ValueError):
            gpu.temporal_accumulate(**kw)
    with pytest.raises(gpu.GnxrError, match="overlaps"):
        gpu.temporal_accumulate(c, m, g, p, history=ok, out={"color": ok["color"]})
    with pytest.raises(gpu.GnxrError, match="overlaps"):
        gpu.temporal_accumulate(c, m, g, p, out={"stat": m})
    # host memory where device memory belongs
    L, A = gpu.lib(), gpu._abi
    hostbuf = np.zeros((5 * 6, 4), f32)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    oc, os_ = torch.empty_like(c), torch.empty_like(c)
    io = A.TemporalBuffers(88, 0, C.c_void_p(hostbuf.ctypes.data), ptr(m), ptr(g), ptr(p), None, None, None, None, ptr(oc), ptr(os_))
    assert L.gnxr_temporal_accumulate_device(C.byref(A.TemporalParams(28, 6, 5, 1, 32, 0.05, 0.9)), C.byref(io), None) == ERR_INVALID
    assert b"not device memory" in L.gnxr_last_error()
    # preallocated outputs and a side stream give the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = {"color": oc, "stat": os_}
    got = gpu.temporal_accumulate(c, m, g, p, history=ok, out=out, stream=side)
    side.synchronize()
    want = gpu.temporal_accumulate(c, m, g, p, history=ok)
    assert got["color"] is oc and torch.equal(oc.view(torch.int32), want["color"].view(torch.int32)) and torch.equal(os_.view(torch.int32), want["stat"].view(torch.int32))


# ---------------------------------------------------------------- GPU 2 - 5: motion
BOX_LO, BOX_HI = (-1.7, -2.5, -1.3), (-0.6, 0.7, -0.2)
W0, H0 = 37, 23


def temporal_scene():
    """the small Cornell scene with a sphere, and a tall box whose 8 vertices are the last of the scene's: (builder, first vertex of the
    box, first triangle of the box)"""
    b = scenes.cornell_sphere("matte", center=(0.9, -1.6, 0.4), radius=0.8)
    first_vertex = b.desc().n_vertices
    v, i = scenes.box_mesh(BOX_LO, BOX_HI)
    first_tri = b.add_mesh(v, i, b.MatteMaterial(scenes.WHITE, 60.0))
    return b, first_vertex, first_tri


def scene_arrays(b):
    d = b.desc()
    return (np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(f32).copy(), np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int32).copy())


def chain(gx, intersect, indices, cam, prev, W, H, prev_vertices=None):
    """numpy ray generation -> `intersect` (rays -> gnxr_hit records) -> numpy reprojection"""
    rays = tr.centre_rays(gx, cam, W, H)
    hits = intersect(rays)
    corners = None
    if prev_vertices is not None:
        is_tri = (hits["prim"] >= 0) & (hits["prim"] < len(indices))
        corners = (prev_vertices[indices[np.where(is_tri, hits["prim"], 0)]], is_tri)
    return tr.reproject(gx, rays, hits, cam, prev, W, H, corners)


def device_intersect(scene):
    return lambda rays: np.ascontiguousarray(host(scene.intersect(dev(rays)).hits)).view(gnxraytracer_amd.HIT_DTYPE).reshape(-1)


def shaped(a, H, W):
    return a.reshape((H, W) + a.shape[1:])


@pytest.fixture(scope="module")
def live(gpu):
    b, first_vertex, first_tri = temporal_scene()
    return {"b": b, "scene": gpu.Scene(b), "first_vertex": first_vertex, "first_tri": first_tri, "arrays": scene_arrays(b)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_motion_equals_its_chain_on_bits(gpu, live, kind):
    cam, prev = cameras(gpu)[kind]
    scene = live["scene"]
    got = scene.motion(W0, H0, [prev], cameras=[cam])
    wm, wg, wp = chain(gpu, device_intersect(scene), live["arrays"][1], cam, prev, W0, H0)
    assert tuple(got["motion"].shape) == (1, H0, W0, 4) and tuple(got["prim"].shape) == (1, H0, W0)
    gm, gg, gp = host(got["motion"])[0], host(got["guide"])[0], host(got["prim"])[0]
    nt = len(live["arrays"][1])
    print(f"motion {kind}: {int((gp < 0).sum())} misses, {int((gp >= nt).sum())} sphere pixels, {int((gm[..., 3] == 0).sum())} unflagged of {gp.size}")
    assert (gp < 0).any() and (gp >= nt).any() and ((gp >= 0) & (gp < nt)).any()        # misses, the sphere and triangles are all in view
    assert (gp == shaped(wp, H0, W0)).all()
    assert tr.biteq(gg, shaped(wg, H0, W0))
    assert tr.biteq(gm, shaped(wm, H0, W0))
    # the scene's own camera (cameras=None) drops the leading dimension; several views are the single views stacked
    scene.set_camera(tuple(cam.eye), tuple(cam.look), tuple(cam.up), cam.fov_deg, cam.lens_radius, cam.focal_distance, bool(cam.orthographic))
    own = scene.motion(W0, H0, prev)
    assert tuple(own["motion"].shape) == (H0, W0, 4) and tr.biteq(host(own["motion"]), gm) and tr.biteq(host(own["guide"]), gg) and (host(own["prim"]) == gp).all()
    two = scene.motion(W0, H0, [prev, cam], cameras=[cam, prev])
    assert tr.biteq(host(two["motion"])[0], gm) and tr.biteq(host(two["guide"])[0], gg)
    back = chain(gpu, device_intersect(scene), live["arrays"][1], prev, cam, W0, H0)
    assert tr.biteq(host(two["motion"])[1], shaped(back[0], H0, W0)) and (host(two["prim"])[1] == shaped(back[2], H0, W0)).all()
    scene.set_camera()


@pytest.mark.gpu
def test_motion_python_checks(gpu, live):
    scene, cam = live["scene"], gpu.camera()
    for kw in (dict(prev_cameras=None), dict(prev_cameras=["cam"]), dict(prev_cameras=[cam, cam]), dict(prev_cameras=[cam], cameras=[cam, cam]), dict(width=0),
               dict(prev_vertices=torch.zeros((3, 3), device=DEV)), dict(prev_vertices=np.zeros((scene.n_vertices, 3), f32)), dict(out={"depth": None}),
               dict(out={"prim": torch.zeros((H0, W0), device=DEV)})):
        args = dict(width=W0, height=H0, prev_cameras=cam)
        args.update(kw)
        with pytest.raises(ValueError):
            scene.motion(**args)
    pre = {"prim": torch.full((H0, W0), -99, dtype=torch.int32, device=DEV)}
    got = scene.motion(W0, H0, cam, out=pre)
    assert got["prim"] is pre["prim"] and (host(pre["prim"]) != -99).all()


def static_checks(motion, guide, prim, W, H, sel=None):
    yy, xx = np.mgrid[0:H, 0:W]
    sel = np.ones((H, W), bool) if sel is None else sel
    assert (motion[..., 3][sel] == 1).all()
    dx, dy = np.abs(motion[..., 0] - (xx + 0.5))[sel], np.abs(motion[..., 1] - (yy + 0.5))[sel]
    assert dx.max() <= 1 / 64 and dy.max() <= 1 / 64, (dx.max(), dy.max())
    hitp = sel & (prim >= 0)
    rel = np.abs(motion[..., 2][hitp] - guide[..., 3][hitp]) / guide[..., 3][hitp]
    assert rel.max() <= 1e-4, rel.max()
    assert (motion[..., 2][sel & (prim < 0)] == 0).all()
    return float(max(dx.max(), dy.max())), float(rel.max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_static_frame_reprojects_onto_itself_and_history_grows_everywhere(gpu, live, kind):
    cam = cameras(gpu)[kind][0]
    mo = live["scene"].motion(W0, H0, cam, cameras=[cam])
    m, g, p = host(mo["motion"])[0], host(mo["guide"])[0], host(mo["prim"])[0]
    worst = static_checks(m, g, p, W0, H0)
    print(f"static {kind}: worst offset {worst[0]:.3e} pixel, worst relative depth {worst[1]:.3e}")
    assert (p < 0).any() and (p >= 0).any()
    color = dev(np.random.default_rng(3).random((1, H0, W0, 4)).astype(f32))
    hist = None
    for k in range(3):
        hist = gpu.temporal_accumulate(color, mo["motion"], mo["guide"], mo["prim"], history=hist)
    assert (host(hist["stat"])[..., 2] == 3).all()          # hits and misses alike
    assert np.abs(host(hist["color"]) - host(color)).max() <= 1e-6


@pytest.mark.gpu
def test_moved_vertices_report_their_motion_only_with_the_previous_vertex_array(gpu):
    b, first_vertex, first_tri = temporal_scene()
    scene = gpu.Scene(b)
    verts, indices = scene_arrays(b)
    cam = cameras(gpu)["perspective"][0]
    delta = np.array([0.3, 0.0, 0.1], f32)
    moved = verts[first_vertex:] + delta
    scene.update_vertices(np.ascontiguousarray(moved, f32), first_vertex=first_vertex)
    with_prev = scene.motion(W0, H0, cam, cameras=[cam], prev_vertices=dev(verts))
    without = scene.motion(W0, H0, cam, cameras=[cam])
    m, g, p = host(with_prev["motion"])[0], host(with_prev["guide"])[0], host(with_prev["prim"])[0]
    on_box = (p >= first_tri) & (p < first_tri + 12)
    assert on_box.sum() > 10 and (~on_box).sum() > 10
    assert (host(without["prim"])[0] == p).all() and tr.biteq(host(without["guide"])[0], g)
    # the moved mesh: the projection of P - delta, in double
    rays = shaped(tr.centre_rays(gpu, cam, W0, H0), H0, W0).astype(np.float64)
    P = rays[..., 0:3] + g[..., 3:4].astype(np.float64) * rays[..., 4:7]
    w2r = gpu.camera_matrices(cam, W0, H0)["w2r"].astype(np.float64)
    q = np.concatenate([P - delta, np.ones((H0, W0, 1))], -1) @ w2r.T
    want = q[..., :2] / q[..., 3:4]
    err = np.abs(m[..., :2] - want)[on_box]
    print(f"moved vertices: {int(on_box.sum())} pixels on the mesh, worst {err.max():.3e} pixel from the projection of P - delta; it moved by "
          f"{np.abs(want - np.stack(np.mgrid[0:H0, 0:W0][::-1], -1) - 0.5)[on_box].max():.2f} pixels")
    assert err.max() <= 1 / 64 and (m[..., 3][on_box] == 1).all()
    # the scene is in bits what a chain with the previous corners gives, and every other pixel is a static one
    wm, wg, wp = chain(gpu, device_intersect(scene), indices, cam, cam, W0, H0, prev_vertices=verts)
    assert tr.biteq(m, shaped(wm, H0, W0))
    static_checks(m, g, p, W0, H0, sel=~on_box)
    # without the previous vertices the same pixels report no motion
    static_checks(host(without["motion"])[0], g, p, W0, H0)


def palette(prim):
    table = np.random.default_rng(9).random((64, 3)).astype(f32) + f32(0.25)
    return table[(prim + 1) % 64]


def disocclusion(gx, intersect, indices, W, H):
    """frame A, then frame B from a camera moved sideways past the edge of the tall box; history and colour are palette[prim]:
    (reference colour, reference stat, the inputs)"""
    camA = gx.camera(eye=(0.0, 0.0, 5.0), look=(0.0, 0.0, 0.0), fov=80.0)
    camB = gx.camera(eye=(0.9, 0.0, 5.0), look=(0.9, 0.0, 0.0), fov=80.0)
    mA, gA, pA = (shaped(a, H, W)[None] for a in chain(gx, intersect, indices, camA, camA, W, H))
    mB, gB, pB = (shaped(a, H, W)[None] for a in chain(gx, intersect, indices, camB, camA, W, H))
    colA = np.concatenate([palette(pA), np.ones((1, H, W, 1), f32)], -1)
    colB = np.concatenate([palette(pB), np.ones((1, H, W, 1), f32)], -1)
    c1, s1 = tr.accumulate(colA, mA, gA, pA, None, 32, 0.05, 0.9)
    hist = {"color": c1, "stat": s1, "guide": gA, "prim": pA}
    c2, s2 = tr.accumulate(colB, mB, gB, pB, hist, 32, 0.05, 0.9)
    return c2, s2, dict(camA=camA, camB=camB, colA=colA, colB=colB, pB=pB)


def disocclusion_checks(color, stat, colB, pB):
    ulp = np.spacing(np.abs(colB[..., :3]))
    assert (np.abs(color[..., :3] - colB[..., :3]) <= 4 * ulp).all()       # history never leaks between surfaces
    N = stat[..., 2]
    hitp = pB >= 0
    assert (N >= 1).all() and (N[hitp] == 1).any() and (N[hitp] > 1).mean() >= 0.5
    return int((N[hitp] == 1).sum()), float((N[hitp] > 1).mean())


DW, DH = 64, 40


def test_disocclusion_by_the_restatement_and_the_cpu_oracle():
    """the same chain with the CPU oracle's Scene::Intersect in place of the device's: the shift meets both conditions before a GPU is involved"""
    b, _, _ = temporal_scene()
    o = ol.OracleScene(b)
    c2, s2, inp = disocclusion(gnxraytracer_amd, o.Intersect, scene_arrays(b)[1], DW, DH)
    n1, share = disocclusion_checks(c2, s2, inp["colB"], inp["pB"])
    print(f"disocclusion (oracle): {n1} hit pixels start over, {share:.2f} of the hit pixels keep their history")


@pytest.mark.gpu
def test_no_ghosting_across_a_disocclusion(gpu, live):
    scene = live["scene"]
    c2, s2, inp = disocclusion(gpu, device_intersect(scene), live["arrays"][1], DW, DH)
    n1, share = disocclusion_checks(c2, s2, inp["colB"], inp["pB"])
    moA = scene.motion(DW, DH, [inp["camA"]], cameras=[inp["camA"]])
    moB = scene.motion(DW, DH, [inp["camA"]], cameras=[inp["camB"]])
    assert (host(moB["prim"]) == inp["pB"]).all()
    hist = gpu.temporal_accumulate(dev(inp["colA"]), moA["motion"], moA["guide"], moA["prim"])
    got = gpu.temporal_accumulate(dev(inp["colB"]), moB["motion"], moB["guide"], moB["prim"], history=hist)
    gn1, gshare = disocclusion_checks(host(got["color"]), host(got["stat"]), inp["colB"], inp["pB"])
    print(f"disocclusion: {gn1} hit pixels start over ({n1} by the restatement), {gshare:.2f} of the hit pixels keep their history")
    assert tr.biteq(host(got["color"]), c2) and tr.biteq(host(got["stat"]), s2)


# ---------------------------------------------------------------- GPU 6: TemporalAccumulator
@pytest.mark.gpu
def test_temporal_accumulator_is_its_chain_and_converges_to_the_full_render(gpu):
    b, _, _ = temporal_scene()
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    W = H = 32
    M, spp = 8, 4
    acc = gpu.TemporalAccumulator(integ, scene, W, H, spp, max_history=M)
    hist, frames = None, []
    st = torch.cuda.current_stream()
    for k in range(M):
        got = acc.frame()
        img = torch.zeros((H, W, 4), dtype=torch.float32, device=DEV)
        integ.RenderDevice(scene, img.data_ptr(), W, H, M * spp, stream=st.cuda_stream, spp_begin=k * spp, spp_end=(k + 1) * spp)
        img[..., :3] *= float(M)
        mo = scene.motion(W, H, scene.camera)
        hist = gpu.temporal_accumulate(img, mo["motion"], mo["guide"], mo["prim"], history=hist, max_history=M)
        frames.append(host(img))
        for key in ("color", "stat", "guide"):
            assert torch.equal(got[key].view(torch.int32), hist[key].view(torch.int32)), (k, key)
        assert torch.equal(got["prim"], hist["prim"]) and torch.equal(got["motion"].view(torch.int32), mo["motion"].view(torch.int32))
    assert (host(hist["stat"])[..., 2] == M).all()
    full, _ = integ.Render(scene, W, H, M * spp)
    bound = 4e-6 * np.abs(np.stack(frames)).max(0)[..., :3]
    err = np.abs(host(hist["color"])[..., :3].astype(np.float64) - full[..., :3])
    print(f"accumulator against Render(spp={M * spp}): worst error {err.max():.3e}, worst error / bound {np.max(err / np.maximum(bound, 1e-30)):.3f}")
    assert (err <= bound).all()
    # the ninth frame wraps around to the first range of samples; reset() starts over
    again = acc.frame(denoise=True)
    assert (host(again["stat"])[..., 2] == M).all() and tuple(again["denoised"].shape) == (H, W, 4) and torch.isfinite(again["denoised"]).all()
    acc.reset()
    assert (host(acc.frame()["stat"])[..., 2] == 1).all()
    with pytest.raises(ValueError):
        gpu.TemporalAccumulator(integ, scene, W, H, 0)
    with pytest.raises(ValueError):
        acc.frame(camera="camera")
    # a camera that moves every frame
    orbit = gpu.TemporalAccumulator(integ, scene, W, H, spp, max_history=M)
    for k in range(6):
        a = 0.03 * k
        got = orbit.frame(gpu.camera(eye=(5.0 * np.sin(a), 0.1, 5.0 * np.cos(a)), look=(0, 0, 0), fov=80.0))
        assert torch.isfinite(got["color"]).all()
    N, p = host(got["stat"])[..., 2], host(got["prim"])
    print(f"orbit: mean history length over hit pixels {N[p >= 0].mean():.2f}")
    assert N[p >= 0].mean() > 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_camera_matrices_round_trip_with_the_library_s_own_rays(gpu, kind):
    """the form the issue words: rays from gnxr_camera_rays, film samples from gnxr_sample_halton"""
    for W, H in ((37, 23), (16, 48)):
        round_trip(gpu, cameras(gpu)[kind][0], W, H, gpu.camera_rays, gpu.sample_halton)
