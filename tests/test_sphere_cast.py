"""Sphere casts (include/gnxr.h, "Sphere casts"): the numpy restatement (tests/spherecast_reference.py) on hand-made cases, the refusals of
the C calls and of the Python method without a device, then gnxr_sphere_cast_device / gnxr_sphere_cast on the GPU against the
restatement's brute force over all triangles.  Every comparison of records is on their bytes; one check in float64 is independent of
the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import scenes
import spherecast_reference as sr
from conftest import ROOT
from query_cases import (assert_same, bound_of, chain_scene, concentric_mesh, dragon, fan_mesh, mesh_of, mesh_scene, sliver_mesh, surface_samples,
                         uniform_in)

ERR_INVALID = -1
F = np.float32
INF = F(np.inf)
EMPTY = sr.empty_records(1)[0]


# ---------------------------------------------------------------- helpers
def device_casts(scene, casts, **kw):
    """the records (sr.RECORD) of one device call on ready-made (n, 8) records"""
    c = torch.from_numpy(np.array(casts, F).reshape(-1, 8)).cuda()
    res = scene.sphere_cast(c, None, None, **kw)
    torch.cuda.synchronize()
    return res.records.cpu().numpy().view(sr.RECORD).reshape(len(c))


def check(scene, v, idx, casts, want=None, what=""):
    want = sr.sphere_casts(v, idx, casts) if want is None else want
    assert_same(device_casts(scene, casts), want, what)
    return want


def directions(n, rng):
    """random directions of lengths 0.05 .. 20, one in eight along an axis"""
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = rng.random(n) < 0.125
    d[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-1.0, 1.0], (axis.sum(), 1))
    return (d * np.exp(rng.uniform(np.log(0.05), np.log(20), (n, 1)))).astype(F)


def towards(origins, targets, rng):
    """directions from origins to targets, scaled so that the target is reached at t = 0.25 .. 4"""
    return ((targets - origins) / rng.uniform(0.25, 4, (len(origins), 1))).astype(F)


def cornell_case():
    """400 casts in the Cornell box (12 triangles: five walls and the light, open towards +z) from on, near and far from the walls, with
    radii from 0 to larger than the room and mixed tmax"""
    b = scenes.cornell()
    v, idx = mesh_of(b)
    rng = np.random.default_rng(71)
    lo, hi = bound_of(v)
    a, bb, c = (v[idx[:, k]] for k in range(3))
    on = np.concatenate([a, bb, c, F(0.5) * (a + bb), (a + bb + c) / F(3)]).astype(F)     # 60: vertices, edge midpoints, centroids
    o = np.concatenate([on, surface_samples(v, idx, 60, rng, 1e-3), uniform_in(lo, hi, 180, rng, 0.9), uniform_in(lo, hi, 100, rng, 3.0)])
    d = directions(len(o), rng)
    aim = rng.random(len(o)) < 0.5      # half of them at a point of the mesh
    d[aim] = towards(o[aim], surface_samples(v, idx, int(aim.sum()), rng, 0.0), rng)
    d[rng.random(len(o)) < 0.03] = 0    # a few balls that do not move
    r = rng.choice([0.0, 0.01, 0.1, 0.4, 1.0, 2.6, 6.0], len(o), p=[0.15, 0.15, 0.2, 0.2, 0.15, 0.1, 0.05]).astype(F)
    tmax = rng.choice([np.inf, 0.0, 0.05, 0.5, 2.0, 50.0], len(o), p=[0.4, 0.05, 0.1, 0.15, 0.15, 0.15]).astype(F)
    return b, v, idx, sr.casts_of(o, d, r, tmax)


def mesh_casts(v, idx, n, rng, radii, tmaxes=(np.inf,)):
    """n casts against a mesh: a third from inside its bound in random directions, a third from twice its bound aimed at the surface,
    a third from near the surface"""
    lo, hi = bound_of(v)
    k = n // 3
    o = np.concatenate([uniform_in(lo, hi, k, rng), uniform_in(lo, hi, k, rng, 2.0), surface_samples(v, idx, n - 2 * k, rng, 0.05)])
    d = directions(n, rng)
    d[k:2 * k] = towards(o[k:2 * k], surface_samples(v, idx, k, rng, 0.0), rng)
    return sr.casts_of(o, d, rng.choice(radii, n).astype(F), rng.choice(tmaxes, n).astype(F))


_dragon_cache = {}


def dragon_case():
    """the 2 k mesh in its Cornell box, 510 casts and the brute force: computed once, shared, never written"""
    if not _dragon_cache:
        v, idx = mesh_of(dragon())
        casts = mesh_casts(v, idx, 510, np.random.default_rng(72), [0.0, 0.01, 0.05, 0.2, 0.7], [np.inf, np.inf, 0.3, 3.0])
        want = sr.sphere_casts(v, idx, casts)
        for x in (v, idx, casts, want):
            x.setflags(write=False)
        _dragon_cache.update(v=v, idx=idx, casts=casts, want=want)
    return _dragon_cache


# ---- the check in float64, independent of the restatement: plain point-triangle distances, nothing of steps 1-3
def _seg_dist(p0, p1, q):
    e = p1 - p0
    ee = (e * e).sum(-1)
    s = np.clip(((q - p0) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    return np.linalg.norm(q - (p0 + s[..., None] * e), axis=-1)


def tri_dist64(a, b, c, q):
    """distance from points q to triangles (a, b, c) in float64: the plane where the foot of the perpendicular is inside, else the edges"""
    a, b, c, q = (np.asarray(x, np.float64) for x in (a, b, c, q))
    ab, ac, ap = b - a, c - a, q - a
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    safe = np.where(nn > 0, nn, 1.0)
    u = (np.cross(ap, ac) * n).sum(-1) / safe     # weight of b
    w = (np.cross(ab, ap) * n).sum(-1) / safe     # weight of c
    inside = (nn > 0) & (u >= 0) & (w >= 0) & (u + w <= 1)
    plane = np.abs((ap * n).sum(-1)) / np.sqrt(safe)
    edges = np.minimum(np.minimum(_seg_dist(a, b, q), _seg_dist(a, c, q)), _seg_dist(b, c, q))
    return np.where(inside, plane, edges)


# The largest residual of the numpy restatement on the inputs of test_geometry (geometry_inputs below), measured on the CPU by
# geometry_residuals and relative to scale: 1.898e-06 (the Cornell case, at a touch; the dragon case 4.83e-08; no sample before an impact
# or along a miss was inside r at all, residual 0).  The tolerance is 4 x the measured value.  The factor covers a different but equally
# valid ordering of ties, not device error: the device matches the restatement on bytes.
RESTATEMENT_RESIDUAL = 1.898e-06
GEOMETRY_TOL = 4 * RESTATEMENT_RESIDUAL


def geometry_residuals(v, idx, casts, rec, samples=64):
    """(touch, early, miss): the largest of | dist(o + t d, winner) - r | / scale over hits with t > 0, of (r - dist(o + s d, mesh)) /
    scale over `samples` evenly spaced s in [0, t) of those hits, and of the same over s in [0, tmax] of misses with a finite tmax;
    all in float64, scale = max(r, extent of the mesh's bound joined with the path)."""
    v64, casts = v.astype(np.float64), casts.astype(np.float64)
    a, b, c = (v64[idx[:, k]] for k in range(3))
    o, r, d, tmax = casts[:, 0:3], casts[:, 3], casts[:, 4:7], casts[:, 7]
    ok = sr.valid_casts(casts.astype(F))
    t = rec["dist2"].astype(np.float64)
    hit = ok & (rec["prim"] >= 0) & (t > 0) & np.isfinite(t)
    miss = ok & (rec["prim"] < 0) & np.isfinite(tmax)
    end = np.where(hit, t, np.where(miss, tmax, 0.0))
    tip = o + end[:, None] * d
    lo = np.minimum(np.minimum(o, tip), v64.min(axis=0))
    hi = np.maximum(np.maximum(o, tip), v64.max(axis=0))
    scale = np.maximum(r, (hi - lo).max(axis=1))
    w = np.where(hit, rec["prim"], 0)
    touch = np.abs(tri_dist64(a[w], b[w], c[w], tip) - r) / scale
    frac = np.arange(samples) / samples      # hits: [0, t), the impact itself excluded
    worst = np.zeros(len(casts))
    for rows, f in ((np.flatnonzero(hit), frac), (np.flatnonzero(miss), np.arange(samples) / (samples - 1))):
        for i in rows:
            pts = o[i] + (f * end[i])[:, None] * d[i]
            dist = tri_dist64(a[None], b[None], c[None], pts[:, None]).min(axis=1)
            worst[i] = ((r[i] - dist) / scale[i]).max()
    return (float(touch[hit].max(initial=0.0)), float(worst[hit].max(initial=0.0)), float(worst[miss].max(initial=0.0)))


def geometry_inputs():
    """the Cornell case and every eighth cast of the dragon case"""
    _, v, idx, casts = cornell_case()
    yield "cornell", v, idx, casts
    case = dragon_case()
    yield "dragon", case["v"], case["idx"], case["casts"][::8]


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_sphere_cast_device", "gnxr_sphere_cast_counted_device", "gnxr_sphere_cast"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.SphereCast) == 32 and C.sizeof(gx._abi.ClosestPoint) == 32 and sr.RECORD.itemsize == 32
    assert [f[0] for f in gx._abi.SphereCast._fields_] == ["o", "radius", "d", "tmax"]
    assert gx.CLOSEST_DTYPE == sr.RECORD
    assert gx._abi.GNXR_ABI_VERSION == 5 and gx._abi.SphereCast not in gx._abi.ABI_STRUCTS
    assert gx.SphereCasts._fields == ("records", "prim", "t", "p", "b1", "b2", "feature")


def one_cast(v, idx, o, d, r, tmax=np.inf):
    return sr.sphere_casts(v, idx, sr.casts_of(np.array([o], F), np.array([d], F), r, tmax))[0]


def test_restatement_exact_cases():
    """Triangle (0,0,0), (4,0,0), (0,4,0) and casts with small integer or power-of-two numbers: every value is exactly representable."""
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F)
    one = np.array([(0, 1, 2)], np.int32)
    rec = lambda r: (int(r["prim"]), float(r["dist2"]), tuple(float(x) for x in r["p"]), float(r["b1"]), float(r["b2"]), int(r["feature"]))
    # head on to the face: the centre stops r = 1 above (1, 1, 0); t is in units of d
    assert rec(one_cast(v, one, (1, 1, 5), (0, 0, -1), 1.0)) == (0, 4.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)
    assert rec(one_cast(v, one, (1, 1, 5), (0, 0, -2), 1.0)) == (0, 2.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)
    assert rec(one_cast(v, one, (1, 1, -5), (0, 0, 0.5), 1.0)) == (0, 8.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)    # from below
    # edge ab: 3 beside it, r = 5, so the contact is 4 above; vertex a: 5 beside it, r = 13, 12 above
    assert rec(one_cast(v, one, (2, -3, 8), (0, 0, -1), 5.0)) == (0, 4.0, (2.0, 0.0, 0.0), 0.5, 0.0, 1)
    assert rec(one_cast(v, one, (-3, -4, 14), (0, 0, -1), 13.0)) == (0, 2.0, (0.0, 0.0, 0.0), 0.0, 0.0, 4)
    # a ray along the centre line of the edge cast misses; so does a ball that is too small
    assert one_cast(v, one, (2, -3, 8), (0, 0, -1), 0.0).tobytes() == EMPTY.tobytes()
    assert one_cast(v, one, (2, -3, 8), (0, 0, -1), 2.5).tobytes() == EMPTY.tobytes()
    # a start in contact: t = 0 and the record is closest_point's at o
    assert rec(one_cast(v, one, (2, -3, 4), (0, 0, -1), 5.0)) == (0, 0.0, (2.0, 0.0, 0.0), 0.5, 0.0, 1)
    assert rec(one_cast(v, one, (1, 1, 0.5), (3, 1, 2), 1.0)) == (0, 0.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)
    # a ball that does not move: t = 0 with overlap, nothing without
    assert rec(one_cast(v, one, (1, 1, 0.5), (0, 0, 0), 1.0)) == (0, 0.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)
    assert one_cast(v, one, (1, 1, 2.5), (0, 0, 0), 1.0).tobytes() == EMPTY.tobytes()
    assert rec(one_cast(v, one, (1, 1, 1), (0, 0, 0), 1.0)) == (0, 0.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)      # touching exactly
    # a static axis exactly on the grown box's face (o.x = hi.x + r, x does not move): the vertex b is touched, and 0 * inf leaks no NaN
    r = one_cast(v, one, (5, 0, 5), (0, 0, -1), 1.0)
    assert rec(r) == (0, 5.0, (4.0, 0.0, 0.0), 1.0, 0.0, 5) and not np.isnan(r["dist2"])
    assert one_cast(v, one, (np.nextafter(F(5), INF), 0, 5), (0, 0, -1), 1.0).tobytes() == EMPTY.tobytes()      # one ulp outside
    assert rec(one_cast(v, one, (5, 0, 5), (1e-45, 0, -1), 1.0))[0:2] == (0, 5.0)    # 1 / denormal overflows: static as well
    # tmax equal to t hits, the next float towards 0 does not
    assert rec(one_cast(v, one, (1, 1, 5), (0, 0, -1), 1.0, 4.0)) == (0, 4.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)
    assert one_cast(v, one, (1, 1, 5), (0, 0, -1), 1.0, np.nextafter(F(4), F(0))).tobytes() == EMPTY.tobytes()
    assert rec(one_cast(v, one, (1, 1, 0.5), (0, 0, -1), 1.0, 0.0))[0:2] == (0, 0.0)     # tmax = 0: contact at the start only
    # a degenerate triangle (three collinear vertices) has no face term and is hit through its edges
    vd = np.array([(0, 0, 0), (2, 0, 0), (4, 0, 0)], F)
    assert rec(one_cast(vd, one, (1, 0, 5), (0, 0, -1), 1.0)) == (0, 4.0, (1.0, 0.0, 0.0), 0.5, 0.0, 1)
    assert rec(one_cast(vd, one, (3, 0, 5), (0, 0, -1), 1.0)) == (0, 4.0, (3.0, 0.0, 0.0), 0.0, 0.75, 2)
    # invalid casts, an infinite origin or direction, no triangles
    for o, d, r, tmax in (((np.nan, 1, 5), (0, 0, -1), 1, np.inf), ((1, 1, 5), (0, np.nan, -1), 1, np.inf), ((1, 1, 5), (0, 0, -1), np.nan, np.inf),
                          ((1, 1, 5), (0, 0, -1), 1, np.nan), ((1, 1, 5), (0, 0, -1), -1, np.inf), ((1, 1, 5), (0, 0, -1), 1, -1),
                          ((1, 1, np.inf), (0, 0, -1), 1, np.inf), ((1, 1, 5), (0, 0, -np.inf), 1, np.inf)):
        assert one_cast(v, one, o, d, r, tmax).tobytes() == EMPTY.tobytes()
    assert rec(one_cast(v, one, (1, 1, 5), (0, 0, -1), np.inf)) == (0, 0.0, (1.0, 1.0, 0.0), 0.25, 0.25, 0)     # r = +inf touches at once
    assert one_cast(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), (1, 1, 5), (0, 0, -1), 1.0).tobytes() == EMPTY.tobytes()
    assert EMPTY["prim"] == -1 and EMPTY["dist2"] == INF and not EMPTY["p"].any() and EMPTY["b1"] == 0 and EMPTY["b2"] == 0 and EMPTY["feature"] == 0
    # the winner is the smallest (t, prim): two copies of the triangle and one nearer
    v2 = np.concatenate([v, v + F((0, 0, 1))])
    assert one_cast(v2, np.array([(0, 1, 2), (1, 2, 0), (3, 4, 5)], np.int32), (1, 1, 5), (0, 0, -1), 1.0)["prim"] == 2
    assert one_cast(v2, np.array([(1, 2, 0), (0, 1, 2)], np.int32), (1, 1, 5), (0, 0, -1), 1.0)["prim"] == 0


def test_restatement_geometry():
    """the restatement passes the float64 check it set the tolerance of (4 x its own largest residual)"""
    for name, v, idx, casts in geometry_inputs():
        res = geometry_residuals(v, idx, casts, sr.sphere_casts(v, idx, casts))
        print(name, "touch %.3e early %.3e miss %.3e" % res)
        assert max(res) <= GEOMETRY_TOL, (name, res)


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0, n < 0 and misaligned pointers are refused before anything is looked at (the handle is a
    dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()   # 256 bytes: room for an aligned base and the offsets below
    p = C.c_void_p(C.addressof(buf))
    for fn in (L.gnxr_sphere_cast_device, lambda s, q, n, o, st: L.gnxr_sphere_cast_counted_device(s, q, n, o, p, st)):
        assert fn(None, p, 1, p, None) == ERR_INVALID
        assert fn(None, p, 0, p, None) == ERR_INVALID
        assert fn(p, None, 4, p, None) == ERR_INVALID
        assert fn(p, p, 4, None, None) == ERR_INVALID
        assert fn(p, p, -1, p, None) == ERR_INVALID
    assert L.gnxr_sphere_cast_counted_device(p, p, 4, p, None, None) == ERR_INVALID
    # misaligned pointers are refused before the handle is looked at; n == 0 returns before that
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    al = lambda k=0: C.c_void_p(base + k)
    assert L.gnxr_sphere_cast_device(p, al(4), 2, al(64), None) == ERR_INVALID and "d_casts is not 16-byte aligned" in L.gnxr_last_error().decode()
    assert L.gnxr_sphere_cast_device(p, al(), 2, al(72), None) == ERR_INVALID and "d_out is not 16-byte aligned" in L.gnxr_last_error().decode()
    assert L.gnxr_sphere_cast_counted_device(p, al(), 2, al(64), al(4), None) == ERR_INVALID and "d_work is not 8-byte aligned" in L.gnxr_last_error().decode()
    assert L.gnxr_sphere_cast_device(p, al(4), 0, al(64), None) == 0
    Q, R = (lambda x: C.cast(x, C.POINTER(gx._abi.SphereCast))), (lambda x: C.cast(x, C.POINTER(gx._abi.ClosestPoint)))
    assert L.gnxr_sphere_cast(None, Q(p), 1, R(p)) == ERR_INVALID
    assert L.gnxr_sphere_cast(p, None, 1, R(p)) == ERR_INVALID
    assert L.gnxr_sphere_cast(p, Q(p), 1, None) == ERR_INVALID
    assert L.gnxr_sphere_cast(p, Q(p), -1, R(p)) == ERR_INVALID


def test_python_refuses_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 3) origins and directions or (n, 8) records on the scene's device pass, radius is a number or an (n,)
    tensor, tmax may also be None, and the launch keywords are `stream` and `counts`; everything else raises before a library call (the
    handle is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    d3 = torch.zeros((4, 3))
    bad = [np.zeros((4, 3), F), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 5)), torch.zeros((3, 4)).t(), torch.zeros((4, 6))[:, ::2],
           torch.zeros(12), "origins", None, torch.zeros((4, 3)), torch.zeros((4, 4))]
    for b in bad:
        with pytest.raises(ValueError):
            s.sphere_cast(b, d3, 1.0)
    for b in (np.zeros((4, 8), F), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((8, 4)).t(), torch.zeros((4, 16))[:, ::2], torch.zeros((4, 8))):
        with pytest.raises(ValueError):
            s.sphere_cast(b, None, None)
    for args in ((d3, 1.0), (None, 1.0), (None, None, 2.0)):
        with pytest.raises(ValueError, match="ready-made"):
            s.sphere_cast(torch.zeros((4, 8)), *args)
    with pytest.raises(ValueError, match="unexpected arguments"):
        s.sphere_cast(torch.zeros((4, 8)), None, None, streams=None)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_python_refusals_on_the_device(gpu):
    """wrong directions, radii and tmax with good origins (these need origins on a device), and the scene still answers afterwards"""
    b, v, idx, casts = cornell_case()
    scene = gpu.Scene(b)
    o, d = torch.from_numpy(casts[:, 0:3].copy()).cuda(), torch.from_numpy(casts[:, 4:7].copy()).cuda()
    for bad in (d.cpu(), d.double(), d[:-1].contiguous(), d.t(), None, casts[:, 4:7]):
        with pytest.raises(ValueError):
            scene.sphere_cast(o, bad, 1.0)
    for r, tmax in ((torch.zeros(5, device="cuda"), None), (1.0, torch.zeros(5, device="cuda")), (torch.zeros(len(o)), None),
                    (torch.zeros(len(o), dtype=torch.float64, device="cuda"), None)):
        with pytest.raises(ValueError):
            scene.sphere_cast(o, d, r, tmax)
    for r, tmax in ((None, None), ("big", None), (True, None), (1.0, "far"), (1.0, False)):
        with pytest.raises(TypeError):
            scene.sphere_cast(o, d, r, tmax)
    c = torch.from_numpy(casts).cuda()
    with pytest.raises(ValueError):
        scene.sphere_cast(c, None, None, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        scene.sphere_cast(c, None, None, out=torch.zeros((len(c) + 1, 8), device="cuda"))
    # the C call: misaligned pointers, host memory, arrays past their allocation
    L = gpu.lib()
    out = torch.zeros((len(c), 8), device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.gnxr_last_error().decode()
    cast = lambda *a: L.gnxr_sphere_cast_device(scene._h, *a)
    assert cast(P(c, 4), 100, P(out), None) == ERR_INVALID and "d_casts is not 16-byte aligned" in err()
    assert cast(P(c), 100, P(out, 8), None) == ERR_INVALID and "d_out is not 16-byte aligned" in err()
    assert cast(P(c), -1, P(out), None) == ERR_INVALID
    host = np.zeros((100, 8), F)
    assert cast(C.c_void_p(host.ctypes.data), 100, P(out), None) == ERR_INVALID and "d_casts is not device memory" in err()
    assert cast(P(c), 100, C.c_void_p(host.ctypes.data), None) == ERR_INVALID and "d_out is not device memory" in err()
    assert cast(P(c), 1 << 20, P(out), None) == ERR_INVALID and "d_casts" in err()
    many = torch.zeros((1 << 20, 8), device="cuda")
    assert cast(P(many), 1 << 20, P(out), None) == ERR_INVALID and "d_out" in err()
    work = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.gnxr_sphere_cast_counted_device(scene._h, P(c), 100, P(out), P(work, 4), None) == ERR_INVALID and "d_work" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (work == 0).all()   # nothing was queued by the refused calls
    check(scene, v, idx, casts)


@pytest.mark.gpu
def test_cornell(gpu):
    b, v, idx, casts = cornell_case()
    assert len(casts) == 400
    want = sr.sphere_casts(v, idx, casts)
    hit = want["prim"] >= 0
    assert (hit & (want["dist2"] > 0)).mean() >= 0.25 and (~hit).mean() >= 0.10 and (hit & (want["dist2"] == 0)).mean() >= 0.05
    assert (casts[:, 3] > 5).any() and (casts[:, 3] == 0).any()
    scene = gpu.Scene(b)
    check(scene, v, idx, casts, want)
    # (n, 3) origins and directions with radius and tmax as tensors, as numbers and tmax as None
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    o, r, d, tmax = dev(casts[:, 0:3]), dev(casts[:, 3]), dev(casts[:, 4:7]), dev(casts[:, 7])
    res = scene.sphere_cast(o, d, r, tmax)
    numbers = scene.sphere_cast(o, d, 0.25, 1.5)
    free = scene.sphere_cast(o, d, r)
    mixed = scene.sphere_cast(o, d, 1, tmax=tmax)
    torch.cuda.synchronize()
    as_rec = lambda x: x.records.cpu().numpy().view(sr.RECORD).reshape(-1)
    assert_same(as_rec(res), want, "tensors")
    assert_same(as_rec(numbers), sr.sphere_casts(v, idx, sr.casts_of(casts[:, 0:3], casts[:, 4:7], 0.25, 1.5)), "numbers")
    assert_same(as_rec(free), sr.sphere_casts(v, idx, sr.casts_of(casts[:, 0:3], casts[:, 4:7], casts[:, 3])), "tmax None")
    assert_same(as_rec(mixed), sr.sphere_casts(v, idx, sr.casts_of(casts[:, 0:3], casts[:, 4:7], 1.0, casts[:, 7])), "mixed")
    # the named views are the records' fields
    for name, field in (("prim", "prim"), ("t", "dist2"), ("p", "p"), ("b1", "b1"), ("b2", "b2"), ("feature", "feature")):
        assert_same(getattr(res, name).cpu().numpy(), want[field], name)
    # the host-array form
    assert_same(scene.SphereCast(casts).view(sr.RECORD), want, "SphereCast")


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts"])
def test_split_methods(gpu, split):
    """the records do not depend on the tree: every split method gives the brute force's bytes"""
    case = dragon_case()
    hit = case["want"]["prim"] >= 0
    assert hit.mean() > 0.5 and (~hit).mean() > 0.05 and len(set(case["want"]["feature"][hit])) >= 6   # faces, edges and vertices are all contacts somewhere
    check(gpu.Scene(dragon(split)), case["v"], case["idx"], case["casts"], case["want"], split)


@pytest.mark.gpu
def test_off_the_wide_tree_and_large_leaves(gpu):
    rng = np.random.default_rng(73)
    v, idx = concentric_mesh(rng)
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    _, meta, _ = scene.bvh()
    assert meta[:, 1].max() > 127   # a leaf the 4-wide encoding cannot hold: the scene is on the binary walk
    check(scene, v, idx, mesh_casts(v, idx, 384, rng, [0.0, 0.05, 0.5, 2.0], [np.inf, 1.0]), what="concentric")
    # slivers: boxes that say little, leaves of many triangles
    v, idx = sliver_mesh(rng)
    check(gpu.Scene(mesh_scene(gpu, v, idx)), v, idx, mesh_casts(v, idx, 384, rng, [0.0, 0.05, 0.5, 2.0], [np.inf, 1.0]), what="slivers")
    # a scene kept on the binary tree by the creation switch
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        binary = gpu.Scene(dragon())
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    case = dragon_case()
    check(binary, case["v"], case["idx"], case["casts"], case["want"], "binary")


FAN_H = 2.5   # the ball of radius 1 starts FAN_H above the apex and moves down the axis: it touches the apex at t = 1.5


@pytest.mark.gpu
@pytest.mark.parametrize("copies,others", [(1, 0), (2, 0), (1, 3000)])
def test_ties(gpu, copies, others):
    """The ball moves down the axis onto fan_mesh's apex: all 12 (24 with coincident copies) triangles are hit through the vertex at one
    bit-equal t, and the smallest authoring index must win -- also with the group spread over the leaves of a tree of 3000 other
    triangles, where entering a box with tb == best is what decides."""
    v, idx, fan = fan_mesh(np.random.default_rng(80 + copies + others), copies, others)
    casts = sr.casts_of(np.array([(0, 0, FAN_H)] * 3, F), np.array([(0, 0, -1), (0, 0, -0.5), (0, 0, -1)], F), [1.0, 1.0, 1.0], [np.inf, np.inf, 1.5])
    hits, t = sr.hit_times(v, idx, casts)
    assert len(fan) == 12 * copies and hits[:, fan].all()
    assert (t[0, fan].view(np.uint32) == F(1.5).view(np.uint32)).all() and (t[1, fan] == F(3)).all()
    want = sr.sphere_casts(v, idx, casts)
    assert (want["prim"] == fan[0]).all() and fan[0] == fan.min() and list(want["dist2"]) == [1.5, 3.0, 1.5] and (want["p"] == 0).all()
    assert_same(device_casts(gpu.Scene(mesh_scene(gpu, v, idx)), casts), want)


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
def test_deep_tree_spills(gpu, binary):
    """chain_scene(36): casts from beyond the smallest triangle walk the whole chain with a sibling on the stack per level.  With the default
    LDS levels on the 4-wide tree, where the tree's need exceeds them, and forced onto 2 LDS levels through GNXR_SPHERECAST_LDS_LEVELS
    on the 4-wide and on the binary tree: the LDS levels and the global spill together."""
    b = chain_scene(gpu)
    v, idx = mesh_of(b)
    rng = np.random.default_rng(74)
    n = 768
    o = np.stack([-(2.0 ** -rng.uniform(20, 36, n)), rng.normal(0, 2.0 ** -37, n), rng.normal(0, 2.0 ** -37, n)], axis=1).astype(F)
    d = np.stack([np.ones(n), rng.normal(0, 0.01, n), rng.normal(0, 0.01, n)], axis=1).astype(F)     # along the chain, towards the large end
    casts = np.concatenate([sr.casts_of(o, d, rng.choice([0.0, 2.0 ** -36, 2.0 ** -20], n).astype(F), rng.choice([np.inf, 2.0 ** -10, 0.5], n).astype(F)),
                            mesh_casts(v, idx, 256, rng, [0.0, 0.01, 0.3], [np.inf, 1.0])])
    want = sr.sphere_casts(v, idx, casts)
    assert (want["prim"][:n] >= 0).mean() > 0.5 and len(set(want["prim"][:n])) > 12
    if binary:
        os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(b)
    finally:
        os.environ.pop("GNXR_BINARY_BVH", None)
    if not binary:
        assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
        check(scene, v, idx, casts, want, "default levels")
    os.environ["GNXR_SPHERECAST_LDS_LEVELS"] = "2"
    try:
        check(scene, v, idx, casts, want, "2 LDS levels")
    finally:
        del os.environ["GNXR_SPHERECAST_LDS_LEVELS"]


@pytest.mark.gpu
def test_live_scene(gpu):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    SkinnedMesh.pose -> the brute force over the vertices it holds; set_geometry with another triangle count -> over the new mesh"""
    case = dragon_case()
    b = dragon()
    v, idx = mesh_of(b)
    casts = case["casts"][::2]
    scene = gpu.Scene(b)
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(0.15) * np.sin(F(5) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    scene.update_vertices(torch.from_numpy(v2[:n_mesh_v].copy()).cuda())
    want2 = sr.sphere_casts(v2, idx, casts)
    assert want2.tobytes() != case["want"][::2].tobytes()
    check(scene, v2, idx, casts, want2, "update_vertices")
    scene.rebuild_bvh()
    check(scene, v2, idx, casts, want2, "rebuild_bvh")
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
    check(scene, v3, idx, casts, what="pose")
    rng = np.random.default_rng(75)
    v4 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v4[1::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    v4[2::3] = v4[0::3] + rng.uniform(-0.2, 0.2, (300, 3)).astype(F)
    idx4 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    scene.set_geometry(v4, idx4, np.zeros(300, np.int32), tri_light=tri_light)
    check(scene, v4, idx4, casts, what="set_geometry")


@pytest.mark.gpu
def test_tmax_on_the_ulp_and_pruning(gpu):
    """Every hit again with tmax = t: the same bytes; with tmax = the next float towards 0: nothing hits before t, so the record is empty.
    With counts=, the run bounded by tmax = t visits no more nodes than the unbounded one: its bound starts where the other's ends and
    the order of visits depends on the boxes alone."""
    case = dragon_case()
    want = case["want"]
    hit = want["prim"] >= 0
    casts = case["casts"][hit].copy()
    t = want["dist2"][hit]
    scene = gpu.Scene(dragon())
    at = casts.copy()
    at[:, 7] = t
    assert_same(device_casts(scene, at), want[hit], "tmax = t")
    assert_same(sr.sphere_casts(case["v"], case["idx"], at), want[hit], "tmax = t, restatement")
    moved = t > 0
    below = casts[moved].copy()
    below[:, 7] = np.nextafter(t[moved], F(0))
    assert moved.sum() > 100
    assert_same(device_casts(scene, below), sr.empty_records(int(moved.sum())), "tmax = nextafter(t, 0)")
    free = casts.copy()
    free[:, 7] = np.inf
    work_free, work_at = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    a = device_casts(scene, free, counts=work_free)
    b = device_casts(scene, at, counts=work_at)
    assert_same(a["prim"], b["prim"])    # the unbounded cast finds the same first impact
    nodes_free, tris_free = (int(x) for x in work_free.cpu())
    nodes_at, tris_at = (int(x) for x in work_at.cpu())
    assert len(casts) <= nodes_at <= nodes_free, (nodes_at, nodes_free)
    assert 0 < tris_at <= tris_free, (tris_at, tris_free)
    # the counting form's records are the timed form's
    assert_same(b, want[hit], "counting form")


@pytest.mark.gpu
def test_degenerate_input(gpu):
    rng = np.random.default_rng(76)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    idx = np.arange(60, dtype=np.int32).reshape(-1, 3)
    v[3:6] = [(0, 0, 0), (0.5, 0.5, 0.5), (1, 1, 1)]          # zero area: three collinear vertices
    v[10] = v[9]                                               # two coincident vertices
    v[12:15] = v[12]                                           # zero area: one point
    casts = mesh_casts(v, idx, 768, rng, [0.0, 0.0, 0.01, 0.1, 0.5, 3.0, 1e30, 3e38, np.inf], [np.inf, 0.0, 1.0, 3e38])
    n = len(casts)
    casts[0:8, 0] = np.nan; casts[8:12, 5] = np.nan; casts[12:16, 3] = np.nan; casts[16:20, 7] = np.nan            # NaN in o, d, radius, tmax
    casts[20:28, 3] = [-1, -0.0, -np.inf, -1e-45] * 2; casts[28:36, 7] = [-1, -0.0, -np.inf, -1e-45] * 2              # negative fields (and -0)
    casts[36:44, 0] = np.inf; casts[44:52, 6] = -np.inf                                                               # infinite o, d
    casts[52:84, 4] = 0; casts[84:100, 4:6] = 0; casts[100:116, 4:7] = 0                                              # zero components, zero d
    casts[116:148, 5] = rng.choice([1e-45, -1e-45, 1e-39, -3e-39], 32)                                                # denormal components: 1 / d overflows or not
    casts[148:164, 4:7] *= F(1e-38)                                                                                   # a denormal direction
    casts[164:180, 4:7] *= F(1e30)
    # along the collinear triangle and onto the point triangle
    line = np.linspace((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 32).astype(F)
    extra = sr.casts_of(line + F((0.3, -0.3, 0)), np.tile(F((-0.3, 0.3, 0)), (32, 1)), rng.choice([0.0, 0.05], 32), 2.0)
    extra2 = sr.casts_of(v[12] + rng.normal(0, 1, (32, 3)).astype(F), np.zeros((32, 3), F), 0.02)
    extra2[:, 4:7] = v[12] - extra2[:, 0:3]
    casts = np.concatenate([casts, extra, extra2])
    want = sr.sphere_casts(v, idx, casts)
    assert (want["prim"][:20] == -1).all() and (want["prim"][36:52] == -1).all()
    assert (want["prim"][[20, 22, 23, 24, 26, 27, 28, 30, 31, 32, 34, 35]] == -1).all()      # -0 is not negative
    assert (want["prim"][n:] == 1).any() and (want["prim"][n + 32:] == 4).any()     # the two degenerate triangles are hit
    assert (want["prim"] >= 0).mean() > 0.4
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    assert_same(device_casts(scene, casts), want)
    # Every scene has a triangle: scene creation refuses a description without one (the restatement's answer without triangles, prim -1
    # and t +inf, is asserted in test_restatement_exact_cases; the library has no such path) ...
    b = gpu.SceneBuilder()
    b.AddSphere((0, 0, 0), 1.0, b.MatteMaterial(scenes.WHITE, 60.0))
    b.AddSkyLight()
    with pytest.raises(gpu.GnxrError, match="no geometry"):
        gpu.Scene(b)
    # ... and a sphere beside triangles is not considered: casts at and from inside the sphere of cornell_sphere get the walls' answer
    b = scenes.cornell_sphere("matte", center=(0.6, -1.5, 0.2), radius=1.0)
    v, idx = mesh_of(b)
    ball = gpu.Scene(b)
    assert ball.n_triangles == len(idx)
    o = (np.array((0.6, -1.5, 0.2)) + rng.normal(0, 1, (128, 3)) * rng.choice([0.0, 0.5, 3.0], (128, 1))).astype(F)
    aim = sr.casts_of(o, towards(o, np.tile(np.array((0.6, -1.5, 0.2)), (128, 1)) + 1e-3, rng), rng.choice([0.0, 0.2], 128))
    check(ball, v, idx, aim, what="sphere primitive")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_batch_sizes_out_and_stream(gpu, n):
    case = dragon_case()
    scene = gpu.Scene(dragon())
    want = case["want"][:n]
    c = torch.from_numpy(case["casts"][:n].copy()).cuda()
    out = torch.full((n, 8), 7.0, device="cuda")
    res = scene.sphere_cast(c, None, None, out=out)
    torch.cuda.synchronize()
    assert res.records is out and out.shape == (n, 8)
    assert_same(out.cpu().numpy().view(sr.RECORD).reshape(n), want)
    again = scene.sphere_cast(c, None, None, out=out)      # the same rows a second time
    torch.cuda.synchronize()
    assert again.records is out
    assert_same(out.cpu().numpy().view(sr.RECORD).reshape(n), want)
    assert_same(scene.SphereCast(case["casts"][:n]).view(sr.RECORD), want)
    # casts written by torch on a side stream, answered there and reduced there with no synchronise in between
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q = c * 1.0
        r = scene.sphere_cast(q, None, None, stream=side)
        total = r.prim.to(torch.int64).sum()
    side.synchronize()
    assert int(total) == int(want["prim"].astype(np.int64).sum())
    assert_same(r.records.cpu().numpy().view(sr.RECORD).reshape(n), want)


@pytest.mark.gpu
def test_geometry(gpu):
    """In float64 and without the restatement: at a hit with t > 0 the centre is r from the winning triangle, at 64 evenly spaced earlier
    times it is at least r from the whole mesh, and a miss with a finite tmax stays r away at 64 times in [0, tmax] -- each to within
    GEOMETRY_TOL x scale."""
    for (name, v, idx, casts), b in zip(geometry_inputs(), (scenes.cornell(), dragon())):
        rec = device_casts(gpu.Scene(b), casts)
        res = geometry_residuals(v, idx, casts, rec)
        print(name, "touch %.3e early %.3e miss %.3e" % res)
        assert (rec["prim"] >= 0).sum() > 50
        assert max(res) <= GEOMETRY_TOL, (name, res)


def test_no_scratch(gx):
    """tools/kernel_regs.py: every instantiation of k_sphere_cast (wide / binary; timed / counting) runs without scratch and without
    spilled VGPRs"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels(gx.LIB_PATH) if "k_sphere_cast<" in k["name"]]
    assert len(ks) == 4, [k["name"] for k in ks]
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in ks), ks
