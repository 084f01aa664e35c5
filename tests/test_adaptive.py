"""Adaptive sampling: gnxr_render_adaptive_device / integrator.RenderAdaptive against tests/adaptive_reference.py.

The per-sample truth never comes from the code under test.  For a power-of-two budget B it is the oracle's
render(spp=B, spp_begin=s, spp_end=s+1) * B (the box average divides by a power of two, so the product is the sample's Li exactly);
for the budget that is no power of two it is the existing integrator.Li on camera_rays_device rays, which tests/test_li_device.py pins.
Every GPU comparison is exact: image bits, count map and rounds equal the model's, no tolerance, no pixel left out.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from adaptive_reference import adaptive_image, adaptive_reference, criterion, guard_window
from conftest import ROOT

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W0, H0, B0 = 32, 24, 32
DEFAULTS = dict(min_spp=4, step_spp=4, floor=0.01)


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def integrator(gx, kind):
    return {"path": lambda: gx.PathIntegrator(5, 1.0, "spatial"), "volpath": lambda: gx.VolPathIntegrator(5, 1.0, "spatial"),
            "whitted": lambda: gx.WhittedIntegrator(5), "direct": lambda: gx.DirectLightingIntegrator("all", 5)}[kind]()


def builder(scene_name):
    return {"cornell": scenes.cornell, "volume": scenes.volume_cornell, "zoo": scenes.material_zoo}[scene_name]()


@functools.lru_cache(maxsize=None)
def oracle_samples(scene_name, kind, W, H, B):
    """L[s, y, x, 3] of the oracle for a power-of-two budget B; computed once per case and shared (read-only)"""
    import gnxraytracer_amd as gx
    assert B & (B - 1) == 0
    osc = ol.OracleScene(builder(scene_name))
    integ = integrator(gx, kind)
    L = np.stack([osc.render(integ, W, H, B, spp_begin=s, spp_end=s + 1)[0][..., :3] * np.float32(B) for s in range(B)])
    L.setflags(write=False)
    return L


def histogram(n):
    v, c = np.unique(n, return_counts=True)
    return dict(zip(v.tolist(), c.tolist()))


def run(integ, scene, W, H, B, threshold, guard, **kw):
    args = dict(DEFAULTS)
    args.update(kw)
    img, cnt, st = integ.RenderAdaptive(scene, W, H, B, threshold, guard=guard, **args)
    torch.cuda.synchronize()
    return img.cpu().numpy(), cnt.cpu().numpy(), st


def check_model(img, cnt, st, L, B, threshold, guard, **kw):
    args = dict(DEFAULTS)
    args.update({k: v for k, v in kw.items() if k in DEFAULTS})
    S, n, rounds = adaptive_reference(L, B, args["min_spp"], args["step_spp"], threshold, args["floor"], guard)
    print("model:", histogram(n), "samples", int(n.sum()), "rounds", rounds, "| device: samples", st["samples"], "rounds", st["rounds"])
    assert (cnt == n).all(), (histogram(cnt), histogram(n))
    assert st["rounds"] == rounds
    assert biteq(img, adaptive_image(S, n)) and img[..., :3].any()
    assert st["samples"] == int(n.sum()) == st["camera_samples"] and st["pixels_at_budget"] == int((n == B).sum())
    return S, n, rounds


# ---------------------------------------------------------------- CPU
def test_adaptive_entry_point_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    assert re.search(r"\bgnxr_render_adaptive_device\s*\(", hdr)
    assert hasattr(gx.lib(), "gnxr_render_adaptive_device") and "gnxr_render_adaptive_device" in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.AdaptiveParams) == 24 and C.sizeof(gx._abi.AdaptiveInfo) == 24
    for cls in (gx.PathIntegrator, gx.VolPathIntegrator, gx.WhittedIntegrator, gx.DirectLightingIntegrator):
        assert cls.RenderAdaptive is gx.PathIntegrator.RenderAdaptive


def test_reference_with_full_budget_reproduces_the_oracle_render(gx):
    """min_spp == spp: the model's image is the oracle's render, bit for bit, in one round"""
    L = oracle_samples("cornell", "path", W0, H0, B0)
    full, _ = ol.OracleScene(builder("cornell")).render(integrator(gx, "path"), W0, H0, B0)
    S, n, rounds = adaptive_reference(L, B0, B0, 4, 0.1, 0.01, 1)
    assert rounds == 1 and (n == B0).all()
    assert biteq(adaptive_image(S, n)[..., :3], full[..., :3]) and full[..., :3].any()


def test_reference_huge_threshold_stops_at_min_spp(gx):
    L = oracle_samples("cornell", "path", W0, H0, B0)
    S, n, rounds = adaptive_reference(L, B0, 4, 4, 1e9, 0.01, 1)
    assert rounds == 1 and (n == 4).all()
    acc = np.zeros((H0, W0, 3), np.float32)
    for s in range(4):
        acc += L[s]
    assert biteq(S, acc)


def test_reference_spread_of_counts_on_the_oracle(gx):
    """the two configurations of the GPU spread test are not degenerate: all eight counts occur; threshold 0 still stops e == 0"""
    L = oracle_samples("cornell", "path", W0, H0, B0)
    want = {(0.1, 0): {4: 347, 8: 116, 12: 66, 16: 48, 20: 28, 24: 18, 28: 18, 32: 127},     # 9 436 of 24 576 samples
            (0.2, 1): {4: 194, 8: 74, 12: 88, 16: 33, 20: 37, 24: 49, 28: 36, 32: 257}}     # 14 100
    for (threshold, guard), hist in want.items():
        _, n, rounds = adaptive_reference(L, B0, 4, 4, threshold, 0.01, guard)
        assert histogram(n) == hist and rounds == 8, histogram(n)
    _, n0, _ = adaptive_reference(L, B0, 4, 4, 0.0, 0.01, 0)
    assert histogram(n0) == {4: 192, 32: 576}


def test_reference_guard_clips_at_the_border():
    noisy = np.zeros((5, 7), bool)
    noisy[0, 0] = noisy[4, 6] = noisy[2, 3] = True
    g0 = guard_window(noisy, 0)
    assert (g0 == noisy).all()
    g1 = guard_window(noisy, 1)
    want = np.zeros((5, 7), bool)
    want[0:2, 0:2] = True          # the corner's window holds 4 pixels, not 9
    want[3:5, 5:7] = True
    want[1:4, 2:5] = True
    assert (g1 == want).all() and g1.sum() == 4 + 4 + 9
    g8 = guard_window(noisy[:, :1] | False, 8)
    assert g8.shape == (5, 1) and g8.all()      # a window wider than the image is the image
    # NaN sums keep a pixel sampling; e == 0 stops it even at threshold 0
    S = np.array([[[1, 1, 1], [np.nan, 0, 0], [2, 2, 2]]], np.float32)
    A = np.array([[[.5, .5, .5], [0, 0, 0], [0, 0, 0]]], np.float32)
    assert criterion(S, A, np.full((1, 3), 4), 0.0, 0.0).tolist() == [[False, True, True]]
    # a stopped pixel never restarts: one noisy pixel with guard 1 keeps only pixels that are still active
    L = np.zeros((8, 1, 3, 3), np.float32)
    L[1::2, 0, 1] = 1.0            # pixel 1: odd samples only -> S = 2 A never holds
    _, n, rounds = adaptive_reference(L, 8, 2, 2, 0.5, 0.0, 1)
    assert n.tolist() == [[8, 8, 8]] and rounds == 4
    _, n, _ = adaptive_reference(L, 8, 2, 2, 0.5, 0.0, 0)
    assert n.tolist() == [[2, 8, 2]]


def test_python_argument_checks_raise_before_the_library(gx, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(gx, "lib", no_lib)
    integ = gx.PathIntegrator(5)
    ok = dict(width=8, height=8, spp=8, threshold=0.1, min_spp=2, step_spp=2, floor=0.01, guard=1)
    for bad in (dict(width=0), dict(height=-1), dict(spp=0), dict(min_spp=0), dict(min_spp=9), dict(step_spp=0), dict(guard=-1), dict(guard=9),
                dict(threshold=-0.1), dict(threshold=float("nan")), dict(floor=-1.0), dict(floor=float("nan")), dict(spp_begin=1), dict(shard_count=2)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match="RenderAdaptive"):
            integ.RenderAdaptive(None, **kw)


def test_adaptive_rejects_null_pointers_before_any_device_work(gx):
    """a null scene is refused before a device is needed (this machine may have none), whatever else is passed; the other refusals need a
    real handle and are exercised on the GPU (test_refusals_leave_outputs_and_handle_untouched)"""
    fn = gx.lib().gnxr_render_adaptive_device
    p = gx.PathIntegrator(5).params(8, 8, 8)
    A, I = gx._abi.AdaptiveParams, gx._abi.AdaptiveInfo
    ap, info, st = A(C.sizeof(A), 2, 2, 1, 0.1, 0.01), I(C.sizeof(I), 0, 0, 0), gx.Stats()
    buf = (C.c_float * 1024)()
    out = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert fn(None, C.byref(p), C.byref(ap), out, None, None, C.byref(st), C.byref(info)) == ERR_INVALID
    assert fn(None, None, None, None, None, None, None, None) == ERR_INVALID
    assert not any(buf)


def test_reference_steps_grow_with_n():
    """the schedule: min_spp, then max(step_spp, n // 8), cut at the budget.  Budget 64 in steps of 4: fixed steps up to n = 40, then 5, 5, 6,
    7 and the last sample"""
    L = np.zeros((64, 1, 2, 3), np.float32)
    L[1::2, 0, 0] = 1.0            # pixel 0 never agrees with itself, pixel 1 stops at once
    _, n, rounds = adaptive_reference(L, 64, 4, 4, 0.5, 0.0, 0)
    assert n.tolist() == [[64, 4]] and rounds == 10 + 5          # 4 .. 40 in tens rounds, then 45, 50, 56, 63, 64
    seen = []
    for B in (45, 50, 56, 63, 64):
        _, nb, _ = adaptive_reference(L[:B], B, 4, 4, 0.5, 0.0, 0)
        seen.append(int(nb[0, 0]))
    assert seen == [45, 50, 56, 63, 64]
    _, n, rounds = adaptive_reference(L, 64, 16, 16, 0.5, 0.0, 0)
    assert n.tolist() == [[64, 16]] and rounds == 4             # n // 8 <= 8 < 16 up to the budget: fixed steps


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("threshold,guard", [(0.1, 0), (0.2, 1)])
def test_spread_of_counts_and_ray_counters(gpu, threshold, guard):
    """1. + 7.: all eight counts 4 .. 32 occur in the model; image, counts and rounds equal it; the ray counters are those of one
    integrator.Li call over exactly the model's (px, py, s) set"""
    L = oracle_samples("cornell", "path", W0, H0, B0)
    _, n_model, _ = adaptive_reference(L, B0, 4, 4, threshold, 0.01, guard)
    assert sorted(histogram(n_model)) == list(range(4, 33, 4)), histogram(n_model)
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    img, cnt, st = run(integ, scene, W0, H0, B0, threshold, guard)
    _, n, _ = check_model(img, cnt, st, L, B0, threshold, guard)
    py, px = np.nonzero(n > 0)
    reps = n[py, px]
    px, py, s = np.repeat(px, reps), np.repeat(py, reps), np.concatenate([np.arange(k) for k in reps])
    assert len(s) == int(n.sum())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rays, samples = gpu.camera_rays_device(gpu.camera(), W0, H0, dev(px), dev(py), dev(s))
    _, lst = integ.Li(scene, rays, samples, W0, H0, B0)
    for k in ("rays_closest", "rays_any", "rays_closest_nee"):
        assert st[k] == lst[k], (k, st[k], lst[k])
    scene.close()


@pytest.mark.gpu
def test_threshold_zero_stops_exact_pixels(gpu):
    """threshold = 0 still stops the pixels whose e is exactly 0 (the void, the light seen directly): that is the definition"""
    L = oracle_samples("cornell", "path", W0, H0, B0)
    scene = gpu.Scene(builder("cornell"))
    img, cnt, st = run(integrator(gpu, "path"), scene, W0, H0, B0, 0.0, 0)
    _, n, _ = check_model(img, cnt, st, L, B0, 0.0, 0)
    assert set(histogram(n)) == {4, 32}
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scene_name,threshold,guard", [("volpath", "volume", 0.1, 0), ("whitted", "cornell", 0.1, 0), ("direct", "cornell", 0.2, 1),
                                                              ("path", "zoo", 0.2, 1)])
def test_other_integrators_and_scenes(gpu, kind, scene_name, threshold, guard):
    """2. the other integrators and the material zoo at the same size and parameters; at least three distinct counts in the model"""
    L = oracle_samples(scene_name, kind, W0, H0, B0)
    _, n_model, _ = adaptive_reference(L, B0, 4, 4, threshold, 0.01, guard)
    assert len(histogram(n_model)) >= 3, histogram(n_model)
    scene = gpu.Scene(builder(scene_name))
    img, cnt, st = run(integrator(gpu, kind), scene, W0, H0, B0, threshold, guard)
    check_model(img, cnt, st, L, B0, threshold, guard)
    scene.close()


@pytest.mark.gpu
def test_equality_with_render(gpu):
    """3. min_spp == spp: image and ray counters are RenderDevice's bit for bit, count == spp, one round; threshold 1e9: count == min_spp
    and the image is S / min_spp of the model"""
    L = oracle_samples("cornell", "path", W0, H0, B0)
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    ref = torch.zeros((H0, W0, 4), device="cuda")
    rst = integ.RenderDevice(scene, ref.data_ptr(), W0, H0, B0)
    torch.cuda.synchronize()
    img, cnt, st = run(integ, scene, W0, H0, B0, 0.1, 1, min_spp=B0)
    assert biteq(img, ref.cpu().numpy()) and img[..., :3].any()
    assert (cnt == B0).all() and st["rounds"] == 1 and st["pixels_at_budget"] == W0 * H0
    for k in ("rays_closest", "rays_any", "rays_closest_nee", "camera_samples"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    check_model(img, cnt, st, L, B0, 0.1, 1, min_spp=B0)
    img, cnt, st = run(integ, scene, W0, H0, B0, 1e9, 1)
    assert (cnt == 4).all() and st["rounds"] == 1 and st["pixels_at_budget"] == 0
    check_model(img, cnt, st, L, B0, 1e9, 1)
    scene.close()


def li_samples_of(gpu, integ, scene, W, H, B):
    """L[s, y, x, 3] from integrator.Li on camera_rays_device rays (a budget that is no power of two)"""
    s, py, px = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij"))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rays, samples = gpu.camera_rays_device(gpu.camera(), W, H, dev(px), dev(py), dev(s))
    L, _ = integ.Li(scene, rays, samples, W, H, B)
    torch.cuda.synchronize()
    return L.cpu().numpy().reshape(B, H, W, 4)[..., :3].copy()


@pytest.mark.gpu
def test_truncated_last_round(gpu):
    """4. budget 30, min_spp 4, step_spp 8: counts in {4, 12, 20, 28, 30}, all five present in the model; L from integrator.Li"""
    B = 30
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    L = li_samples_of(gpu, integ, scene, W0, H0, B)
    img, cnt, st = run(integ, scene, W0, H0, B, 0.1, 0, step_spp=8)
    _, n, _ = check_model(img, cnt, st, L, B, 0.1, 0, step_spp=8)
    assert sorted(histogram(n)) == [4, 12, 20, 28, 30], histogram(n)
    scene.close()


@pytest.mark.gpu
def test_growing_steps(gpu):
    """budget 64 in steps of 4: beyond n = 40 the step is n // 8 (5, 5, 6, 7) and the last round is cut to one sample"""
    B = 64
    L = oracle_samples("cornell", "path", W0, H0, B)
    scene = gpu.Scene(builder("cornell"))
    img, cnt, st = run(integrator(gpu, "path"), scene, W0, H0, B, 0.1, 0)
    _, n, rounds = check_model(img, cnt, st, L, B, 0.1, 0)
    assert rounds == 15 and sorted(histogram(n)) == list(range(4, 41, 4)) + [45, 50, 56, 63, 64], histogram(n)
    scene.close()


@pytest.mark.gpu
def test_beyond_one_compaction_tile_and_across_sub_passes(gpu):
    """5. 160 x 120 = 19 200 pixels against kCompactTile = 16 384, budget 8 in steps of 2: once with default sub-passes, once with rounds cut
    into chunks of 5000 paths, four in flight -- the sums must still be added in sample order"""
    W, H, B = 160, 120, 8
    L = oracle_samples("cornell", "path", W, H, B)
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    kw = dict(min_spp=2, step_spp=2)
    img, cnt, st = run(integ, scene, W, H, B, 0.2, 1, **kw)
    _, n, _ = check_model(img, cnt, st, L, B, 0.2, 1, **kw)
    assert sorted(histogram(n)) == [2, 4, 6, 8], histogram(n)
    img2, cnt2, st2 = run(integ, scene, W, H, B, 0.2, 1, samples_per_pass=5000, passes_in_flight=4, **kw)
    check_model(img2, cnt2, st2, L, B, 0.2, 1, **kw)
    assert st2["passes"] > st["passes"] and st2["passes_in_flight"] == 4
    for k in ("rays_closest", "rays_any"):
        assert st[k] == st2[k]
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scene_name", [("volpath", "volume"), ("whitted", "cornell")])
def test_one_pass_integrators_across_chunks(gpu, kind, scene_name):
    """VolPath / Whitted render a round one chunk after the other (and VolPath packs its survivors inside a chunk): rounds cut into chunks
    of 1000 paths -- no multiple of the 768 pixels -- must still give the model's bits"""
    L = oracle_samples(scene_name, kind, W0, H0, B0)
    scene = gpu.Scene(builder(scene_name))
    img, cnt, st = run(integrator(gpu, kind), scene, W0, H0, B0, 0.1, 0, samples_per_pass=1000)
    check_model(img, cnt, st, L, B0, 0.1, 0)
    assert st["passes"] > st["rounds"]
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(37, 5), (1, 1)])
def test_odd_and_tiny_images(gpu, W, H):
    """6. a width that is no multiple of 64, and a single pixel, at budget 8"""
    B = 8
    L = oracle_samples("cornell", "path", W, H, B)
    scene = gpu.Scene(builder("cornell"))
    kw = dict(min_spp=2, step_spp=2)
    img, cnt, st = run(integrator(gpu, "path"), scene, W, H, B, 0.2, 1, **kw)
    check_model(img, cnt, st, L, B, 0.2, 1, **kw)
    scene.close()


@pytest.mark.gpu
def test_refusals_leave_outputs_and_handle_untouched(gpu):
    """8. every GNXR_ERR_INVALID condition leaves the outputs untouched, and a Render on the same handle afterwards is still bit-exact
    (an output on a device without a copy of the scene needs a second device and is not exercised here)"""
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    W, H, B = W0, H0, 8
    ref, _ = integ.Render(scene, W, H, B)
    fn = gpu.lib().gnxr_render_adaptive_device
    A, I = gpu._abi.AdaptiveParams, gpu._abi.AdaptiveInfo
    out = torch.full((H, W, 4), 7.0, device="cuda")
    cnt = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    host_img, host_cnt = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.int32)
    vp = lambda t: C.c_void_p(t.data_ptr())
    good = lambda: A(C.sizeof(A), 2, 2, 1, 0.1, 0.01)
    calls = 0

    def refused(p=None, ap=None, o=None, c=None, info=None, scene_h=scene._h, null=()):
        nonlocal calls
        args = dict(p=C.byref(p or integ.params(W, H, B)), ap=C.byref(ap or good()), o=o or vp(out), c=c or vp(cnt), st=C.byref(gpu.Stats()),
                    info=C.byref(info or I(C.sizeof(I), 0, 0, 0)))
        for k in null:
            args[k] = None
        assert fn(scene_h, args["p"], args["ap"], args["o"], args["c"], None, args["st"], args["info"]) == ERR_INVALID, gpu.lib().gnxr_last_error()
        calls += 1

    refused(scene_h=None)
    for k in ("p", "ap", "o", "info"):
        refused(null=(k,))
    refused(o=C.c_void_p(out.data_ptr() + 4))
    refused(c=C.c_void_p(cnt.data_ptr() + 2))
    refused(o=C.c_void_p(host_img.ctypes.data))
    refused(c=C.c_void_p(host_cnt.ctypes.data))
    for field, v in (("struct_size", 20), ("min_spp", 0), ("min_spp", B + 1), ("step_spp", 0), ("guard", -1), ("guard", 9), ("threshold", -1.0), ("threshold", float("nan")),
                     ("floor", -1.0), ("floor", float("nan"))):
        bad = good()
        setattr(bad, field, v)
        refused(ap=bad)
    refused(info=I(8, 0, 0, 0))
    for kw in (dict(spp_begin=1), dict(spp_end=4), dict(shard_index=1, shard_count=2), dict(shard_count=2), dict(shard_rows=2)):
        refused(p=integ.params(W, H, B, **kw))
    refused(p=integ.params(0, H, B))
    torch.cuda.synchronize()
    assert calls == 26 and (out == 7.0).all() and (cnt == 7).all() and not host_img.any() and not host_cnt.any()
    again, _ = integ.Render(scene, W, H, B)
    assert biteq(again, ref) and ref[..., :3].any()
    # count_out may be NULL
    info, st = I(C.sizeof(I), 0, 0, 0), gpu.Stats()
    p, ap = integ.params(W, H, B), good()
    assert fn(scene._h, C.byref(p), C.byref(ap), vp(out), None, None, C.byref(st), C.byref(info)) == 0
    torch.cuda.synchronize()
    L = oracle_samples("cornell", "path", W, H, B)
    S, n, rounds = adaptive_reference(L, B, 2, 2, 0.1, 0.01, 1)
    assert biteq(out.cpu().numpy(), adaptive_image(S, n)) and info.rounds == rounds and info.samples == int(n.sum()) and (cnt == 7).all()
    scene.close()
    # a scene with image textures: PathIntegrator renders, the others are refused as documented
    tex = os.path.join(ROOT, "tests", "golden", "tex_smile_96x80.hdr")
    tscene = gpu.Scene(scenes.textured_cornell(tex))
    tref, _ = integ.Render(tscene, W, H, B)
    timg, tcnt, _ = run(integ, tscene, W, H, B, 0.1, 1, min_spp=B)
    assert biteq(timg, tref) and (tcnt == B).all()
    for kind in ("whitted", "direct", "volpath"):
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
            integrator(gpu, kind).RenderAdaptive(tscene, W, H, B, 0.1, min_spp=2, step_spp=2, out=out)
    tscene.close()


@pytest.mark.gpu
def test_live_edits(gpu):
    """9. after Scene.set_camera and after update_materials the adaptive result equals that of a fresh scene"""
    integ = integrator(gpu, "path")
    W, H, B = W0, H0, 16
    cam = dict(eye=(1.2, 0.6, 4.4), look=(-0.2, -0.4, 0.0), fov=55.0)
    rec = gpu.material(type=gpu._abi.MAT_MATTE, kd=(0.1, 0.7, 0.3), sigma=20.0)
    red = 1   # scenes.cornell(): white, red, blue

    def fresh(camera, material):
        b = builder("cornell")
        if camera:
            b.set_camera(**cam)
        if material:
            b.desc().materials[red] = rec
        sc = gpu.Scene(b)
        res = run(integ, sc, W, H, B, 0.1, 1)
        sc.close()
        return res

    scene = gpu.Scene(builder("cornell"))
    base = run(integ, scene, W, H, B, 0.1, 1)
    scene.set_camera(**cam)
    a = run(integ, scene, W, H, B, 0.1, 1)
    fa = fresh(True, False)
    assert biteq(a[0], fa[0]) and (a[1] == fa[1]).all() and a[2]["rounds"] == fa[2]["rounds"] and not biteq(a[0], base[0])
    scene.update_materials([rec], first_material=red)
    m = run(integ, scene, W, H, B, 0.1, 1)
    fm = fresh(True, True)
    assert biteq(m[0], fm[0]) and (m[1] == fm[1]).all() and m[2]["rounds"] == fm[2]["rounds"] and not biteq(m[0], a[0])
    assert len(histogram(m[1])) >= 3
    scene.close()


@pytest.mark.gpu
def test_stream_semantics(gpu):
    """10. outputs filled on a side stream just before the call are overwritten, not raced; a second call on that stream follows the first"""
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("cornell"))
    W, H, B = 64, 48, 8
    kw = dict(min_spp=2, step_spp=2)
    e1 = run(integ, scene, W, H, B, 0.1, 1, **kw)
    e2 = run(integ, scene, W, H, B, 1e9, 0, **kw)
    assert not biteq(e1[0], e2[0])
    stream = torch.cuda.Stream()
    out = torch.zeros((H, W, 4), device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out.fill_(7.0)
        cnt.fill_(7)
        integ.RenderAdaptive(scene, W, H, B, 0.1, guard=1, floor=0.01, out=out, count_out=cnt, stream=stream, **kw)
        c1, n1 = out.clone(), cnt.clone()
        out.fill_(9.0)
        integ.RenderAdaptive(scene, W, H, B, 1e9, guard=0, floor=0.01, out=out, count_out=cnt, **kw)   # torch's current stream is `stream`
        c2, n2 = out.clone(), cnt.clone()
    stream.synchronize()
    assert biteq(c1.cpu().numpy(), e1[0]) and (n1.cpu().numpy() == e1[1]).all()
    assert biteq(c2.cpu().numpy(), e2[0]) and (n2.cpu().numpy() == e2[1]).all()
    scene.close()
