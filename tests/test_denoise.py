"""The edge-aware denoiser: gnxr_denoise_device / gx.denoise / integrator.RenderDenoised against tests/denoise_reference.py.

The definition (include/gnxr.h) is a sequence of single fp32 operations, so every GPU comparison is exact: the uint32 views of the
device's output equal the numpy restatement's, no tolerance, no pixel left out.  The reference's expf is the device's libm probe on
the GPU tests (glibc's bits) and the C library's expf on the CPU tests.
"""
import ctypes as C
import functools
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import scenes
from conftest import ROOT
from denoise_reference import denoise_reference, glibc_expf

ERR_INVALID = -1
GUIDES = ("albedo", "normal", "depth")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def biteq(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


@functools.lru_cache(maxsize=None)
def synthetic():
    """The two-plane input of the issue's prototype, 35 x 67: (inputs dict, noise-free image)"""
    H, W = 35, 67
    y, x = np.mgrid[0:H, 0:W]
    left = x < 30
    normal = np.zeros((H, W, 4), np.float32)
    normal[left, :3] = (0.6, 0.0, 0.8)
    normal[~left, :3] = (0.0, 0.0, 1.0)
    depth = np.where(left, 3 + 0.02 * (30 - x), 3 + 0.001 * y).astype(np.float32)
    albedo = np.ones((H, W, 4), np.float32)
    albedo[..., :3] = (0.2 + 0.6 * ((x // 4 + y // 4) % 2))[..., None]
    irradiance = np.where(left, 0.5, 1.0) * (1 + 0.3 * np.sin(y / 8))
    truth = np.ones((H, W, 4), np.float32)
    truth[..., :3] = albedo[..., :3] * irradiance[..., None]
    rng = np.random.default_rng(1)
    shares = []
    for _ in range(2):
        s = np.ones((H, W, 4), np.float32)
        s[..., :3] = truth[..., :3] * rng.gamma(2.0, 0.5, (H, W, 3)) * 0.5
        shares.append(s)
    arrs = dict(color=shares[0], color_b=shares[1], albedo=albedo, normal=normal, depth=depth)
    for v in list(arrs.values()) + [truth]:
        v.setflags(write=False)
    return arrs, truth


@functools.lru_cache(maxsize=None)
def random_inputs(V, H, W, seed=0):
    """Uniform random shares and albedo over smooth guides, different in every view; V == 0: a single (H, W, 4) image.
    The guides are a plane per view with a little noise -- its own normal, a depth ramp of 0.2 % per column and 0.1 % per row --
    so that under the default sigmas a neighbouring tap's exponent is a few tenths and EVERY tap moves bits of the sums
    (uniform random normals and depths would give most taps weights of e^-30, which vanish in the rounding)."""
    rng = np.random.default_rng(seed + 1000 * V + 10 * H + W)
    lead = (V,) if V else ()
    u = lambda *tail: rng.random(lead + (H, W) + tail, dtype=np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    plane = rng.random(lead + (1, 1, 4), dtype=np.float32) * 2 - 1                # the normal of each view's plane
    normal = (plane + (u(4) * 2 - 1) * np.float32(0.1)).astype(np.float32)
    normal[..., 3] = 0
    near = 2 + 3 * rng.random(lead + (1, 1), dtype=np.float32)                    # the depth of each view's first pixel
    depth = (near * (1 + np.float32(0.002) * x + np.float32(0.001) * y) * (1 + np.float32(0.001) * u())).astype(np.float32)
    arrs = dict(color=u(4), color_b=u(4), albedo=u(4), normal=normal, depth=depth)
    for v in arrs.values():
        v.setflags(write=False)
    return arrs


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3]) ** 2)))


def pick(arrs, second, guides):
    return {k: v for k, v in arrs.items() if k == "color" or (k == "color_b" and second) or k in guides}


def device_expf(gx):
    return lambda x: gx.eval_libm("exp", x)


def on_device(arrs):
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in arrs.items()}


def run_device(gx, arrs, **kw):
    out = gx.denoise(**on_device(arrs), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_case(gx, arrs, **kw):
    got = run_device(gx, arrs, **kw)
    want = denoise_reference(**arrs, expf=device_expf(gx), **kw)
    diff = bits(got) != bits(want)
    print("pixels that differ:", int(diff.any(axis=-1).sum()), "of", diff[..., 0].size)
    assert got.shape == want.shape and not diff.any()
    return got


# ---------------------------------------------------------------- CPU
def test_denoise_entry_point_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    assert re.search(r"\bgnxr_denoise_device\s*\(", hdr)
    assert hasattr(gx.lib(), "gnxr_denoise_device") and "gnxr_denoise_device" in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.DenoiseParams) == 32 and C.sizeof(gx._abi.DenoiseBuffers) == 48
    assert callable(gx.denoise) and gx.VolPathIntegrator.RenderDenoised is gx.PathIntegrator.RenderDenoised


def test_reference_lowers_the_error_of_the_synthetic_input():
    """five iterations with the defaults: the RMSE against the noise-free image falls below half that of a + b (prototype: 0.14 of it)"""
    arrs, truth = synthetic()
    out = denoise_reference(**arrs, expf=glibc_expf)
    noisy = arrs["color"] + arrs["color_b"]
    e_in, e_out = rmse(noisy, truth), rmse(out, truth)
    print(f"rmse: a + b {e_in:.4f}, denoised {e_out:.4f}, ratio {e_out / e_in:.3f}")
    assert np.isfinite(out).all() and biteq(out[..., 3], arrs["color"][..., 3])
    assert e_out < 0.5 * e_in
    single = denoise_reference(noisy, None, arrs["albedo"], arrs["normal"], arrs["depth"], expf=glibc_expf)
    print(f"rmse without a second image: {rmse(single, truth):.4f}")
    assert rmse(single, truth) < 0.5 * e_in


def test_reference_repairs_non_finite_pixels_and_runs_on_a_tiny_image():
    arrs, _ = synthetic()
    a = np.array(arrs["color"])
    a[5, 7, 1] = np.nan
    a[20, 40, 0] = np.inf
    out = denoise_reference(a, arrs["color_b"], arrs["albedo"], arrs["normal"], arrs["depth"], expf=glibc_expf)
    assert np.isfinite(out).all()
    tiny = random_inputs(0, 2, 3)
    out = denoise_reference(**tiny, iterations=5, expf=glibc_expf)
    assert out.shape == (2, 3, 4) and np.isfinite(out).all()


# ---------------------------------------------------------------- GPU: bit equality with the reference
@pytest.mark.gpu
@pytest.mark.parametrize("second", [True, False], ids=["two_shares", "one_image"])
@pytest.mark.parametrize("guides", [g for n in range(4) for g in itertools.combinations(GUIDES, n)], ids=lambda g: "+".join(g) or "no_guides")
def test_synthetic_input_every_subset_of_guides(gpu, second, guides):
    check_case(gpu, pick(synthetic()[0], second, guides))


@pytest.mark.gpu
@pytest.mark.parametrize("second", [True, False], ids=["two_shares", "one_image"])
@pytest.mark.parametrize("zero", ["sigma_color", "sigma_normal", "sigma_depth"])
def test_synthetic_input_each_sigma_at_zero(gpu, second, zero):
    check_case(gpu, pick(synthetic()[0], second, GUIDES), **{zero: 0.0})


@pytest.mark.gpu
@pytest.mark.parametrize("second", [True, False], ids=["two_shares", "one_image"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("shape", [(0, 2, 3), (0, 35, 67), (0, 5, 4100), (3, 19, 70)], ids=lambda s: "x".join(map(str, s)))
def test_random_images_sizes_views_and_iterations(gpu, shape, iterations, second):
    """a step of 128 reaches beyond every image; 4100 columns are more than one row of tiles; in the three views a tap that leaks into
    the neighbouring view changes bits"""
    check_case(gpu, pick(random_inputs(*shape), second, GUIDES), iterations=iterations)


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 5])
def test_non_finite_and_degenerate_data(gpu, iterations):
    arrs = {k: np.array(v) for k, v in random_inputs(0, 19, 23, seed=3).items()}
    a, b, albedo, normal = arrs["color"], arrs["color_b"], arrs["albedo"], arrs["normal"]
    a[2, 3, 0] = np.nan
    a[2, 9, 2] = np.inf
    b[7, 3, 1] = np.nan
    b[7, 9, 0] = -np.inf
    normal[12, 4, 1] = np.nan
    normal[12, 10, 0] = np.inf
    albedo[1:4, 14:18] = (0, 0, 0, 1)       # albedo 0 under full coverage: divided by 1/1024
    albedo[5:8, 14:18, 3] = 0               # coverage 0: a miss counts as albedo 1
    a[12:17, 16:21, 0] = np.nan             # a whole 5 x 5 block invalid: one iteration leaves its centre as it is
    for second in (True, False):
        got = check_case(gpu, pick(arrs, second, GUIDES), iterations=iterations)
        assert np.isfinite(got[14, 18]).all() == (iterations > 1)
        if iterations > 1:
            assert np.isfinite(got).all()


@pytest.mark.gpu
def test_in_place(gpu):
    arrs = pick(synthetic()[0], True, GUIDES)
    want = run_device(gpu, arrs)
    for target in ("color", "color_b"):
        dev = on_device(arrs)
        out = gpu.denoise(**dev, out=dev[target])
        torch.cuda.synchronize()
        assert out is dev[target] and biteq(out.cpu().numpy(), want)
    dev = on_device(pick(synthetic()[0], False, GUIDES))
    want = run_device(gpu, pick(synthetic()[0], False, GUIDES))
    assert biteq(gpu.denoise(**dev, out=dev["color"]).cpu().numpy(), want)


@pytest.mark.gpu
def test_ordering_on_a_side_stream_and_repeatability(gpu):
    arrs = pick(random_inputs(3, 19, 70), True, GUIDES)
    want = run_device(gpu, arrs)
    assert biteq(run_device(gpu, arrs), want)
    host = {k: torch.from_numpy(np.array(v)).pin_memory() for k, v in arrs.items()}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = {k: torch.zeros_like(v, device="cuda") for k, v in host.items()}
        for k in dev:
            dev[k].copy_(host[k], non_blocking=True)   # queued on the side stream; the call below must run after them
        out = gpu.denoise(**dev, stream=side)
    side.synchronize()
    assert biteq(out.cpu().numpy(), want)


# ---------------------------------------------------------------- GPU: refusals
def raw_call(gx, bufs, out, width=8, height=6, n_views=1, iterations=5, sigmas=(4.0, 0.5, 0.05), p_size=None, b_size=None, null_p=False, null_in=False):
    """gnxr_denoise_device with every field under the caller's control; bufs: dict name -> address"""
    A = gx._abi
    p = A.DenoiseParams(C.sizeof(A.DenoiseParams) if p_size is None else p_size, width, height, n_views, iterations, *sigmas)
    b = A.DenoiseBuffers(C.sizeof(A.DenoiseBuffers) if b_size is None else b_size, 0, *[C.c_void_p(bufs.get(k) or None) for k in ("color", "color_b") + GUIDES])
    return gx.lib().gnxr_denoise_device(None if null_p else C.byref(p), None if null_in else C.byref(b), C.c_void_p(out or None), None)


@pytest.mark.gpu
def test_every_refusal_leaves_the_output_untouched(gpu):
    gx = gpu
    H, W = 6, 8
    dev = on_device(random_inputs(0, H, W))
    out = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    spare = torch.zeros((H * W * 4 + 8,), dtype=torch.float32, device="cuda")
    host = np.zeros((H, W, 4), np.float32)
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    o = out.data_ptr()
    assert o % 16 == 0 and all(v % 16 == 0 for v in ptr.values()) and spare.data_ptr() % 16 == 0
    nan = float("nan")
    cases = {
        "null params": dict(bufs=ptr, out=o, null_p=True),
        "null buffers": dict(bufs=ptr, out=o, null_in=True),
        "null d_color": dict(bufs={**ptr, "color": 0}, out=o),
        "null d_rgba_out": dict(bufs=ptr, out=0),
        "params struct_size": dict(bufs=ptr, out=o, p_size=28),
        "buffers struct_size": dict(bufs=ptr, out=o, b_size=40),
        "width 0": dict(bufs=ptr, out=o, width=0),
        "height 0": dict(bufs=ptr, out=o, height=0),
        "n_views -1": dict(bufs=ptr, out=o, n_views=-1),
        "iterations 0": dict(bufs=ptr, out=o, iterations=0),
        "iterations 9": dict(bufs=ptr, out=o, iterations=9),
        "sigma_color < 0": dict(bufs=ptr, out=o, sigmas=(-1.0, 0.5, 0.05)),
        "sigma_normal < 0": dict(bufs=ptr, out=o, sigmas=(4.0, -0.5, 0.05)),
        "sigma_depth < 0": dict(bufs=ptr, out=o, sigmas=(4.0, 0.5, -0.05)),
        "sigma_color NaN": dict(bufs=ptr, out=o, sigmas=(nan, 0.5, 0.05)),
        "sigma_normal NaN": dict(bufs=ptr, out=o, sigmas=(4.0, nan, 0.05)),
        "sigma_depth NaN": dict(bufs=ptr, out=o, sigmas=(4.0, 0.5, nan)),
        "host d_rgba_out": dict(bufs=ptr, out=host.ctypes.data),
        "d_rgba_out misaligned": dict(bufs=ptr, out=spare.data_ptr() + 4),
        "d_rgba_out overlaps d_albedo": dict(bufs=ptr, out=ptr["albedo"]),
        "d_rgba_out overlaps d_normal": dict(bufs=ptr, out=ptr["normal"]),
        "d_rgba_out overlaps d_depth": dict(bufs={**ptr, "depth": o + 64}, out=o),
        "d_rgba_out overlaps d_color at an offset": dict(bufs=ptr, out=ptr["color"] + 64),
        "d_rgba_out overlaps d_color_b at an offset": dict(bufs={**ptr, "color_b": o + 16}, out=o),
        "too many pixels": dict(bufs=ptr, out=o, width=65536, height=65536),
    }
    for k in ("color", "color_b") + GUIDES:
        cases[f"host d_{k}"] = dict(bufs={**ptr, k: host.ctypes.data}, out=o)
        cases[f"d_{k} misaligned"] = dict(bufs={**ptr, k: spare.data_ptr() + (2 if k == "depth" else 4)}, out=o)
    for name, kw in cases.items():
        rc = raw_call(gx, **kw)
        assert rc == ERR_INVALID, (name, rc)
        with pytest.raises(gx.GnxrError):
            gx._check(rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all().item())
    # n_views == 0 is a no-op; the same buffers with valid arguments are accepted
    assert raw_call(gx, ptr, o, width=W, height=H, n_views=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all().item())
    assert raw_call(gx, ptr, o, width=W, height=H) == 0
    torch.cuda.synchronize()
    want = denoise_reference(**random_inputs(0, H, W), sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.05, expf=device_expf(gx))   # raw_call's sigmas
    assert biteq(out.cpu().numpy(), want)


@pytest.mark.gpu
def test_python_value_errors(gpu):
    gx = gpu
    dev = on_device(random_inputs(0, 6, 8))
    c = dev["color"]
    bad = [
        dict(color=c.cpu()), dict(color=c.double()), dict(color=c[:, :, :3]), dict(color=c[0]), dict(color=c.permute(1, 0, 2)), dict(color=np.zeros((6, 8, 4), np.float32)),
        dict(color=c, color_b=c[:5]), dict(color=c, albedo=c.cpu()), dict(color=c, normal=c.half()), dict(color=c, depth=dev["depth"][None]), dict(color=c, depth=c),
        dict(color=c, iterations=0), dict(color=c, iterations=9), dict(color=c, sigma_color=-1.0), dict(color=c, sigma_normal=float("nan")), dict(color=c, sigma_depth=-0.1),
        dict(color=c, out=torch.zeros((6, 8, 3), device="cuda")), dict(color=c, out=torch.zeros((6, 8, 4), dtype=torch.float64, device="cuda")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            gx.denoise(**kw)
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(scenes.cornell())
    for kw in (dict(spp=3), dict(spp=0), dict(spp=4, normal="ids"), dict(spp=4, media=[-1]), dict(spp=4, sigma=1.0), dict(spp=4, iterations=9)):
        with pytest.raises(ValueError):
            integ.RenderDenoised(scene, 16, 16, **kw)
    with pytest.raises(gx.GnxrError):   # a guide as the output: the library's refusal reaches the caller
        gx.denoise(c, albedo=dev["albedo"], out=dev["albedo"])
    scene.close()


# ---------------------------------------------------------------- GPU: end to end
CAMS = [dict(eye=(1.2, 0.6, 4.4), look=(-0.2, -0.4, 0.0), fov=55.0), dict(eye=(-0.8, 0.2, 4.0), look=(0.3, -0.6, 0.0), fov=70.0)]


def composition(gx, integ, scene, W, H, spp, cameras):
    """RenderDenoised by hand: the two halves, the feature buffers, denoise; returns (inputs as numpy, device output, stats of the halves)"""
    halves, stats = [], []
    for lo, hi in ((0, spp // 2), (spp // 2, spp)):
        if cameras is not None:
            img, st = integ.RenderViews(scene, cameras, W, H, spp, spp_begin=lo, spp_end=hi)
        else:
            img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            st = integ.RenderDevice(scene, img.data_ptr(), W, H, spp, stream=torch.cuda.current_stream().cuda_stream, spp_begin=lo, spp_end=hi)
        halves.append(img)
        stats.append(st)
    aov, aov_st = integ.RenderAOV(scene, W, H, spp, cameras=cameras, channels=("albedo", "shading_normal", "depth"))
    out = gx.denoise(halves[0], halves[1], albedo=aov["albedo"], normal=aov["shading_normal"], depth=aov["depth"])
    torch.cuda.synchronize()
    arrs = dict(color=halves[0], color_b=halves[1], albedo=aov["albedo"], normal=aov["shading_normal"], depth=aov["depth"])
    return {k: v.cpu().numpy() for k, v in arrs.items()}, out.cpu().numpy(), stats, aov_st


@pytest.mark.gpu
@pytest.mark.parametrize("views", ["own_camera", "two_cameras"])
def test_render_denoised_is_its_composition_and_the_reference(gpu, views):
    gx = gpu
    W, H, spp = 64, 64, 16
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(scenes.cornell())
    cameras = [gx.camera(**c) for c in CAMS] if views == "two_cameras" else None
    img, st = integ.RenderDenoised(scene, W, H, spp, cameras=cameras)
    torch.cuda.synchronize()
    img = img.cpu().numpy()
    arrs, by_hand, stats, aov_st = composition(gx, integ, scene, W, H, spp, cameras)
    assert img.shape == ((2, H, W, 4) if cameras else (H, W, 4)) and img[..., :3].any()
    assert biteq(img, by_hand)
    assert biteq(img, denoise_reference(**arrs, expf=device_expf(gx)))
    for k in ("rays_closest", "rays_any", "camera_samples"):
        assert st[k] == stats[0][k] + stats[1][k]
    assert st["camera_samples"] == W * H * spp * (2 if cameras else 1) == st["aov"]["camera_samples"] == aov_st["camera_samples"]
    scene.close()


@pytest.mark.gpu
def test_default_settings_lower_the_error_of_a_cornell_render(gpu):
    """128 x 128 at 16 spp against 2048 spp: the reference's output -- which the device equals -- is closer than the sum of the halves"""
    gx = gpu
    W, H, spp = 128, 128, 16
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(scenes.cornell())
    arrs, out, _, _ = composition(gx, integ, scene, W, H, spp, None)
    want = denoise_reference(**arrs, expf=device_expf(gx))
    assert biteq(out, want)
    truth, _ = integ.Render(scene, W, H, 2048)
    noisy = arrs["color"] + arrs["color_b"]
    e_in, e_out = rmse(noisy, truth), rmse(want, truth)
    print(f"rmse against 2048 spp: 16 spp {e_in:.5f}, denoised {e_out:.5f}, ratio {e_out / e_in:.3f}")
    assert e_out < e_in
    scene.close()
