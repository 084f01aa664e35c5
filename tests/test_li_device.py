"""Radiance along caller rays on device memory: gnxr_li_device and PathIntegrator.Li (inherited by VolPath, Whitted, DirectLighting).

Integrator::Render is a camera loop around SamplerIntegrator::Li (core/Integrator.cpp:256-293: colObj += Li(ray, ...), then / spp), so Li
of the camera rays, summed in sample order and divided by spp, must give the render's image bit for bit -- and through it the oracle's.
Every comparison here is bit for bit (NaN-aware)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import GOLDEN, ROOT

ERR_INVALID, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -2, -4
W, H = 64, 64
ENV = os.path.join(GOLDEN, "env_100x50.hdr")
TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def camera(eye=(0, 0, 5), look=(0, 0, 0), up=(0, 1, 0), fov=90.0, lens_radius=0.0, focal_distance=3.0):
    import gnxraytracer_amd as gx
    return gx.Camera(gx._f3(eye), gx._f3(look), gx._f3(up), fov, lens_radius, focal_distance, 0)


def cam_batch(cam, spp, medium=-1, w=W, h=H):
    """the camera rays of every pixel and sample (sample-major, as the render's slots) and their records, on the device"""
    import gnxraytracer_amd as gx
    s, py, px = (a.reshape(-1) for a in np.meshgrid(np.arange(spp), np.arange(h), np.arange(w), indexing="ij"))
    o, d = gx.camera_rays(cam, w, h, px, py, s)
    rays = torch.from_numpy(gx.make_rays(o, d)).cuda()
    return rays, gx.li_samples(torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda(), torch.from_numpy(s).cuda(), medium)


def resolve(L, spp, w=W, h=H):
    """colObj += Li in sample order from 0, / spp: what k_resolve and k_finish do with the camera rays' L"""
    L = L.reshape(spp, h, w, 4)
    acc = np.zeros((h, w, 3), np.float32)
    for s in range(spp):
        acc += L[s, :, :, :3]
    return acc / np.float32(spp)


def li(integ, scene, rays, samples, spp, **kw):
    L, st = integ.Li(scene, rays, samples, W, H, spp, **kw)
    torch.cuda.synchronize()
    return L.cpu().numpy(), st


def check_identity(gpu, b, integ, spp=16, medium=None, oracle_samples=()):
    """Li of the scene camera's rays == Render, per pixel and per sample; the ray counts add up to the render's"""
    scene = gpu.Scene(b)
    d = b.desc()
    rays, samples = cam_batch(d.camera, spp, d.camera_medium if medium is None else medium)
    L, st = li(integ, scene, rays, samples, spp)
    assert (L[:, 3] == 1).all()
    img, rst = integ.Render(scene, W, H, spp)
    assert biteq(resolve(L, spp), img[..., :3])
    for k in ("rays_closest", "rays_any", "rays_closest_nee"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["camera_samples"] == W * H * spp and st["state_bytes"] > 0 and st["passes_in_flight"] >= 1
    per = L.reshape(spp, H, W, 4)[..., :3] / np.float32(spp)
    for s in sorted({0, spp - 1}):
        one, _ = integ.Render(scene, W, H, spp, spp_begin=s, spp_end=s + 1)
        assert biteq(per[s], one[..., :3]), s
    if oracle_samples:
        osc = ol.OracleScene(b)
        for s in oracle_samples:
            oimg, _ = osc.render(integ, W, H, spp, spp_begin=s, spp_end=s + 1)
            assert biteq(per[s], oimg[..., :3]), s
    scene.close()
    return L


# ---- CPU ----

def test_li_device_is_declared_exported_and_bound(gx):
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    assert re.search(r"\bgnxr_li_device\s*\(", hdr)
    assert hasattr(C.CDLL(gx.LIB_PATH), "gnxr_li_device")
    assert "gnxr_li_device" in gx._abi.PROTOTYPES


def test_li_sample_abi(gx):
    assert gx.lib().gnxr_abi_sizeof(11) == 16 == C.sizeof(gx.LiSample)
    assert gx._abi.ABI_STRUCTS[-1] is gx.LiSample and gx._abi.ABI_STRUCTS.index(gx.LiSample) == 11
    assert gx.lib().gnxr_abi_version() == 5


def test_li_samples_layout_and_checks(gx):
    t = gx.li_samples(torch.tensor([1, 2, 3]), 4, torch.tensor([5, 6, 7], dtype=torch.int16))
    assert t.dtype == torch.int32 and t.shape == (3, 4) and t.is_contiguous()
    assert t.tolist() == [[1, 4, 5, -1], [2, 4, 6, -1], [3, 4, 7, -1]]
    assert gx.li_samples(0, 1, 2, 3).tolist() == [[0, 1, 2, 3]]
    for bad in ((torch.zeros(3), 0, 0), (torch.zeros((3, 1), dtype=torch.int32), 0, 0), (0.5, 0, 0), (0, "1", 0),
                (torch.arange(3), torch.arange(4), 0)):
        with pytest.raises(ValueError):
            gx.li_samples(*bad)


def test_li_tensor_checks(gx):
    integ = gx.PathIntegrator(5)
    rays, samples = torch.zeros((4, 8)), torch.zeros((4, 4), dtype=torch.int32)
    for r, s, kw in ((rays.double(), samples, {}), (rays[:, :7].contiguous(), samples, {}), (rays, samples.long(), {}),
                     (rays, samples[:, :3].contiguous(), {}), (rays, samples[:3], {}), (rays.t().contiguous().t(), samples, {}),
                     (rays, samples, {"out": torch.zeros((4, 3))}), (rays, samples, {"out": torch.zeros((3, 4))})):
        with pytest.raises(ValueError):
            integ.Li(None, r, s, 64, 64, 4, **kw)


def test_li_device_without_a_device(gx):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the failure path cannot be observed")
    p = gx.PathIntegrator(5).params(64, 64, 4)
    assert gx.lib().gnxr_li_device(None, C.byref(p), None, None, 0, None, None, None) == ERR_NO_DEVICE


# ---- GPU ----

@pytest.mark.gpu
def test_li_of_camera_rays_equals_render(gpu):
    """1. Li of every pixel's camera rays == PathIntegrator.Render, image and ray counts; one sample == the render of that sample."""
    check_identity(gpu, scenes.cornell(), gpu.PathIntegrator(5, 1.0, "spatial"), oracle_samples=(0, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dragon_env", "sphere_glass", "delta", "textured"])
def test_li_scene_coverage(gpu, name):
    """2. the escape class and the environment light, a glass sphere, delta lights, image textures under Path"""
    b = {"dragon_env": lambda: scenes.dragon_cornell(2000, "glass+metal", env=ENV),
         "sphere_glass": lambda: scenes.cornell_sphere("glass"),
         "delta": lambda: scenes.delta_cornell(),
         "textured": lambda: scenes.textured_cornell(TEX)}[name]()
    check_identity(gpu, b, gpu.PathIntegrator(5, 1.0, "spatial"), oracle_samples=(3,) if name == "dragon_env" else ())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fog", "volume"])
def test_li_volpath(gpu, name):
    """3. VolPath: the camera in fog (every record names the camera's medium) and a heterogeneous volume"""
    b = scenes.cornell_in_fog() if name == "fog" else scenes.volume_cornell()
    assert (b.desc().camera_medium >= 0) == (name == "fog")
    check_identity(gpu, b, gpu.VolPathIntegrator(5, 1.0, "spatial"), spp=8)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["whitted", "direct_all", "direct_one"])
def test_li_whitted_and_direct(gpu, kind):
    """3. Whitted and DirectLighting ("all", "one") on untextured scenes"""
    integ = {"whitted": lambda: gpu.WhittedIntegrator(5), "direct_all": lambda: gpu.DirectLightingIntegrator("all", 5),
             "direct_one": lambda: gpu.DirectLightingIntegrator("one", 5)}[kind]()
    b = scenes.cornell_sphere("glass")
    L = check_identity(gpu, b, integ, spp=8)
    scene = gpu.Scene(b)
    rays, samples = cam_batch(b.desc().camera, 8)
    Lc, st = li(integ, scene, rays, samples, 8, samples_per_pass=3000)   # the pass loop in chunks of 3000 rays, the last one short
    assert biteq(Lc, L) and st["passes"] == -(-rays.shape[0] // 3000)
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["whitted", "direct", "volpath"])
def test_li_textured_needs_differentials(gpu, kind):
    """3. Whitted / DirectLighting / VolPath on an image-textured scene would need camera ray differentials: GNXR_ERR_UNSUPPORTED"""
    b = scenes.textured_cornell(TEX)
    scene = gpu.Scene(b)
    integ = {"whitted": gpu.WhittedIntegrator(5), "direct": gpu.DirectLightingIntegrator("all", 5), "volpath": gpu.VolPathIntegrator(5)}[kind]
    rays, samples = cam_batch(b.desc().camera, 1)
    out = torch.full((rays.shape[0], 4), 7.0, device="cuda")
    with pytest.raises(gpu.GnxrError, match="-4"):
        integ.Li(scene, rays, samples, W, H, 1, out=out)
    assert (out == 7.0).all()


@pytest.mark.gpu
def test_li_is_independent_of_the_scene_camera(gpu):
    """4. rays and records of camera B (another eye, fov, a lens) on a scene whose camera is A == the render after set_camera(B)"""
    b = scenes.cornell()
    scene = gpu.Scene(b)
    B = dict(eye=(1.0, 0.5, 4.0), look=(-0.2, -0.3, 0.0), up=(0, 1, 0), fov=70.0, lens_radius=0.08, focal_distance=4.0)
    spp = 8
    integ = gpu.PathIntegrator(5)
    rays, samples = cam_batch(camera(**B), spp)
    L, _ = li(integ, scene, rays, samples, spp)
    scene.set_camera(**B)
    img, _ = integ.Render(scene, W, H, spp)
    assert biteq(resolve(L, spp), img[..., :3])
    scene.close()


@pytest.mark.gpu
def test_li_batch_shape_invariance(gpu):
    """5. shuffled records give shuffled results; small sub-passes with 1 and 4 in flight change nothing; two image batches
    interleaved in one call give what each gives alone"""
    b = scenes.dragon_cornell(2000, "glass+metal", env=ENV)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5)
    spp = 4
    rays, samples = cam_batch(b.desc().camera, spp)
    L, _ = li(integ, scene, rays, samples, spp)
    perm = torch.randperm(rays.shape[0], generator=torch.Generator().manual_seed(5)).cuda()
    Lp, _ = li(integ, scene, rays[perm].contiguous(), samples[perm].contiguous(), spp)
    assert biteq(Lp, L[perm.cpu().numpy()])
    for pif in (1, 4):
        Ls, st = li(integ, scene, rays, samples, spp, samples_per_pass=3000, passes_in_flight=pif)
        assert biteq(Ls, L) and st["passes_in_flight"] == pif, pif
    rays_b, samples_b = cam_batch(camera(eye=(-1, 1, 4.5), fov=60.0), spp)
    Lb, _ = li(integ, scene, rays_b, samples_b, spp)
    mix_r = torch.stack([rays, rays_b], 1).reshape(-1, 8).contiguous()
    mix_s = torch.stack([samples, samples_b], 1).reshape(-1, 4).contiguous()
    Lm, _ = li(integ, scene, mix_r, mix_s, spp, samples_per_pass=5000)
    assert biteq(Lm[0::2], L) and biteq(Lm[1::2], Lb)
    scene.close()


@pytest.mark.gpu
def test_li_volpath_mixed_media(gpu):
    """5. VolPath: fog rays (medium = m) interleaved with rays that start in no medium == each batch alone"""
    b = scenes.cornell_in_fog()
    m = b.desc().camera_medium
    scene = gpu.Scene(b)
    integ = gpu.VolPathIntegrator(5)
    spp = 4
    rays, fog = cam_batch(b.desc().camera, spp, m)
    clear = fog.clone()
    clear[:, 3] = -1
    La, _ = li(integ, scene, rays, fog, spp)
    Lb, _ = li(integ, scene, rays, clear, spp)
    assert not biteq(La, Lb)
    Lm, _ = li(integ, scene, torch.stack([rays, rays], 1).reshape(-1, 8).contiguous(), torch.stack([fog, clear], 1).reshape(-1, 4).contiguous(), spp)
    assert biteq(Lm[0::2], La) and biteq(Lm[1::2], Lb)
    Lc, _ = li(integ, scene, torch.stack([rays, rays], 1).reshape(-1, 8).contiguous(), torch.stack([fog, clear], 1).reshape(-1, 4).contiguous(), spp,
               samples_per_pass=5000)
    assert biteq(Lc, Lm)
    scene.close()


@pytest.mark.gpu
def test_li_volpath_packed(gpu):
    """VolPath at 128 x 128 x 16 in fog: enough survivors for the rounds that pack the live paths to the front (k_vol_pack), whose results
    stay at their original slots"""
    b = scenes.cornell_in_fog()
    scene = gpu.Scene(b)
    integ = gpu.VolPathIntegrator(5)
    w = h = 128
    spp = 16
    rays, samples = cam_batch(b.desc().camera, spp, b.desc().camera_medium, w, h)
    L, st = integ.Li(scene, rays, samples, w, h, spp)
    img, rst = integ.Render(scene, w, h, spp)
    assert biteq(resolve(L.cpu().numpy(), spp, w, h), img[..., :3])
    assert (st["rays_closest"], st["media_segments"]) == (rst["rays_closest"], rst["media_segments"])
    scene.close()


@pytest.mark.gpu
def test_li_caller_tmax(gpu):
    """6. rays that end before their first hit: Path adds beta * Le of the infinite lights at bounce 0 (oracle light_le), or nothing"""
    spp = 2
    for b, env in ((scenes.dragon_cornell(2000, "glass+metal", env=ENV), True), (scenes.cornell(), False)):
        scene = gpu.Scene(b)
        rays, samples = cam_batch(b.desc().camera, spp)
        rays[:, 3] = 1e-3
        L, _ = li(gpu.PathIntegrator(5), scene, rays, samples, spp)
        if env:
            d = b.desc()
            assert d.n_lights == 3   # two area-light triangles, then the InfiniteAreaLight
            ref = ol.OracleScene(b).light_le(2, rays.cpu().numpy())
            assert (ref > 0).any() and biteq(L[:, :3], ref)
        else:
            assert (L[:, :3] == 0).all()
        scene.close()


@pytest.mark.gpu
def test_li_errors(gpu):
    """7. host memory, misaligned pointers and bad params fail before anything runs; a record out of range fails after the run with
    its row zeroed and every other row unchanged; n == 0 is a no-op"""
    b = scenes.cornell()
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5)
    spp = 2
    rays, samples = cam_batch(b.desc().camera, spp)
    n = rays.shape[0]
    fn = gpu.lib().gnxr_li_device
    p = integ.params(W, H, spp)
    st = gpu.Stats()
    out = torch.full((n + 1, 4), 7.0, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    hr, hs, hl = rays.cpu(), samples.cpu(), out.cpu()
    assert fn(scene._h, C.byref(p), vp(hr), vp(hs), n, vp(hl), None, C.byref(st)) == ERR_INVALID
    assert fn(scene._h, C.byref(p), vp(rays), vp(samples), n, vp(out, 4), None, C.byref(st)) == ERR_INVALID
    assert fn(scene._h, C.byref(p), vp(rays), vp(samples), n, None, None, C.byref(st)) == ERR_INVALID
    assert fn(None, C.byref(p), vp(rays), vp(samples), n, vp(out), None, C.byref(st)) == ERR_INVALID
    assert fn(scene._h, C.byref(p), vp(rays), vp(samples), -1, vp(out), None, C.byref(st)) == ERR_INVALID
    for bad in (dict(spp_begin=1, spp_end=2), dict(shard_count=2), dict(shard_index=1)):
        q = integ.params(W, H, spp, **bad)
        assert fn(scene._h, C.byref(q), vp(rays), vp(samples), n, vp(out), None, C.byref(st)) == ERR_INVALID, bad
    q = integ.params(0, H, spp)
    assert fn(scene._h, C.byref(q), vp(rays), vp(samples), n, vp(out), None, C.byref(st)) == ERR_INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    good, _ = li(integ, scene, rays, samples, spp)
    bad = samples.clone()
    bad[100, 0] = W
    bad[200, 3] = 0    # cornell() has no media: medium 0 is out of range too
    out = torch.full((n, 4), 7.0, device="cuda")
    with pytest.raises(gpu.GnxrError, match="record 100 "):
        integ.Li(scene, rays, bad, W, H, spp, out=out)
    got = out.cpu().numpy()
    assert (got[100] == 0).all() and (got[200] == 0).all()
    keep = np.ones(n, bool)
    keep[[100, 200]] = False
    assert biteq(got[keep], good[keep])
    # the handle is fine afterwards
    again, _ = li(integ, scene, rays, samples, spp)
    assert biteq(again, good)
    e = torch.empty((0, 8), device="cuda")
    L0, st0 = integ.Li(scene, e, torch.empty((0, 4), dtype=torch.int32, device="cuda"), W, H, spp)
    assert L0.shape == (0, 4) and st0["camera_samples"] == 0
    scene.close()


@pytest.mark.gpu
def test_li_panorama_example(gpu):
    """the equirectangular panorama of INTEGRATION.md section 2e, small: runs, and sees the walls and the light"""
    import math
    b = scenes.cornell()
    scene = gpu.Scene(b)
    W_, H_, spp = 64, 32, 4
    s, y, x = torch.meshgrid(torch.arange(spp), torch.arange(H_), torch.arange(W_), indexing="ij")
    s, y, x = (t.reshape(-1).cuda() for t in (s, y, x))
    g = torch.Generator(device="cuda").manual_seed(1)
    u, v = torch.rand(x.shape, device="cuda", generator=g), torch.rand(x.shape, device="cuda", generator=g)
    phi, theta = 2 * math.pi * (x + u) / W_, math.pi * (y + v) / H_
    d = torch.stack([torch.sin(theta) * torch.sin(phi), torch.cos(theta), -torch.sin(theta) * torch.cos(phi)], 1)
    eye = torch.tensor(list(b.desc().camera.eye), device="cuda").expand_as(d)
    L, st = gpu.PathIntegrator(5).Li(scene, gpu.rays_tensor(eye, d), gpu.li_samples(x, y, s), W_, H_, spp)
    pano = L.view(spp, H_, W_, 4)[..., :3].mean(0).cpu().numpy()
    assert pano.shape == (H_, W_, 3) and np.isfinite(pano).all() and (pano.sum(-1) > 0).mean() > 0.05 and st["camera_samples"] == W_ * H_ * spp
    scene.close()
