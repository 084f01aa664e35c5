"""gnxr_scene_update_textures: image textures of a live scene replaced on the device, their MIP pyramids built there
(csrc/texture_build_kernel.hip.h, csrc/api_textures.hip.h).

Every comparison is bit for bit and against gnxr_scene_create, whose host code (build_textures, csrc/scene_compile.cpp -- pinned against
the compiled reference by test_textured_images and test_textured_materials_match_reference) is the yardstick: scene A is created from the
base description and edited, scene B is created from a description carrying the new records and texels, and the two must hold the same
tables (Scene.texture_tables: every word of the device's texture records, the level offsets among them, and every texel of every level)
and give the same results.  The base scene is scenes.textured_cornell: texture 0 the back wall's Kd = Ks (EWA, Repeat), texture 1 the
floor's Kd (trilinear, Clamp, gamma, scale 0.8); renders are 48 x 40 at 4 spp.  No tolerance anywhere.  Texels are finite: NaN and
infinite values are out of scope."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import scenes
from conftest import ROOT
from gnxraytracer_amd import _abi as A
from test_aov import TEX
from test_material_update import desc_materials
from test_scene_update import biteq, deform, emissive_vertices, same_render, vertices
from test_shading_queries import dbsdf, probes, synthetic_differentials

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W, H, SPP = 48, 40, 4
WALL, FLOOR = 0, 1                    # the textures of scenes.textured_cornell
WRAPS = {"repeat": 0, "black": 1, "clamp": 2}
N_LEVELS, W0, H0, OFFSET0 = 0, 1, 2, 10   # words of a texture record (DTexture): the levels, the padded size, level_offset[0]
SHAPES = [(4, 4), (1, 1), (8, 2), (5, 3), (1, 7), (6, 1), (33, 17), (100, 60)]   # (w, h): see test_tables_equal_a_created_scene


# ---------------------------------------------------------------- helpers
def base(**kw):
    return scenes.textured_cornell(TEX, **kw)


def copy_of(t):
    out = A.Texture()
    C.memmove(C.byref(out), C.byref(t), C.sizeof(A.Texture))
    return out


def desc_textures(b):
    """copies of the description's texture records, and per texture its image as (h, w, 3)"""
    d = b.desc()
    recs, images = [], []
    for i in range(d.n_textures):
        t = copy_of(d.textures[i])
        n = t.width * t.height * 3
        images.append(np.ctypeslib.as_array(d.texels, shape=(t.texel_offset + n,))[t.texel_offset:].copy().reshape(t.height, t.width, 3))
        recs.append(t)
    return recs, images


def edited(t, image=None, **params):
    """a copy of record t with the size of `image` and other parameters (the keywords of add_image_texture)"""
    out = copy_of(t)
    if image is not None:
        out.height, out.width = image.shape[:2]
    for k, v in params.items():
        setattr(out, k, WRAPS[v] if k == "wrap" else (int(bool(v)) if k in ("trilinear", "gamma") else v))
    return out


class WithTextures:
    """The builder's description carrying other texture records and texels, and / or other vertices and materials (all kept alive here)."""

    def __init__(self, builder, recs, images, verts=None, materials=None):
        self.builder = builder
        self.textures = (A.Texture * len(recs))(*[copy_of(t) for t in recs])
        parts, at = [], 0
        for t, g in zip(self.textures, images):
            assert g.shape == (t.height, t.width, 3) and g.dtype == np.float32
            t.texel_offset = at
            parts.append(np.ascontiguousarray(g).reshape(-1))
            at += g.size
        self.texels = np.concatenate(parts)
        self.verts = None if verts is None else np.ascontiguousarray(verts, np.float32)
        self.materials = None if materials is None else (A.Material * len(materials))(*materials)

    def desc(self):
        d = self.builder.desc()
        assert len(self.textures) == d.n_textures
        d.textures = C.cast(self.textures, C.POINTER(A.Texture))
        d.texels = self.texels.ctypes.data_as(C.POINTER(C.c_float))
        if self.verts is not None:
            assert self.verts.shape == (d.n_vertices, 3)
            d.vertices = self.verts.ctypes.data_as(C.POINTER(C.c_float))
        if self.materials is not None:
            assert len(self.materials) == d.n_materials
            d.materials = C.cast(self.materials, C.POINTER(A.Material))
        return d


def created(gx, b, recs, images, **kw):
    e = WithTextures(b, recs, images, **kw)
    s = gx.Scene(e.desc())
    s._keep = e
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_tables(a, b):
    ta, tb = a.texture_tables(), b.texture_tables()
    assert ta["records"].dtype == np.uint32 and ta["records"].shape == tb["records"].shape == (len(ta["texels"]), A.DTEXTURE_BYTES // 4)
    assert np.array_equal(ta["records"], tb["records"])
    assert len(ta["texels"]) == len(tb["texels"])
    for i, (xa, xb) in enumerate(zip(ta["texels"], tb["texels"])):
        assert xa.dtype == np.float32 and xa.shape == xb.shape
        bad = np.nonzero(bits(xa) != bits(xb))[0]
        assert bad.size == 0, f"texture {i}: {bad.size} of {xa.size} floats differ, first at {bad[:8].tolist()}"
    return ta


def tables_unchanged(scene, before):
    now = scene.texture_tables()
    assert np.array_equal(now["records"], before["records"])
    for x0, x1 in zip(before["texels"], now["texels"]):
        assert x0.shape == x1.shape and np.array_equal(bits(x0), bits(x1))


def picture(w, h, seed):
    """a smooth colourful image in [0.02, 0.98]: what the renders show"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3).astype(np.float32)
    img = np.stack([0.5 + 0.48 * np.sin(0.9 * x + 0.4 * y + ph[0]), 0.5 + 0.48 * np.cos(0.3 * x - 0.7 * y + ph[1]), 0.5 + 0.48 * np.sin(0.5 * (x + y) + ph[2])], -1)
    return np.ascontiguousarray(img, np.float32)


def specials(w, h, seed):
    """seeded texels with, spread over them, negatives, +-0, the two floats around the gamma branch's 0.04045f, values above 1 and a
    denormal (tables only, never rendered)"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.25, 1.5, (h, w, 3)).astype(np.float32)
    edge = np.float32(0.04045)
    vals = np.array([0.0, -0.0, edge, np.nextafter(edge, np.float32(1)), np.nextafter(edge, np.float32(0)), 1e-40, -1e-40, 7.5, 1.0, 0.03, -3.0, 0.05], np.float32)
    flat = img.reshape(-1)
    at = rng.permutation(flat.size)[:vals.size]
    flat[at] = vals[:at.size]
    return img


# ---------------------------------------------------------------- CPU
def test_entry_points_exported_and_declared(gx):
    lib = C.CDLL(gx.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gnxr.h")).read()
    for name in ("gnxr_scene_update_textures", "gnxr_scene_texture_tables"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES and f"int {name}(" in header
    assert gx.lib().gnxr_abi_version() == 5


def test_null_scene_is_invalid(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    rec = gx.Texture()
    rec.width, rec.height, rec.scale = 2, 2, 1.0
    d = np.ones(12, np.float32)
    assert gx.lib().gnxr_scene_update_textures(None, 0, 1, C.byref(rec), C.c_void_p(d.ctypes.data), None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_textures(None, 0, 1, C.byref(rec), None, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_textures(None, 0, 0, None, None, None) == ERR_INVALID
    n = C.c_int64(0)
    assert gx.lib().gnxr_scene_texture_tables(None, 0, 0, None, 0, C.byref(n)) == ERR_INVALID
    assert gx.lib().gnxr_scene_texture_tables(None, 1, 0, None, 0, C.byref(n)) == ERR_INVALID


def test_python_surface(gx):
    assert callable(gx.Scene.update_textures) and callable(gx.Scene.texture_tables)
    s = object.__new__(gx.Scene)
    s._h, s.device, s._env_light = None, 0, None
    s._textures = [gx.Texture(), gx.Texture()]
    ok = np.zeros((3, 4, 3), np.float32)
    on_device = torch.zeros((3, 4, 3), device="meta")   # a tensor that is no CUDA tensor on the scene's device
    for bad in ([[[0.0] * 3] * 4] * 3, np.zeros((3, 4, 3), np.float64), np.zeros((3, 4), np.float32), np.zeros((3, 4, 4), np.float32), np.zeros((0, 4, 3), np.float32),
                np.zeros(36, np.float32), "image", [ok, on_device], [ok, "image"], on_device, [ok, ok, ok]):
        with pytest.raises(ValueError):
            s.update_textures(bad)
    with pytest.raises(ValueError):
        s.update_textures(ok, first_texture=2)                  # past the list
    with pytest.raises(ValueError):
        s.update_textures([ok, ok], params=[dict(su=2.0)])      # one dict per image
    with pytest.raises(ValueError):
        s.update_textures(ok, params=dict(filter="ewa"))        # an unknown keyword
    with pytest.raises(ValueError):
        s.update_textures(ok, params=dict(wrap="mirror"))
    with pytest.raises(ValueError):
        s.update_textures()                                     # nothing to do
    assert s._textures[0].width == 0                            # (no refused call left a trace in the kept records)


# ---------------------------------------------------------------- GPU: the tables
@pytest.mark.gpu
@pytest.mark.parametrize("wrap", list(WRAPS))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_tables_equal_a_created_scene(gpu, shape, wrap):
    """The smallest shapes that reach each branch, under each wrap mode, gamma off (texture 0) and on (texture 1), scale 0.8: 4x4 a power
    of two (no resample), 1x1 one level (no pyramid), 8x2 levels that are 1 wide in one dimension only (2s + 1 falls outside: Black yields
    0, Clamp repeats, Repeat wraps), 5x3 both passes with taps off both edges, 1x7 and 6x1 one side a power of two, 33x17 pads to 64x32
    (the first level of the one-block tail is read from global memory), 100x60 pads to 128x64 (one per-level launch, then the tail)."""
    w, h = shape
    b = base(glass_sheet=False)
    recs0, _ = desc_textures(b)
    imgs = [specials(w, h, 11), specials(w, h, 12)]
    a = gpu.Scene(b)
    a.update_textures(imgs, params=[dict(wrap=wrap, gamma=False, scale=0.8), dict(wrap=wrap, gamma=True, scale=0.8)])
    recs = [edited(recs0[WALL], imgs[0], wrap=wrap, gamma=False, scale=0.8), edited(recs0[FLOOR], imgs[1], wrap=wrap, gamma=True, scale=0.8)]
    t = same_tables(a, created(gpu, b, recs, imgs))
    pw, ph = (w, h) if (w & (w - 1)) == 0 and (h & (h - 1)) == 0 else (1 << (w - 1).bit_length(), 1 << (h - 1).bit_length())
    n_levels = max(pw, ph).bit_length()
    n_texels = sum(max(1, pw >> i) * max(1, ph >> i) for i in range(n_levels))
    for i in (WALL, FLOOR):
        assert tuple(t["records"][i, [N_LEVELS, W0, H0]]) == (n_levels, pw, ph) and t["texels"][i].size == 4 * n_texels
    assert t["records"][WALL, OFFSET0] == 0 and t["records"][FLOOR, OFFSET0] == n_texels   # packed in index order, no padding
    if (pw, ph) == (w, h):   # level 0 without gamma is the flipped image times the scale
        assert np.array_equal(bits(t["texels"][WALL][:4 * w * h].reshape(h, w, 4)[..., :3]), bits(np.float32(0.8) * imgs[0][::-1]))


@pytest.mark.gpu
def test_gamma_sweep(gpu):
    """convertIn's inverse gamma on a stream of caller data: gx_pow (csrc/device_math.h) against the host's glibc powf.  One 1024 x 1024
    texture (a power of two: nothing but the convert kernel touches level 0), gamma on, scale 1; its texels are an even stride through
    every float of (0.04045, 1], a band up to 1e4 and the linear branch."""
    lo, hi = int(np.float32(0.04045).view(np.uint32)) + 1, int(np.float32(1.0).view(np.uint32))
    n = 1024 * 1024 * 3
    n_band, n_lin = 1 << 19, 1 << 18
    n_pow = n - n_band - n_lin
    sweep = np.linspace(lo, hi, n_pow).round().astype(np.uint32).view(np.float32)
    assert sweep[0] > np.float32(0.04045) and sweep[-1] == 1.0 and np.all(np.diff(sweep.view(np.uint32).astype(np.int64)) <= (hi - lo) // (n_pow - 1) + 1)
    band = np.geomspace(1.0, 1e4, n_band).astype(np.float32)
    lin = np.linspace(-0.5, 0.04045, n_lin).astype(np.float32)
    img = np.concatenate([sweep, band, lin]).reshape(1024, 1024, 3)
    b = base(glass_sheet=False)
    recs0, imgs0 = desc_textures(b)
    a = gpu.Scene(b)
    a.update_textures(img, params=dict(gamma=True, scale=1.0))
    fresh = created(gpu, b, [edited(recs0[WALL], img, gamma=True, scale=1.0), recs0[FLOOR]], [img, imgs0[FLOOR]])
    ta, tb = a.texture_tables(), fresh.texture_tables()
    la, lb = ta["texels"][WALL][:4 << 20].reshape(1024, 1024, 4)[::-1, :, :3].reshape(-1), tb["texels"][WALL][:4 << 20].reshape(1024, 1024, 4)[::-1, :, :3].reshape(-1)
    bad = np.nonzero(bits(la) != bits(lb))[0]
    src = img.reshape(-1)
    assert bad.size == 0, f"{bad.size} inputs differ, the first: " + ", ".join(f"{float(src[i])!r} ({int(bits(src[i:i + 1])[0]):#x}): {float(la[i])!r} != {float(lb[i])!r}" for i in bad[:8])
    assert np.array_equal(ta["records"], tb["records"])


@pytest.mark.gpu
def test_middle_of_three(gpu):
    """Three textures, the middle one replaced by one of another size: the neighbours' texels stay, the third one's offsets shift."""
    b = base(glass_sheet=False)
    third = picture(12, 20, 3)
    b.add_image_texture(third, wrap="black", scale=0.5)
    recs0, imgs0 = desc_textures(b)
    a = gpu.Scene(b)
    t0 = a.texture_tables()
    new = specials(37, 9, 5)
    a.update_textures(new, first_texture=1)
    recs = [recs0[0], edited(recs0[1], new), recs0[2]]
    t = same_tables(a, created(gpu, b, recs, [imgs0[0], new, imgs0[2]]))
    for i in (0, 2):
        assert np.array_equal(bits(t["texels"][i]), bits(t0["texels"][i]))
    assert np.array_equal(t["records"][0], t0["records"][0])
    shift = int(t["texels"][1].size // 4) - int(t0["texels"][1].size // 4)
    assert shift != 0 and np.array_equal(t["records"][2, OFFSET0:OFFSET0 + 16][:t["records"][2, N_LEVELS]].astype(np.int64),
                                         t0["records"][2, OFFSET0:OFFSET0 + 16][:t0["records"][2, N_LEVELS]].astype(np.int64) + shift)


@pytest.mark.gpu
def test_size_change_and_back(gpu):
    b = base()
    recs0, imgs0 = desc_textures(b)
    a, initial = gpu.Scene(b), gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    integ.Render(a, 16, 12, 1)
    small = picture(7, 5, 2)
    a.update_textures(small)
    fresh = created(gpu, b, [edited(recs0[WALL], small), recs0[FLOOR]], [small, imgs0[FLOOR]])
    same_tables(a, fresh)
    same_render(gpu, integ, a, fresh, W, H, SPP)
    a.update_textures(imgs0[WALL])
    same_tables(a, initial)
    same_render(gpu, integ, a, initial, W, H, SPP)


@pytest.mark.gpu
def test_device_memory_source(gpu):
    """The image as a tensor produced on a side stream by a kernel queued just before the call (the stream is passed: the read is ordered
    after that kernel), then a view that starts 4 bytes into its storage."""
    b = base()
    recs0, _ = desc_textures(b)
    x, y = picture(45, 31, 5), picture(45, 31, 7)
    g = x * np.float32(0.5) + y * np.float32(0.25)
    params = dict(gamma=True, scale=0.9, wrap="clamp")
    host = gpu.Scene(b)
    host.update_textures(g, params=params)
    a = gpu.Scene(b)
    tx, ty = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = tx * 0.5 + ty * 0.25
    a.update_textures(t, params=params, stream=st)
    assert np.array_equal(bits(t.cpu().numpy()), bits(g))
    same_tables(a, host)
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), a, host, W, H, SPP)
    big = torch.zeros(y.size + 5, device="cuda:0")
    view = big[1:1 + y.size].view(31, 45, 3)
    view.copy_(torch.from_numpy(y))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    a.update_textures([view, t], first_texture=0)      # two device images: one call each
    host.update_textures([y, g], first_texture=0)
    t1 = same_tables(a, host)
    with pytest.raises(ValueError):
        a.update_textures(t.double())
    with pytest.raises(ValueError):
        a.update_textures(t.permute(1, 0, 2))
    with pytest.raises(ValueError):
        a.update_textures([t, y])
    tables_unchanged(a, t1)


@pytest.mark.gpu
def test_parameters_only(gpu):
    """images=None: the mapping, max_aniso and trilinear change, the texels stay; a changed wrap, gamma, scale or size is refused."""
    b = base()
    recs0, imgs0 = desc_textures(b)
    a = gpu.Scene(b)
    integ = gpu.WhittedIntegrator(5)
    img0, _ = integ.Render(a, W, H, SPP)
    before = a.texture_tables()
    p_wall, p_floor = dict(su=2.0, sv=1.5, du=0.3, dv=-0.2, max_aniso=4.0), dict(trilinear=False, su=2.5)
    a.update_textures(params=[p_wall, p_floor])
    t = a.texture_tables()
    for i in (WALL, FLOOR):
        assert np.array_equal(bits(t["texels"][i]), bits(before["texels"][i])) and not np.array_equal(t["records"][i], before["records"][i])
    fresh = created(gpu, b, [edited(recs0[WALL], **p_wall), edited(recs0[FLOOR], **p_floor)], imgs0)
    same_tables(a, fresh)
    assert not biteq(same_render(gpu, integ, a, fresh, W, H, SPP), img0)
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), a, fresh, W, H, SPP)
    now = a.texture_tables()
    for bad in (dict(wrap="black"), dict(gamma=True), dict(scale=0.5)):
        with pytest.raises(gpu.GnxrError, match="send the texels"):
            a.update_textures(params=bad)
    call = gpu.lib().gnxr_scene_update_textures
    cur = edited(recs0[WALL], **p_wall)
    for size in (dict(width=cur.width + 1), dict(height=cur.height - 1)):
        assert call(a._h, WALL, 1, (A.Texture * 1)(edited(cur, **size)), None, None) == ERR_INVALID
    tables_unchanged(a, now)
    # after a texel edit has repacked the buffer, parameters of the other texture
    small = picture(7, 5, 2)
    a.update_textures(small)
    a.update_textures(params=dict(su=1.0, sv=1.0), first_texture=FLOOR)
    fresh = created(gpu, b, [edited(cur, small), edited(recs0[FLOOR], trilinear=False, su=1.0, sv=1.0)], [small, imgs0[FLOOR]])
    same_tables(a, fresh)
    same_render(gpu, integ, a, fresh, W, H, SPP)


# ---------------------------------------------------------------- GPU: results
def edit_both(b):
    """one edit of both textures: other images at other sizes, other filters and wrap modes"""
    recs0, _ = desc_textures(b)
    imgs = [picture(50, 36, 8), picture(21, 64, 9)]
    params = [dict(wrap="clamp", su=2.0, sv=2.0, gamma=True, scale=0.9), dict(wrap="repeat", trilinear=False, max_aniso=4.0, gamma=False, scale=1.0)]
    return imgs, params, [edited(r, g, **p) for r, g, p in zip(recs0, imgs, params)]


@pytest.mark.gpu
def test_results_equal_a_created_scene(gpu):
    """One edit, then everything a caller can ask of the handle."""
    b = base(uv_quads=True)
    imgs, params, recs = edit_both(b)
    a = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = path.Render(a, W, H, SPP)
    rays, wi, u = probes(512, 32)
    diffs = synthetic_differentials(rays, 20)
    bsdf0 = dbsdf(a, rays, wi, u, 31, diffs=diffs)
    a.update_textures(imgs, params=params)
    fresh = created(gpu, b, recs, imgs)
    same_tables(a, fresh)
    integrators = (path, gpu.VolPathIntegrator(5, 1.0, "spatial"), gpu.WhittedIntegrator(5), gpu.DirectLightingIntegrator("all", 5))
    for integ in integrators:
        img = same_render(gpu, integ, a, fresh, W, H, SPP)
        if integ is path:
            assert not biteq(img, before)
    # gnxr_bsdf_device, without and with ray differentials, on rays of which many hit the textured walls
    for d in (None, diffs):
        ga, gb = dbsdf(a, rays, wi, u, 31, diffs=d), dbsdf(fresh, rays, wi, u, 31, diffs=d)
        assert biteq(ga, gb)
    assert not biteq(dbsdf(a, rays, wi, u, 31, diffs=diffs), bsdf0)
    # the albedo channel reads the Kd texture at the first hit
    fa, _ = path.RenderAOV(a, W, H, SPP, channels=("albedo",))
    fb, _ = path.RenderAOV(fresh, W, H, SPP, channels=("albedo",))
    torch.cuda.synchronize()
    assert torch.equal(fa["albedo"].view(torch.int32), fb["albedo"].view(torch.int32)) and bool(fa["albedo"].any())
    cams = [gpu.camera(eye=(0.3, 0.2, 4.8), look=(0.0, -0.5, 0.0), fov=50.0), gpu.camera(eye=(1.5, 1.0, 3.0), look=(-0.5, -2.0, -1.0), fov=70.0)]
    for integ in (path, integrators[2], integrators[3]):
        va, sa = integ.RenderViews(a, cams, 24, 20, 2)
        vb, sb = integ.RenderViews(fresh, cams, 24, 20, 2)
        torch.cuda.synchronize()
        assert torch.equal(va.view(torch.int32), vb.view(torch.int32)) and bool(va.any())
        assert (sa["rays_closest"], sa["rays_any"]) == (sb["rays_closest"], sb["rays_any"])
    # gnxr_li_device (Path: the other integrators need camera differentials on a textured scene)
    from test_li_device import cam_batch
    r2, s2 = cam_batch(cams[0], 2, -1, w=24, h=20)
    la, lb = path.Li(a, r2, s2, 24, 20, 2)[0], path.Li(fresh, r2, s2, 24, 20, 2)[0]
    torch.cuda.synchronize()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and bool(la.any())


@pytest.mark.gpu
def test_composes_with_the_other_edits(gpu):
    """update_textures, then a refit and a rebuild, then a material edit that points the floor's Kd at the other (edited) texture; and the
    texture edit last."""
    b = base()
    imgs, params, recs = edit_both(b)
    nv = int(emissive_vertices(b).min())   # the walls and the glass sheet; the light's quad, added last, stays
    v2 = deform(vertices(b), nv, seed=4, amount=0.01, shift=(0.02, -0.01, 0.03))
    mats = desc_materials(gpu, b)
    floor = next(i for i, m in enumerate(mats) if m.kd_texture == FLOOR + 1)
    mats[floor].kd_texture = WALL + 1
    whitted, path = gpu.WhittedIntegrator(5), gpu.PathIntegrator(5, 1.0, "spatial")

    def others(s):
        s.update_vertices(v2[:nv])
        s.rebuild_bvh()
        s.update_materials(mats[floor:floor + 1], first_material=floor)

    scenes_ = []
    for textures_first in (True, False):
        s = gpu.Scene(b)
        path.Render(s, W, H, SPP)
        if textures_first:
            s.update_textures(imgs, params=params)
        others(s)
        if not textures_first:
            s.update_textures(imgs, params=params)
        scenes_.append(s)
    b.set_bvh_split_method("hlbvh")
    fresh = created(gpu, b, recs, imgs, verts=v2, materials=mats)
    for s in scenes_:
        same_tables(s, fresh)
        same_render(gpu, path, s, fresh, W, H, SPP)
        same_render(gpu, whitted, s, fresh, W, H, SPP)


@pytest.mark.gpu
def test_refusals_leave_the_scene_as_it_was(gpu):
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    d12 = np.full(12, 0.5, np.float32)
    p12 = C.c_void_p(d12.ctypes.data)
    call = gpu.lib().gnxr_scene_update_textures
    # a scene without textures
    s0 = gpu.Scene(scenes.cornell())
    img0, _ = integ.Render(s0, W, H, SPP)
    rec = gpu.Texture()
    rec.width, rec.height, rec.scale = 2, 2, 1.0
    assert call(s0._h, 0, 1, (A.Texture * 1)(rec), p12, None) == ERR_UNSUPPORTED
    assert call(s0._h, 0, 1, (A.Texture * 1)(rec), None, None) == ERR_UNSUPPORTED
    t0 = s0.texture_tables()
    assert t0["records"].shape == (0, A.DTEXTURE_BYTES // 4) and t0["texels"] == []
    assert biteq(integ.Render(s0, W, H, SPP)[0], img0)
    # a scene with two
    b = base()
    recs0, imgs0 = desc_textures(b)
    scene = gpu.Scene(b)
    before, _ = integ.Render(scene, W, H, SPP)
    tables = scene.texture_tables()

    def unchanged():
        tables_unchanged(scene, tables)
        assert biteq(integ.Render(scene, W, H, SPP)[0], before)

    ok = edited(recs0[WALL], d12.reshape(2, 2, 3))
    one = lambda t: (A.Texture * 1)(t)
    assert call(scene._h, 0, 1, None, p12, None) == ERR_INVALID                        # null textures
    for first, n in ((-1, 1), (2, 1), (1, 2), (0, 3), (0, -1)):                          # ranges outside the two textures
        assert call(scene._h, first, n, (A.Texture * 3)(ok, ok, ok), p12, None) == ERR_INVALID, (first, n)
    unchanged()
    for size in (dict(width=0), dict(height=0), dict(width=-4), dict(height=-1)):
        assert call(scene._h, 0, 1, one(edited(ok, **size)), p12, None) == ERR_INVALID, size
    for wrap in (-1, 3):
        r = edited(ok)
        r.wrap = wrap
        assert call(scene._h, 0, 1, one(r), p12, None) == ERR_INVALID, wrap
    for size in (dict(width=32769, height=1), dict(width=1, height=32769), dict(width=(1 << 31) - 1, height=1)):   # a 17th MIP level
        assert call(scene._h, 0, 1, one(edited(ok, **size)), p12, None) == ERR_INVALID, size
    for off in (-1, 1 << 60, (1 << 63) - 1):                                             # an offset that is negative, or 2^60 or more
        assert call(scene._h, 0, 1, one(edited(ok, texel_offset=off)), p12, None) == ERR_INVALID, off
    unchanged()
    # texels == NULL: what is baked into the texels must stay
    for change in (dict(width=2, height=2), dict(wrap="black"), dict(gamma=True), dict(scale=0.25)):
        assert call(scene._h, 0, 1, one(edited(recs0[WALL], **change)), None, None) == ERR_INVALID, change
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.update_textures(params=dict(scale=2.0))
    unchanged()
    # a packed total of 2^31 texels or more (one 32768 x 32768 pyramid stays below it); nothing of the small array is read
    huge = edited(ok, width=32768, height=32768)
    assert call(scene._h, 0, 2, (A.Texture * 2)(huge, huge), p12, None) == ERR_INVALID
    unchanged()
    # a valid first record, then one that is not: nothing of the first may have been applied
    assert call(scene._h, 0, 2, (A.Texture * 2)(ok, edited(ok, width=0)), p12, None) == ERR_INVALID
    assert call(scene._h, 1, 2, (A.Texture * 2)(ok, ok), p12, None) == ERR_INVALID       # the second record lies past the list
    unchanged()
    if torch.cuda.device_count() >= 2:                                                   # texels in another device's memory
        far = torch.full((12,), 0.5, device="cuda:1")
        torch.cuda.synchronize()
        assert call(scene._h, 0, 1, one(ok), C.c_void_p(far.data_ptr()), None) == ERR_INVALID
        unchanged()
    # the hook's own refusals
    n = C.c_int64(0)
    hook = gpu.lib().gnxr_scene_texture_tables
    assert hook(scene._h, 2, 0, None, 0, C.byref(n)) == ERR_INVALID and hook(scene._h, -1, 0, None, 0, C.byref(n)) == ERR_INVALID
    assert hook(scene._h, 1, 2, None, 0, C.byref(n)) == ERR_INVALID and hook(scene._h, 1, -1, None, 0, C.byref(n)) == ERR_INVALID
    assert hook(scene._h, 0, 0, None, 0, None) == ERR_INVALID
    assert hook(scene._h, 0, 99, None, 0, C.byref(n)) == 0 and n.value == 2 * A.DTEXTURE_BYTES   # which 0 ignores `texture`
    # n_textures == 0 is a no-op, and the handle still takes an edit
    assert call(scene._h, 1, 0, None, None, None) == 0
    unchanged()
    g = d12.reshape(2, 2, 3)
    scene.update_textures(g)
    same_tables(scene, created(gpu, b, [ok, recs0[FLOOR]], [g, imgs0[FLOOR]]))


@pytest.mark.gpu
def test_on_replicas(gpu):
    """Device 0 listed twice: both copies take the edit (rows are dealt over the replicas), from host and from device memory."""
    b = base()
    imgs, params, recs = edit_both(b)
    recs0, imgs0 = desc_textures(b)
    p_only = dict(su=3.0, dv=0.5)
    integ = gpu.WhittedIntegrator(5)
    single = created(gpu, b, recs, imgs)
    remapped = created(gpu, b, [edited(recs[WALL], **p_only), recs[FLOOR]], imgs)
    t = torch.from_numpy(imgs[WALL]).to("cuda:0")
    torch.cuda.synchronize()
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        integ.Render(multi, 16, 12, 1)
        multi.update_textures(imgs, params=params)
        same_tables(multi, single)
        same_render(gpu, integ, multi, single, W, H, SPP)
        multi.update_textures(params=p_only)
        same_render(gpu, integ, multi, remapped, W, H, SPP)
        multi.update_textures(imgs0[WALL], params=dict(su=1.0, dv=0.0))
        multi.update_textures(t, params=params[WALL])      # the replica takes a device-memory image by peer copy
        same_tables(multi, single)
        same_render(gpu, integ, multi, single, W, H, SPP)
    finally:
        gpu.init(0)
