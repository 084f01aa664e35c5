"""gnxr_scene_update_media: density grids and medium records of a live scene replaced on the device (csrc/media_kernel.hip.h,
csrc/api_media.hip.h).

Every comparison is bit for bit and against gnxr_scene_create, whose host code (compile_scene / compile_medium, csrc/scene_compile.cpp) is
the yardstick: scene A is created from the base description and edited, scene B is created from a description carrying the new records
and grids, and the two must hold the same tables (Scene.media_tables: every word of the device's medium records, 1 / the grid's maximum
among them, and the grids' floats) and give the same results.  The base scene is the "vol_synth" scene of the parity tests: the Cornell
box, a 24 x 24 x 12 GridDensityMedium in one null-material box (medium 0) and a HomogeneousMedium in another (medium 1); renders are
48 x 40 at 4 spp.  No tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import ROOT
from gnxraytracer_amd import _abi as A
from test_li_device import cam_batch
from test_material_update import desc_materials
from test_scene_update import biteq, same_render, vertices

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W, H, SPP = 48, 40, 4
GRID, HOM = 0, 1                      # the media of scenes.volume_cornell
GRID_LO, GRID_HI = (-1.6, -2.4, -1.2), (0.2, -0.6, 0.4)   # its grid's box
INV_MAX = 28                          # word of a medium record that holds 1 / the grid's maximum (DMedium::inv_max_density)
COUNTERS = ("rays_closest", "rays_any", "rays_closest_nee", "camera_samples", "media_segments", "media_steps")
INSIDE = dict(eye=(-0.7, -1.5, -0.4), look=(0.4, 0.2, 3.0), fov=70.0)   # a camera inside the grid's box
OUTSIDE = dict(eye=(0.3, 0.2, 4.8), look=(0.0, -0.5, 0.0), fov=50.0)


# ---------------------------------------------------------------- helpers
def base():
    return scenes.volume_cornell(sigma_a=(0.5,) * 3, sigma_s=(3.5,) * 3, g_grid=0.3)


def copy_of(m):
    out = A.Medium()
    C.memmove(C.byref(out), C.byref(m), C.sizeof(A.Medium))
    return out


def desc_media(b):
    """copies of the description's medium records, and per medium its grid as (nz, ny, nx) (None for a homogeneous one)"""
    d = b.desc()
    media, grids = [], []
    for i in range(d.n_media):
        m = copy_of(d.media[i])
        media.append(m)
        n = m.nx * m.ny * m.nz
        grids.append(np.ctypeslib.as_array(d.grid_density, shape=(m.density_offset + n,))[m.density_offset:].copy().reshape(m.nz, m.ny, m.nx) if m.type == A.MEDIUM_GRID else None)
    return media, grids


def edited(m, grid=None, **fields):
    """a copy of record m with other fields; grid: it becomes a GRID record of that (nz, ny, nx) array's resolution"""
    out = copy_of(m)
    if grid is not None:
        out.type = A.MEDIUM_GRID
        out.nz, out.ny, out.nx = grid.shape
    for k, v in fields.items():
        if k in ("sigma_a", "sigma_s", "medium_to_world"):
            getattr(out, k)[:] = [float(x) for x in np.asarray(v, np.float32).reshape(-1)]
        else:
            setattr(out, k, v)
    return out


class WithMedia:
    """The builder's description carrying other medium records and grids, and / or other vertices and materials (all kept alive here)."""

    def __init__(self, builder, media, grids, verts=None, materials=None):
        self.builder = builder
        self.media = (A.Medium * len(media))(*[copy_of(m) for m in media])
        parts, at = [np.zeros(0, np.float32)], 0
        for m, g in zip(self.media, grids):
            if m.type == A.MEDIUM_GRID:
                assert g.shape == (m.nz, m.ny, m.nx)
                m.density_offset = at
                parts.append(np.ascontiguousarray(g, np.float32).reshape(-1))
                at += g.size
        self.density = np.concatenate(parts)
        self.verts = None if verts is None else np.ascontiguousarray(verts, np.float32)
        self.materials = None if materials is None else (A.Material * len(materials))(*materials)

    def desc(self):
        d = self.builder.desc()
        assert len(self.media) == d.n_media
        d.media = C.cast(self.media, C.POINTER(A.Medium))
        d.grid_density = self.density.ctypes.data_as(C.POINTER(C.c_float)) if self.density.size else None
        if self.verts is not None:
            assert self.verts.shape == (d.n_vertices, 3)
            d.vertices = self.verts.ctypes.data_as(C.POINTER(C.c_float))
        if self.materials is not None:
            assert len(self.materials) == d.n_materials
            d.materials = C.cast(self.materials, C.POINTER(A.Material))
        return d


def created(gx, b, media, grids, **kw):
    e = WithMedia(b, media, grids, **kw)
    s = gx.Scene(e.desc())
    s._keep = e
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_tables(a, b):
    ta, tb = a.media_tables(), b.media_tables()
    assert ta["records"].dtype == np.uint32 and ta["records"].shape == tb["records"].shape == (len(ta["grids"]), A.DMEDIUM_BYTES // 4)
    assert np.array_equal(ta["records"][:, INV_MAX], tb["records"][:, INV_MAX])
    assert np.array_equal(ta["records"], tb["records"])
    assert len(ta["grids"]) == len(tb["grids"])
    for ga, gb in zip(ta["grids"], tb["grids"]):
        assert ga.dtype == np.float32 and ga.shape == gb.shape and np.array_equal(bits(ga), bits(gb))
    return ta


def tables_unchanged(scene, before):
    now = scene.media_tables()
    assert np.array_equal(now["records"], before["records"])
    for g0, g1 in zip(before["grids"], now["grids"]):
        assert g0.shape == g1.shape and np.array_equal(bits(g0), bits(g1))


def same_result(gx, integ, s1, s2, w=W, h=H, spp=SPP):
    """image and every ray counter, media_segments included"""
    i1, st1 = integ.Render(s1, w, h, spp)
    i2, st2 = integ.Render(s2, w, h, spp)
    assert {k: st1[k] for k in COUNTERS} == {k: st2[k] for k in COUNTERS}
    assert biteq(i1[..., :3], i2[..., :3]) and i1[..., :3].any()
    return i1, st1


def fold_max(d):
    """GridDensityMedium.h:28-31: m = 0; m = std::max(m, d[k]) -- NaNs and negative values never win"""
    d = d.reshape(-1)
    d = d[~np.isnan(d)]
    return np.float32(max(np.float32(0), d.max())) if d.size else np.float32(0)


def smoke(nx, ny, nz, seed):
    return scenes.synthetic_density(nx, ny, nz, seed)


def peak(shape, at):
    d = np.full(shape, 0.25, np.float32)
    d.reshape(-1)[at] = 2.0
    return d


def nan_and_negative():
    d = smoke(9, 7, 5, 4) - np.float32(0.3)
    d.reshape(-1)[[0, 17, 100, -1]] = np.nan
    d.reshape(-1)[[1, 50]] = -np.inf
    return d


def head_of_specials():
    """a NaN, -0 and a negative value where the scalar head of a 4-byte aligned source reads them; tables only, never rendered"""
    d = smoke(6, 5, 4, 6)
    d.reshape(-1)[:3] = (np.nan, -0.0, -1.0)
    return d


M2W = np.array([[1.7, 0, 0, -1.5], [0, 1.9, 0, -2.4], [0, 0, 1.5, -1.1], [0, 0, 0, 1]], np.float32)   # another box for the grid

# name -> the (nz, ny, nx) grids sent in ONE call, for media 0, 1, ...: the smallest shapes at which each branch of the kernel can go wrong
GRIDS = {
    "1x1x1": lambda: [np.full((1, 1, 1), 0.75, np.float32)],           # the scalar tail alone
    "5x3x7": lambda: [smoke(5, 3, 7, 1)],                              # 105 values: less than two waves, no multiple of 4
    "24x24x12": lambda: [smoke(24, 24, 12, 2)],                        # the base resolution, other values
    "41x43x41": lambda: [smoke(41, 43, 41, 3)],                        # 72 283 values: many blocks, odd tail
    "max_first": lambda: [peak((7, 6, 11), 0)],
    "max_last": lambda: [peak((7, 6, 11), -1)],
    "nan_negative": lambda: [nan_and_negative()],                      # tables only, never rendered
    "two_packed": lambda: [smoke(5, 3, 7, 1), head_of_specials()],     # the second grid starts at float 105 of the packed array: a 4-byte aligned source
    "negative_zero": lambda: [np.full((3, 2, 5), -0.0, np.float32)],   # maximum +0, 1 / maximum +inf; tables only, never rendered
}


# ---------------------------------------------------------------- CPU
def test_entry_points_exported_and_declared(gx):
    lib = C.CDLL(gx.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gnxr.h")).read()
    for name in ("gnxr_scene_update_media", "gnxr_scene_media_tables"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES and f"int {name}(" in header
    assert gx.lib().gnxr_abi_version() == 5


def test_null_scene_is_invalid(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    rec = gx.Medium()
    rec.type, rec.nx, rec.ny, rec.nz = A.MEDIUM_GRID, 2, 2, 2
    d = np.ones(8, np.float32)
    assert gx.lib().gnxr_scene_update_media(None, 0, 1, C.byref(rec), C.c_void_p(d.ctypes.data), None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_media(None, 0, 1, C.byref(rec), None, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_media(None, 0, 0, None, None, None) == ERR_INVALID
    n = C.c_int64(0)
    assert gx.lib().gnxr_scene_media_tables(None, 0, 0, None, 0, C.byref(n)) == ERR_INVALID
    assert gx.lib().gnxr_scene_media_tables(None, 1, 0, None, 0, C.byref(n)) == ERR_INVALID


def test_python_surface(gx):
    assert callable(gx.Scene.update_media) and callable(gx.Scene.media_tables)
    s = object.__new__(gx.Scene)
    s._h, s.device, s._env_light = None, 0, None
    rec = gx.Medium()
    rec.type, rec.nx, rec.ny, rec.nz = A.MEDIUM_GRID, 4, 3, 2
    hom = gx.Medium()
    hom.type = A.MEDIUM_HOMOGENEOUS
    ok = np.zeros((2, 3, 4), np.float32)
    for bad in ([[[0.0] * 4] * 3] * 2, np.zeros((2, 3, 4), np.float64), np.zeros((4, 3, 2), np.float32), np.zeros(23, np.float32), np.zeros((2, 3, 4, 1), np.float32), "grid",
                [ok, ok], []):
        with pytest.raises(ValueError):
            s.update_media(rec, bad)
    with pytest.raises(ValueError):
        s.update_media([rec, hom, rec], [ok])       # one array per GRID record
    with pytest.raises(ValueError):
        s.update_media(hom, ok)                     # ... and none for a HOMOGENEOUS one
    with pytest.raises(ValueError):
        s.update_media(["medium"], ok)


# ---------------------------------------------------------------- GPU: the tables
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRIDS))
def test_tables_equal_a_created_scene(gpu, name):
    grids = GRIDS[name]()
    b = base()
    media, grids0 = desc_media(b)
    a = gpu.Scene(b)
    before = a.media_tables()
    assert before["grids"][GRID].size == 24 * 24 * 12 and before["grids"][HOM].size == 0
    recs = [edited(media[i], g, g=0.1 * (i + 1), medium_to_world=M2W) for i, g in enumerate(grids)]
    a.update_media(recs, grids if len(grids) > 1 else grids[0])
    new_media, new_grids = recs + media[len(recs):], grids + grids0[len(grids):]
    t = same_tables(a, created(gpu, b, new_media, new_grids))
    for i, g in enumerate(grids):
        assert np.array_equal(bits(t["grids"][i]), bits(g.reshape(-1)))
        with np.errstate(divide="ignore"):
            assert t["records"][i, INV_MAX] == bits(np.float32(1) / fold_max(g))
    if name == "negative_zero":
        assert t["records"][GRID, INV_MAX] == 0x7f800000   # +inf, not -inf
    if len(grids) == 1:
        assert np.array_equal(t["records"][HOM], before["records"][HOM])


# ---------------------------------------------------------------- GPU: results
@pytest.mark.gpu
def test_results_equal_a_created_scene(gpu):
    """One edit -- another grid at another resolution, other coefficients, another medium_to_world -- then everything a caller can ask
    of the handle."""
    b = base()
    media, grids0 = desc_media(b)
    g = smoke(20, 16, 10, 5)
    rec = edited(media[GRID], g, sigma_a=(0.4,) * 3, sigma_s=(3.0,) * 3, g=-0.2, medium_to_world=M2W)
    a = gpu.Scene(b)
    vol, path = gpu.VolPathIntegrator(5, 1.0, "spatial"), gpu.PathIntegrator(5, 1.0, "spatial")
    before, st0 = vol.Render(a, W, H, SPP)
    a.update_media(rec, g)
    fresh = created(gpu, b, [rec, media[HOM]], [g, None])
    same_tables(a, fresh)
    img, st = same_result(gpu, vol, a, fresh)
    assert not biteq(img, before) and st["media_segments"] > 0
    same_result(gpu, path, a, fresh)
    # gnxr_li_device on camera rays that start in the medium
    cam = gpu.camera(**INSIDE)
    rays, samples = cam_batch(cam, 2, GRID, w=24, h=20)
    la, lb = vol.Li(a, rays, samples, 24, 20, 2)[0], vol.Li(fresh, rays, samples, 24, 20, 2)[0]
    torch.cuda.synchronize()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and bool(la.any())
    # views, one of them inside the medium
    cams = [gpu.camera(**INSIDE), gpu.camera(**OUTSIDE)]
    va, sa = vol.RenderViews(a, cams, 24, 20, 2, media=[GRID, -1])
    vb, sb = vol.RenderViews(fresh, cams, 24, 20, 2, media=[GRID, -1])
    torch.cuda.synchronize()
    assert torch.equal(va.view(torch.int32), vb.view(torch.int32)) and {k: sa[k] for k in COUNTERS} == {k: sb[k] for k in COUNTERS}
    fa, _ = path.RenderAOV(a, W, H, SPP, channels=("depth",))
    fb, _ = path.RenderAOV(fresh, W, H, SPP, channels=("depth",))
    assert torch.equal(fa["depth"].view(torch.int32), fb["depth"].view(torch.int32))


@pytest.mark.gpu
def test_against_the_oracle(gpu):
    """The edited scene against the CPU restatement of the reference directly: image and ray counts."""
    b = base()
    media, _ = desc_media(b)
    g = smoke(20, 16, 10, 5)
    rec = edited(media[GRID], g, sigma_a=(0.4,) * 3, sigma_s=(3.0,) * 3, g=-0.2)
    a = gpu.Scene(b)
    a.update_media(rec, g)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    img, st = vol.Render(a, 32, 32, 2)
    oimg, ost = ol.OracleScene(WithMedia(b, [rec, media[HOM]], [g, None])).render(vol, 32, 32, 2)
    assert (st["rays_closest"], st["rays_any"]) == (ost["rays_closest"], ost["rays_any"])
    assert biteq(img[..., :3], oimg[..., :3]) and img[..., :3].any()


@pytest.mark.gpu
def test_device_memory_source(gpu):
    """The grid as a tensor produced on a side stream by a kernel queued just before the call (the stream is passed: the read is ordered
    after that kernel), then a view that starts 4 bytes into its storage."""
    b = base()
    media, _ = desc_media(b)
    x, y = smoke(20, 16, 10, 5), smoke(20, 16, 10, 7)
    g = x * np.float32(0.5) + y
    rec = edited(media[GRID], g, g=0.1)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    host = gpu.Scene(b)
    host.update_media(rec, g)
    a = gpu.Scene(b)
    tx, ty = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = tx * 0.5 + ty
    a.update_media(rec, t, stream=st)
    t0 = same_tables(a, host)
    assert np.array_equal(bits(t0["grids"][GRID]), bits(g.reshape(-1)))
    same_result(gpu, vol, a, host)
    # a source that is only 4-byte aligned: element 1 of a larger tensor
    big = torch.zeros(g.size + 5, device="cuda:0")
    view = big[1:1 + g.size]
    view.copy_(torch.from_numpy(y.reshape(-1)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    rec_y = edited(media[GRID], y, g=0.1)
    a.update_media(rec_y, view)
    host.update_media(rec_y, y.reshape(-1))   # (flat arrays are taken too)
    t1 = same_tables(a, host)
    assert np.array_equal(bits(t1["grids"][GRID]), bits(y.reshape(-1)))
    with pytest.raises(ValueError):
        a.update_media(rec, t.double())
    with pytest.raises(ValueError):
        a.update_media(rec, t.permute(2, 1, 0))   # neither the shape nor contiguous
    with pytest.raises(ValueError):
        a.update_media(rec, t.cpu())
    tables_unchanged(a, t1)


@pytest.mark.gpu
def test_resolution_and_type_changes(gpu):
    """24 x 24 x 12 -> 7 x 5 x 3 -> 24 x 24 x 12; GRID -> HOMOGENEOUS -> GRID; the homogeneous medium -> GRID: every state equals its
    created twin and the last one the initial scene."""
    b = base()
    media, grids0 = desc_media(b)
    a, initial = gpu.Scene(b), gpu.Scene(b)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    vol.Render(a, 16, 12, 1)
    small = smoke(7, 5, 3, 8)
    thin = edited(media[GRID], type=A.MEDIUM_HOMOGENEOUS, sigma_a=(0.3, 0.2, 0.1), sigma_s=(0.8, 0.9, 1.0), g=0.4)
    other = smoke(6, 5, 4, 6)
    states = [
        ([edited(media[GRID], small)], [small], 0),                      # a smaller grid
        ([media[GRID]], [grids0[GRID]], 0),                              # ... and back
        ([thin], [], 0),                                                 # the grid medium turns homogeneous (its grid leaves with the next repack)
        ([edited(media[HOM], other, sigma_a=(0.2,) * 3, sigma_s=(2.0,) * 3)], [other], 1),   # the homogeneous medium takes a grid
        ([media[GRID], media[HOM]], [grids0[GRID]], 0),                  # everything back, in one call
    ]
    now_media, now_grids = list(media), list(grids0)
    for recs, gs, first in states:
        a.update_media(recs, gs if gs else None, first_medium=first)
        gi = iter(gs)
        for k, r in enumerate(recs):
            now_media[first + k] = r
            now_grids[first + k] = next(gi) if r.type == A.MEDIUM_GRID else None
        fresh = created(gpu, b, now_media, now_grids)
        same_tables(a, fresh)
        same_result(gpu, vol, a, fresh)
    same_tables(a, initial)
    same_result(gpu, vol, a, initial)


@pytest.mark.gpu
def test_coefficients_only(gpu):
    """density=None: sigma_s, g and medium_to_world change, the grid's floats and 1 / its maximum stay."""
    b = base()
    media, grids0 = desc_media(b)
    a = gpu.Scene(b)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    img0, _ = vol.Render(a, W, H, SPP)
    before = a.media_tables()
    rec = edited(media[GRID], sigma_s=(2.5, 2.5, 2.5), g=-0.3, medium_to_world=M2W, density_offset=12345)   # (the offset is ignored)
    a.update_media(rec)
    t = a.media_tables()
    assert np.array_equal(bits(t["grids"][GRID]), bits(before["grids"][GRID])) and t["records"][GRID, INV_MAX] == before["records"][GRID, INV_MAX]
    assert not np.array_equal(t["records"][GRID], before["records"][GRID]) and np.array_equal(t["records"][HOM], before["records"][HOM])
    fresh = created(gpu, b, [rec, media[HOM]], grids0)
    same_tables(a, fresh)
    img, _ = same_result(gpu, vol, a, fresh)
    assert not biteq(img, img0)
    # the homogeneous medium's coefficients, after the grid has been repacked by a grid edit
    g = smoke(7, 5, 3, 8)
    a.update_media(edited(rec, g), g)
    hom = edited(media[HOM], sigma_a=(1.0, 1.2, 1.4), sigma_s=(0.7,) * 3, g=0.1)
    a.update_media(hom, first_medium=HOM)
    fresh = created(gpu, b, [edited(rec, g), hom], [g, None])
    same_tables(a, fresh)
    same_result(gpu, vol, a, fresh)


@pytest.mark.gpu
def test_composes_with_the_other_edits(gpu):
    """update_media with a refit of the medium's boundary box, a rebuild, a camera inside the medium and a material edit, the media edit
    first and last; path state reserved before the edits is still the one in use."""
    b = base()
    media, grids0 = desc_media(b)
    g = smoke(20, 16, 10, 5)
    rec = edited(media[GRID], g, sigma_a=(0.4,) * 3, sigma_s=(3.0,) * 3, medium_to_world=M2W)
    first_box = scenes.cornell().desc().n_vertices       # the grid's box follows the Cornell box in the vertex array
    n_box = len(scenes.box_mesh(GRID_LO, GRID_HI)[0])
    v2 = vertices(b)
    v2[first_box:first_box + n_box] = v2[first_box:first_box + n_box] * np.float32(1.05) + np.array([0.05, 0.0, -0.1], np.float32)
    mats = desc_materials(gpu, b)
    mats[0] = gpu.material(type=A.MAT_MATTE, kd=(0.2, 0.6, 0.3), sigma=20.0)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")

    def others(s):
        s.update_vertices(v2[first_box:first_box + n_box], first_vertex=first_box)
        s.rebuild_bvh()
        s.set_camera(**INSIDE, medium=GRID)
        s.update_materials(mats[0:1], first_material=0)

    scenes_ = []
    for media_first in (True, False):
        s = gpu.Scene(b)
        vol.Reserve(s, W, H, SPP)
        state_bytes = vol.Render(s, W, H, SPP)[1]["state_bytes"]
        if media_first:
            s.update_media(rec, g)
        others(s)
        if not media_first:
            s.update_media(rec, g)
        scenes_.append((s, state_bytes))
    b.set_bvh_split_method("hlbvh")
    b.set_camera(**INSIDE)
    b.set_camera_medium(GRID)
    fresh = created(gpu, b, [rec, media[HOM]], [g, None], verts=v2, materials=mats)
    for s, state_bytes in scenes_:
        same_tables(s, fresh)
        _, st = same_result(gpu, vol, s, fresh)
        assert st["state_bytes"] == state_bytes and st["media_segments"] > 0
        same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s, fresh, W, H, SPP)


@pytest.mark.gpu
def test_refusals_leave_the_scene_as_it_was(gpu):
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    d8 = np.full(8, 0.5, np.float32)
    p8 = C.c_void_p(d8.ctypes.data)
    call = gpu.lib().gnxr_scene_update_media
    # a scene without media
    s0 = gpu.Scene(scenes.cornell())
    img0, _ = vol.Render(s0, W, H, SPP)
    hom = gpu.Medium()
    hom.type = A.MEDIUM_HOMOGENEOUS
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        s0.update_media(hom)
    t0 = s0.media_tables()
    assert t0["records"].shape == (0, A.DMEDIUM_BYTES // 4) and t0["grids"] == []
    assert biteq(vol.Render(s0, W, H, SPP)[0], img0)
    # a scene with two
    b = base()
    media, grids0 = desc_media(b)
    scene = gpu.Scene(b)
    before, _ = vol.Render(scene, W, H, SPP)
    tables = scene.media_tables()

    def unchanged():
        tables_unchanged(scene, tables)
        assert biteq(vol.Render(scene, W, H, SPP)[0], before)

    ok = edited(media[GRID], d8.reshape(2, 2, 2))
    one = lambda m: (A.Medium * 1)(m)
    assert call(scene._h, 0, 1, None, p8, None) == ERR_INVALID                       # null media
    for first, n in ((-1, 1), (2, 1), (1, 2), (0, 3), (0, -1)):                        # ranges outside the two media
        recs = (A.Medium * 3)(ok, ok, ok)
        assert call(scene._h, first, n, recs, p8, None) == ERR_INVALID, (first, n)
    unchanged()
    assert call(scene._h, 0, 1, one(edited(ok, type=7)), p8, None) == ERR_INVALID      # unknown type
    assert call(scene._h, 0, 1, one(edited(ok, type=0)), None, None) == ERR_INVALID
    for dims in (dict(nx=0), dict(ny=-2), dict(nz=0)):                                 # an empty grid
        assert call(scene._h, 0, 1, one(edited(ok, **dims)), p8, None) == ERR_INVALID, dims
    for off in (-1, 1 << 60, (1 << 63) - 1):                                           # an offset that is negative, or 2^60 or more
        assert call(scene._h, 0, 1, one(edited(ok, density_offset=off)), p8, None) == ERR_INVALID, off
    unchanged()
    # density == NULL: a GRID record must name a medium that is GRID now, with the same resolution
    assert call(scene._h, 0, 1, one(ok), None, None) == ERR_INVALID                    # 2 x 2 x 2 over 24 x 24 x 12
    assert call(scene._h, 1, 1, one(ok), None, None) == ERR_INVALID                    # the homogeneous medium
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.update_media(edited(media[GRID], nx=12))
    unchanged()
    # grids whose packed total would reach 2^31 floats; nothing of the (small) array is read
    for dims in (dict(nx=2048, ny=1024, nz=1024), dict(nx=1 << 30, ny=1 << 30, nz=1 << 30)):
        assert call(scene._h, 1, 1, one(edited(ok, **dims)), p8, None) == ERR_INVALID, dims
    half = edited(ok, nx=1024, ny=1024, nz=1024)                                       # 2^30 floats each: only the total reaches 2^31
    assert call(scene._h, 0, 2, (A.Medium * 2)(half, half), p8, None) == ERR_INVALID
    unchanged()
    # a valid first record, then one that is not: nothing of the first may have been applied
    recs = (A.Medium * 2)(ok, edited(ok, type=9))
    assert call(scene._h, 0, 2, recs, p8, None) == ERR_INVALID
    recs = (A.Medium * 2)(edited(media[HOM], g=0.9), ok)
    assert call(scene._h, 1, 2, recs, p8, None) == ERR_INVALID                         # the second record lies past the list
    unchanged()
    # the hook's own refusals
    n = C.c_int64(0)
    hook = gpu.lib().gnxr_scene_media_tables
    assert hook(scene._h, 2, 0, None, 0, C.byref(n)) == ERR_INVALID and hook(scene._h, -1, 0, None, 0, C.byref(n)) == ERR_INVALID
    assert hook(scene._h, 1, 2, None, 0, C.byref(n)) == ERR_INVALID and hook(scene._h, 1, -1, None, 0, C.byref(n)) == ERR_INVALID
    assert hook(scene._h, 0, 0, None, 0, None) == ERR_INVALID
    assert hook(scene._h, 0, 99, None, 0, C.byref(n)) == 0 and n.value == 2 * A.DMEDIUM_BYTES   # which 0 ignores `medium`
    # n_media == 0 is a no-op, and the handle still takes an edit
    assert call(scene._h, 1, 0, None, None, None) == 0
    unchanged()
    g = d8.reshape(2, 2, 2)
    scene.update_media(ok, g)
    same_tables(scene, created(gpu, b, [ok, media[HOM]], [g, None]))


@pytest.mark.gpu
def test_density_on_another_device_is_invalid(gpu):
    """A density in device memory of a device other than the scene's first."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: the refusal reads the device of the pointer")
    b = base()
    media, _ = desc_media(b)
    scene = gpu.Scene(b)
    tables = scene.media_tables()
    t = torch.full((8,), 0.5, device="cuda:1")
    torch.cuda.synchronize()
    rec = (A.Medium * 1)(edited(media[GRID], np.zeros((2, 2, 2), np.float32)))
    assert gpu.lib().gnxr_scene_update_media(scene._h, 0, 1, rec, C.c_void_p(t.data_ptr()), None) == ERR_INVALID
    tables_unchanged(scene, tables)


@pytest.mark.gpu
def test_on_replicas(gpu):
    """Device 0 listed twice: both copies take the edit (rows are dealt over the replicas)."""
    b = base()
    media, grids0 = desc_media(b)
    g = smoke(20, 16, 10, 5)
    rec = edited(media[GRID], g, sigma_a=(0.4,) * 3, sigma_s=(3.0,) * 3, medium_to_world=M2W)
    thin = edited(rec, sigma_s=(1.5,) * 3)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    single = created(gpu, b, [rec, media[HOM]], [g, None])
    thinned = created(gpu, b, [thin, media[HOM]], [g, None])
    t = torch.from_numpy(g).to("cuda:0")
    torch.cuda.synchronize()
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        vol.Render(multi, 16, 12, 1)
        multi.update_media(rec, g)
        same_tables(multi, single)
        same_result(gpu, vol, multi, single)
        multi.update_media(thin)
        same_result(gpu, vol, multi, thinned)
        multi.update_media(media[GRID], grids0[GRID])
        multi.update_media(rec, t)                       # the replica takes a device-memory grid by peer copy
        same_tables(multi, single)
        same_result(gpu, vol, multi, single)
    finally:
        gpu.init(0)
