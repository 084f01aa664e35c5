"""gnxr_scene_update_environment: the environment map of a live scene replaced or rotated, its tables rebuilt on the device
(csrc/env_build_kernel.hip.h, csrc/api_env.hip.h).

Every comparison is bit for bit and against gnxr_scene_create, whose host build (build_env, csrc/scene_compile.cpp) is the yardstick: scene A
is created with some other map and edited, scene B is created from a description carrying the new map and record, and the two must hold
the same tables (Scene.env_tables: the eight device tables, the DEnv record and the Power lookup) and give the same results.  The scene is
the 2 k-triangle Cornell box of the refit tests with an environment light, 64 x 48 at 4 spp."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import scenes
from conftest import ROOT
from gnxraytracer_amd import _abi as gx_abi
from test_light_update import desc_lights, dragon, fresh_scene, light_records
from test_scene_update import ENV, biteq, deform, model_vertex_count, same_render, vertices, MESH2K

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W, H, SPP = 64, 48, 4
ENV_LIGHT = 2   # dragon(env=ENV): the area light's two triangles, then the INFINITE light
ROT = [0.8, 0.0, 0.6, 0.0, 0.36, 0.8, -0.48, 0.0, -0.48, 0.6, 0.64, 0.0, 0.0, 0.0, 0.0, 1.0]   # a rotation (rows orthonormal)


# ---------------------------------------------------------------- helpers
class WithEnv:
    """The builder's description carrying another environment map, other light records and / or other vertices (all kept alive here)."""

    def __init__(self, builder, rgb=None, lights=None, verts=None):
        self.builder = builder
        self.rgb = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        self.lights = None if lights is None else (gx_abi.Light * len(lights))(*lights)
        self.verts = None if verts is None else np.ascontiguousarray(verts, np.float32)

    def desc(self):
        d = self.builder.desc()
        if self.rgb is not None:
            d.env_rgb = self.rgb.ctypes.data_as(C.POINTER(C.c_float))
            d.env_height, d.env_width = self.rgb.shape[:2]
        if self.lights is not None:
            assert len(self.lights) == d.n_lights
            d.lights = C.cast(self.lights, C.POINTER(gx_abi.Light))
        if self.verts is not None:
            assert self.verts.shape == (d.n_vertices, 3)
            d.vertices = self.verts.ctypes.data_as(C.POINTER(C.c_float))
        return d


def created(gx, b, rgb=None, lights=None, verts=None):
    e = WithEnv(b, rgb, lights, verts)
    s = gx.Scene(e.desc())
    s._keep = e
    return s


def env_map(w, h, seed=1):
    """positive values and one bright texel: the importance table is not flat"""
    m = (0.05 + np.random.default_rng(seed).random((h, w, 3))).astype(np.float32)
    m[h // 3, w // 4] = (60.0, 50.0, 40.0)
    return m


def same_tables(a, b):
    ta, tb = a.env_tables(), b.env_tables()
    assert list(ta) == [n for n, _ in a.ENV_TABLES] and list(ta) == list(tb)
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape, k
        assert np.array_equal(ta[k].view(np.uint8), tb[k].view(np.uint8)), k
    return ta


def edited_lights(gx, b, index=ENV_LIGHT, le=None, l2w=None, n_samples=None):
    ls = desc_lights(gx, b)
    if le is not None:
        ls[index].le[:] = le
    if l2w is not None:
        ls[index].light_to_world[:] = l2w
    if n_samples is not None:
        ls[index].n_samples = n_samples
    return ls


def zero_rows(m, rows):
    m = m.copy()
    m[list(rows)] = 0.0
    return m


# name -> (map, le or None): the smallest shapes at which each branch of the build can go wrong
MAPS = {
    "8x4": (lambda: env_map(8, 4), None),                      # powers of two: no resample
    "13x7": (lambda: env_map(13, 7), None),                    # resample in both axes; taps wrap below 0 and past the edge
    "1x1": (lambda: env_map(1, 1), None),                      # one-level pyramid: the Power lookup's `level < 0` branch
    "2x1": (lambda: env_map(2, 1), None),                      # two levels; modi on the 1-wide levels
    "1x2": (lambda: env_map(1, 2), None),
    "5x12": (lambda: env_map(5, 12), None),                    # taller than wide
    "300x3": (lambda: env_map(300, 3), None),                  # a 1025-entry cdf row: past one wave and one block's lanes in chain and bisection
    "3x300": (lambda: env_map(3, 300), None),                  # a 1025-entry marginal
    "16x8_zero": (lambda: np.zeros((8, 16, 3), np.float32), None),            # funcInt == 0 in every row and in the marginal
    "16x8_zero_rows": (lambda: zero_rows(env_map(16, 8), (2, 5)), None),      # funcInt == 0 in single conditional rows only
    "16x8_le": (lambda: env_map(16, 8), (0.0, 1.5, 0.25)),                    # a zero channel; le folded before the square root
    "1000x500": (lambda: scenes.synthetic_env(), None),                       # the cfg 4 size, once
}


# ---------------------------------------------------------------- CPU
def test_entry_points_exported_and_declared(gx):
    lib = C.CDLL(gx.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gnxr.h")).read()
    for name in ("gnxr_scene_update_environment", "gnxr_scene_env_tables"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES and f"int {name}(" in header
    assert gx.lib().gnxr_abi_version() == 5


def test_null_scene_is_invalid(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    rec = gx.Light()
    rec.type = gx._abi.LIGHT_INFINITE
    m = env_map(4, 2)
    assert gx.lib().gnxr_scene_update_environment(None, C.byref(rec), C.c_void_p(m.ctypes.data), 4, 2, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_environment(None, C.byref(rec), None, 0, 0, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_environment(None, None, None, 0, 0, None) == ERR_INVALID
    n = C.c_int64(0)
    assert gx.lib().gnxr_scene_env_tables(None, 0, None, 0, C.byref(n)) == ERR_INVALID


def test_python_surface(gx):
    assert callable(gx.Scene.update_environment) and callable(gx.Scene.env_tables)
    assert [n for n, _ in gx.Scene.ENV_TABLES] == ["env_texels4", "env_cond_func", "env_cond_cdf", "env_cond_int", "env_marg_func", "env_marg_cdf", "env_marg_guide",
                                                   "env_cond_guide", "env", "env_power_lookup"]
    s = object.__new__(gx.Scene)
    s._h, s.device, s._env_light = None, 0, None
    for bad in ([[[0.0, 0.0, 0.0]]], np.zeros((2, 3, 3), np.float64), np.zeros((2, 3), np.float32), np.zeros((2, 3, 4), np.float32), "rgb"):
        with pytest.raises(ValueError):
            s.update_environment(bad)


# ---------------------------------------------------------------- GPU: the tables
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MAPS))
def test_tables_equal_a_created_scene(gpu, name):
    make, le = MAPS[name]
    m = make()
    b = dragon(env=ENV)
    a = gpu.Scene(b)
    before = a.env_tables()
    a.update_environment(m, le=le)
    fresh = created(gpu, b, m, edited_lights(gpu, b, le=le))
    t = same_tables(a, fresh)
    assert not np.array_equal(t["env_texels4"], before["env_texels4"])
    rx, ry = (1 << (m.shape[1] - 1).bit_length()), (1 << (m.shape[0] - 1).bit_length())
    assert t["env_texels4"].size == 4 * rx * ry and t["env_cond_cdf"].size == (2 * rx + 1) * 2 * ry and t["env_marg_cdf"].size == 2 * ry + 1


@pytest.mark.gpu
def test_device_memory_source(gpu):
    """The map as a tensor produced on a side stream immediately before the call (the stream is passed: the read is ordered after the
    kernel that writes it), then the same map from host memory."""
    m = env_map(13, 7)
    b = dragon(env=ENV)
    a = gpu.Scene(b)
    fresh = created(gpu, b, m)
    half = torch.from_numpy(m * np.float32(0.5)).to("cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = half * 2.0   # (exact)
    a.update_environment(t, stream=st)
    same_tables(a, fresh)
    a.update_environment(env_map(8, 4))
    a.update_environment(m)
    same_tables(a, fresh)
    with pytest.raises(ValueError):
        a.update_environment(t.double())
    with pytest.raises(ValueError):
        a.update_environment(t.permute(1, 0, 2))   # not contiguous


@pytest.mark.gpu
def test_flip_after_a_sky_box(gpu):
    """A SKYBOX light earlier in the light list flips the rows of the map, as at creation."""
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    b.AddSkyLight()
    b.AddInfLight(ENV)
    assert [l.type for l in desc_lights(gpu, b)] == [1, 1, 3, 2]
    m = env_map(13, 7)
    a = gpu.Scene(b)
    a.update_environment(m)
    t = same_tables(a, created(gpu, b, m))
    plain = gpu.Scene(dragon(env=ENV))
    plain.update_environment(m)
    assert not np.array_equal(t["env_texels4"], plain.env_tables()["env_texels4"])
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), a, created(gpu, b, m), W, H, SPP)


@pytest.mark.gpu
def test_size_change_and_back(gpu):
    b = dragon(env=ENV)
    a = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    integ.Render(a, 16, 12, 1)
    for w, h, seed in ((16, 8, 1), (40, 20, 2), (16, 8, 1)):
        m = env_map(w, h, seed)
        a.update_environment(m)
        fresh = created(gpu, b, m)
        same_tables(a, fresh)
        same_render(gpu, integ, a, fresh, W, H, SPP)


# ---------------------------------------------------------------- GPU: results
@pytest.mark.gpu
def test_results_equal_a_created_scene(gpu):
    """One edit -- a 13 x 7 map, a new le, a rotated light_to_world, another n_samples -- then everything a caller can ask of the handle."""
    m, le = env_map(13, 7), (0.7, 1.2, 2.0)
    b = dragon(env=ENV)
    a = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = path.Render(a, W, H, SPP)
    a.update_environment(m, le=le, light_to_world=ROT, n_samples=3)
    fresh = created(gpu, b, m, edited_lights(gpu, b, le=le, l2w=ROT, n_samples=3))
    same_tables(a, fresh)
    img = same_render(gpu, path, a, fresh, W, H, SPP)
    assert not biteq(img, before)
    for integ in (gpu.VolPathIntegrator(5, 1.0, "spatial"), gpu.WhittedIntegrator(5), gpu.DirectLightingIntegrator("all", 5), gpu.PathIntegrator(5, 1.0, "power")):
        same_render(gpu, integ, a, fresh, W, H, SPP)
    for strategy in ("spatial", "uniform", "power"):
        assert biteq(light_records(a, 3, strategy), light_records(fresh, 3, strategy)), strategy
        for on_host in (0, 1):
            assert biteq(a.light_grid_table(strategy, on_host), fresh.light_grid_table(strategy, on_host)), (strategy, on_host)
    fa, _ = path.RenderAOV(a, W, H, SPP, channels=("depth",))
    fb, _ = path.RenderAOV(fresh, W, H, SPP, channels=("depth",))
    assert torch.equal(fa["depth"].view(torch.int32), fb["depth"].view(torch.int32))


@pytest.mark.gpu
def test_rotation_only(gpu):
    """rgb=None: the table buffers stay, the DEnv record, the light record and the light-selection table follow the new transform."""
    b = dragon(env=ENV)
    a = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    img0, _ = integ.Render(a, W, H, SPP)
    before = a.env_tables()
    a.update_environment(light_to_world=ROT)
    after = a.env_tables()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)) == (k != "env"), k
    fresh = fresh_scene(gpu, b, lights=edited_lights(gpu, b, l2w=ROT))
    same_tables(a, fresh)
    img = same_render(gpu, integ, a, fresh, W, H, SPP)
    assert not biteq(img, img0)
    same_render(gpu, gpu.DirectLightingIntegrator("all", 5), a, fresh, W, H, SPP)
    a.update_environment(n_samples=2)   # the record alone
    same_render(gpu, gpu.DirectLightingIntegrator("all", 5), a, fresh_scene(gpu, b, lights=edited_lights(gpu, b, l2w=ROT, n_samples=2)), W, H, SPP)


@pytest.mark.gpu
def test_composes_with_refit_and_rebuild(gpu):
    """update_environment, a refit that grows the world bound, a rebuild: the environment's bounding sphere follows the refit and the tables
    survive the rebuild."""
    m = env_map(13, 7)
    b = dragon(env=ENV)
    nv = model_vertex_count(gpu, MESH2K)
    a = gpu.Scene(b)
    a.update_environment(m, le=(1.5, 1.0, 0.5))
    radius0 = a.env_tables()["env"].view(np.float32)[39]   # DEnv::world_radius
    v2 = deform(vertices(b), nv, seed=4, shift=(0.5, 0.8, 3.0))
    a.update_vertices(v2[:nv])
    a.rebuild_bvh()
    assert a.env_tables()["env"].view(np.float32)[39] > radius0
    b.set_bvh_split_method("hlbvh")
    fresh = created(gpu, b, m, edited_lights(gpu, b, le=(1.5, 1.0, 0.5)), v2)
    same_tables(a, fresh)
    for integ in (gpu.PathIntegrator(5, 1.0, "spatial"), gpu.PathIntegrator(5, 1.0, "power")):
        same_render(gpu, integ, a, fresh, W, H, SPP)


@pytest.mark.gpu
def test_refusals_leave_the_scene_as_it_was(gpu):
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    m = env_map(8, 4)
    p = C.c_void_p(m.ctypes.data)
    # a scene without an environment light
    b0 = dragon()
    s0 = gpu.Scene(b0)
    img0, _ = integ.Render(s0, W, H, SPP)
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        s0.update_environment(m)
    assert all(t.size == 0 for t in s0.env_tables().values())
    assert biteq(integ.Render(s0, W, H, SPP)[0], img0)
    # a scene with one
    b = dragon(env=ENV)
    scene = gpu.Scene(b)
    before, _ = integ.Render(scene, W, H, SPP)
    tables = scene.env_tables()
    rec = desc_lights(gpu, b)[ENV_LIGHT]

    def unchanged():
        now = scene.env_tables()
        for k in tables:
            assert np.array_equal(tables[k].view(np.uint8), now[k].view(np.uint8)), k
        assert biteq(integ.Render(scene, W, H, SPP)[0], before)

    call = gpu.lib().gnxr_scene_update_environment
    for w, h in ((0, 4), (8, 0), (-8, 4)):
        assert call(scene._h, C.byref(rec), p, w, h, None) == ERR_INVALID
    unchanged()
    with pytest.raises(gpu.GnxrError, match="send the map again"):
        scene.update_environment(le=(0.5, 0.5, 0.5))
    unchanged()
    point = desc_lights(gpu, b)[ENV_LIGHT]
    point.type = gpu._abi.LIGHT_POINT
    assert call(scene._h, C.byref(point), p, 8, 4, None) == ERR_INVALID
    assert call(scene._h, None, p, 8, 4, None) == ERR_INVALID
    unchanged()
    wide = np.full((1, 40000, 3), 0.5, np.float32)   # 2 * 65536 + 1 does not fit a guide entry
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.update_environment(wide)
    unchanged()
    # update_lights still refuses a changed INFINITE record
    ls = desc_lights(gpu, b)
    ls[ENV_LIGHT].le[:] = [0.5, 0.5, 0.5]
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        scene.update_lights(ls[ENV_LIGHT:ENV_LIGHT + 1], first_light=ENV_LIGHT)
    unchanged()
    # and the handle still takes an edit
    scene.update_environment(m)
    same_tables(scene, created(gpu, b, m))


@pytest.mark.gpu
def test_on_replicas(gpu):
    """Device 0 listed twice: both copies build their tables (rows are dealt over the replicas)."""
    m, le = env_map(13, 7), (0.7, 1.2, 2.0)
    b = dragon(env=ENV)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    ident = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    single = created(gpu, b, m, edited_lights(gpu, b, le=le, l2w=ROT))
    turned_back = created(gpu, b, m, edited_lights(gpu, b, le=le, l2w=ident))
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        integ.Render(multi, 16, 12, 1)
        multi.update_environment(m, le=le, light_to_world=ROT)
        same_tables(multi, single)
        same_render(gpu, integ, multi, single, W, H, SPP)
        multi.update_environment(light_to_world=ident)
        same_render(gpu, integ, multi, turned_back, W, H, SPP)
    finally:
        gpu.init(0)
