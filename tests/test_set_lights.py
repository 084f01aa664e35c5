"""gnxr_scene_set_lights: the light list of a live scene replaced -- lights added, removed and retyped, other triangles made emissive
(csrc/api_lights.hip.h, csrc/lights_kernel.hip.h, compile_light_list in csrc/scene_compile.cpp).

The reference of every GPU case is a FRESH scene created from the builder's description with `lights`, `n_lights` and `tri_light`
replaced (Relit).  Every comparison is bit for bit: renders of all four integrators (Path with the three light strategies, VolPath,
Whitted, DirectLighting "one" and "all") with their ray counts, the device's light records and DTri::light (Scene.light_tables),
Scene.sample_light of every light at the fixed points of test_light_update, and the light-selection tables of the three strategies,
device- and host-built.  The 2 k-triangle Cornell scene of the refit tests, 64 x 48 at 4 spp."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded, as in test_scene_update.py)

import oracle_lib as ol
import scenes
from gnxraytracer_amd import _abi as gx_abi
from test_light_update import desc_lights, dragon, light_records, move_light
from test_scene_update import ENV, biteq, indices, vertices
from test_set_geometry import geometry_of, on_device

ERR_INVALID, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -2, -4
W, H, SPP = 64, 48, 4
AREA, INFINITE, SKYBOX, POINT, SPOT, DISTANT = gx_abi.LIGHT_AREA_TRI, gx_abi.LIGHT_INFINITE, gx_abi.LIGHT_SKYBOX, gx_abi.LIGHT_POINT, gx_abi.LIGHT_SPOT, gx_abi.LIGHT_DISTANT
IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


# ---------------------------------------------------------------- helpers
class Relit:
    """The builder's description with another light list -- lights, n_lights and the tri_light that matches them -- and optionally other
    vertices, another mesh (the keyword dictionary of Scene.set_geometry, its tri_light ignored) and another split method; everything
    is kept alive here."""

    def __init__(self, builder, lights, verts=None, geom=None, split=None):
        self.builder, self.split = builder, split
        self.verts = None if verts is None else np.ascontiguousarray(verts, np.float32)
        self.geom = None if geom is None else {k: (None if v is None else np.ascontiguousarray(v)) for k, v in geom.items()}
        self.arr = (gx_abi.Light * max(len(lights), 1))()
        for k, l in enumerate(lights):
            C.memmove(C.byref(self.arr[k]), C.byref(l), C.sizeof(gx_abi.Light))
        self.n = len(lights)

    def desc(self):
        d, g = self.builder.desc(), self.geom
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        if g is not None:
            d.n_vertices, d.n_triangles = len(g["vertices"]), len(g["indices"])
            d.vertices, d.indices, d.tri_material = fp(g["vertices"]), ip(g["indices"]), ip(g["tri_material"])
            d.tri_medium_inside, d.tri_medium_outside = ip(g["medium_inside"]), ip(g["medium_outside"])
            d.tri_uv, d.tri_n, d.tri_s = fp(g["uv"]), fp(g["normals"]), fp(g["tangents"])
        if self.verts is not None:
            assert self.verts.shape == (d.n_vertices, 3)
            d.vertices = fp(self.verts)
        self.tri_light = np.full(d.n_triangles, -1, np.int32)
        for k in range(self.n):
            if self.arr[k].type == AREA:
                self.tri_light[self.arr[k].tri] = k
        d.tri_light, d.lights, d.n_lights = ip(self.tri_light), C.cast(self.arr, C.POINTER(gx_abi.Light)), self.n
        if self.split:
            d.bvh_split_method = {"sah": 0, "hlbvh": 1}[self.split]
        d.keep_alive = self   # a Scene keeps the description it was created from
        return d


def fresh(gx, b, lights, **kw):
    return gx.Scene(Relit(b, lights, **kw).desc())


def copy_of(l):
    c = gx_abi.Light()
    C.memmove(C.byref(c), C.byref(l), C.sizeof(gx_abi.Light))
    return c


def area(tri, le, two_sided=0, n_samples=1):
    l = gx_abi.Light()
    l.type, l.tri, l.two_sided, l.n_samples = AREA, int(tri), two_sided, n_samples
    l.le[:] = le
    l.light_to_world[:] = IDENTITY
    return l


def delta(kind, le, to_world=IDENTITY, direction=(0.0, 0.0, 1.0), cone=(30.0, 20.0)):
    l = gx_abi.Light()
    l.type, l.tri, l.n_samples = kind, -1, 1
    l.le[:] = le
    l.light_to_world[:] = to_world
    l.center[:] = direction
    l.radius, l.falloff_start = cone
    return l


def extra_lights():
    """a point, a spot, a distant and a sky-box light"""
    sky = gx_abi.Light()
    sky.type, sky.tri, sky.n_samples, sky.radius = SKYBOX, -1, 1, 20.0
    sky.le[:] = [0.3, 0.4, 0.6]
    sky.light_to_world[:] = IDENTITY
    return [delta(POINT, (6.0, 5.0, 4.0), [1, 0, 0, 0.8, 0, 1, 0, 1.2, 0, 0, 1, 0.9, 0, 0, 0, 1]),
            delta(SPOT, (40.0, 30.0, 20.0), [0.8, 0.0, 0.6, 0.9, 0.36, 0.8, -0.48, 2.1, -0.48, 0.6, 0.64, 0.7, 0.0, 0.0, 0.0, 1.0], cone=(38.0, 12.0)),
            delta(DISTANT, (1.5, 1.2, 0.9), direction=(0.3, 1.0, 0.4)), sky]


def layout(b):
    """(model triangles, wall triangles, the two ceiling-light triangles) of dragon(): AddModel first, then AddCornell, then AddAreaLight"""
    nt = b.desc().n_triangles
    return np.arange(nt - 12), np.arange(nt - 12, nt - 2), np.arange(nt - 2, nt)


def integrators(gx):
    return ([gx.PathIntegrator(5, 1.0, s) for s in ("spatial", "power", "uniform")] +
            [gx.VolPathIntegrator(5, 1.0, "spatial"), gx.WhittedIntegrator(5), gx.DirectLightingIntegrator("one", 5), gx.DirectLightingIntegrator("all", 5)])


def same_image(gx, integ, s1, s2):
    """images and ray counts of two scenes (or a scene and the oracle); a scene without lights may render black"""
    i1, st1 = integ.Render(s1, W, H, SPP)
    i2, st2 = integ.Render(s2, W, H, SPP) if isinstance(s2, gx.Scene) else s2.render(integ, W, H, SPP)
    assert (st1["rays_closest"], st1["rays_any"]) == (st2["rays_closest"], st2["rays_any"])
    assert biteq(i1[..., :3], i2[..., :3])
    return i1


def same_tables(s1, s2, n_lights, records=True):
    """records: the trees are the same, so the DLight words (tri_leaf among them) must be"""
    (r1, t1), (r2, t2) = s1.light_tables(), s2.light_tables()
    assert s1.n_lights == s2.n_lights == n_lights and r1.shape == r2.shape == (n_lights, 28)
    assert np.array_equal(t1, t2)
    if records:
        assert np.array_equal(r1, r2)
    if n_lights:
        for strategy in ("power", "spatial"):
            assert biteq(light_records(s1, n_lights, strategy), light_records(s2, n_lights, strategy))
    for strategy in ("spatial", "power", "uniform"):
        for on_host in (0, 1):
            ta, tb = s1.light_grid_table(strategy, on_host), s2.light_grid_table(strategy, on_host)
            assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes(), (strategy, on_host)


def same_everything(gx, s1, s2, n_lights, records=True):
    for integ in integrators(gx):
        same_image(gx, integ, s1, s2)
    same_tables(s1, s2, n_lights, records)


def moved_emission(gx, b):
    """the ceiling light's two records gone, two wall triangles emissive with other radiance"""
    _, walls, _ = layout(b)
    return [l for l in desc_lights(gx, b) if l.type != AREA] + [area(walls[2], (7.0, 3.0, 1.0)), area(walls[7], (1.0, 4.0, 9.0), two_sided=1)]


def empty_scene(gx):
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_lights, s._env_light = None, 0, 0, None
    return s


# ---------------------------------------------------------------- CPU
def test_entry_points_exported_with_prototypes(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_scene_set_lights", "gnxr_scene_light_tables"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert gx.lib().gnxr_abi_version() == 5 and gx._abi.DLIGHT_BYTES == 112


def test_declared_in_the_header(gx):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(gx.__file__))), "include", "gnxr.h")).read()
    assert "int gnxr_scene_set_lights(gnxr_scene *scene, const gnxr_light *lights, int32_t n_lights, void *hip_stream);" in header
    assert "int gnxr_scene_light_tables(" in header


def test_argument_checks_answer_before_a_device(gx):
    """Null scene, negative count, null array with n > 0: GNXR_ERR_INVALID on a machine without a GPU too, never GNXR_ERR_NO_DEVICE.  No
    handle exists without a GPU, so the scene here is null and that check answers first; the others run against a live handle in
    test_refusals_leave_the_scene_alone."""
    l = (gx.Light * 2)()
    for lights, n in ((l, 2), (None, 0), (l, -1), (None, 3), (l, 0)):
        assert gx.lib().gnxr_scene_set_lights(None, lights, n, None) == ERR_INVALID
    n = C.c_int64(0)
    assert gx.lib().gnxr_scene_light_tables(None, 0, None, 0, C.byref(n)) == ERR_INVALID


def test_set_lights_rejects_other_inputs_before_the_library(gx):
    """Anything that is not a Light raises ValueError, a bad stream TypeError / ValueError, before a library call (the handle here is
    empty: a call would fail differently)."""
    s = empty_scene(gx)
    for bad in ([1, 2], [gx.Light(), None], [gx.Material()], "ab", [(1, 2, 3)]):
        with pytest.raises(ValueError):
            s.set_lights(bad)
    with pytest.raises(TypeError):
        s.set_lights([gx.Light()], stream="s")
    with pytest.raises(ValueError):
        s.set_lights([gx.Light()], stream=-1)
    assert s.n_lights == 0


def test_light_list_validation_host(tmp_path):
    """The host part of the call (compile_light_list: ranges, duplicates, unknown types, the INFINITE rules, nothing written on a
    refusal) in a stand-alone program over the library's host sources: tests/set_lights_check.cpp."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "gnxraytracer_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "set_lights_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(root, "include"), "-I" + csrc, os.path.join(root, "tests", "set_lights_check.cpp"),
                           os.path.join(csrc, "scene_compile.cpp"), os.path.join(csrc, "scene_builder.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_move_the_emission(gpu):
    """1. The ceiling light removed, two wall triangles emissive: a fresh scene's results, and the oracle's on the edited description
    walking the device's tree (the fresh scene and the edited one sharing a bug would otherwise agree)."""
    b = dragon()
    scene = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = path.Render(scene, W, H, SPP)   # (leaves a light-selection table of the old list behind)
    ls = moved_emission(gpu, b)
    scene.set_lights(ls)
    same_everything(gpu, scene, fresh(gpu, b, ls), 2)
    o = ol.OracleScene(Relit(b, ls))
    o.set_bvh(*scene.bvh())
    after = same_image(gpu, path, scene, o)
    assert after[..., :3].any() and not biteq(after, before)
    tri = scene.light_tables()[1]
    _, walls, ceiling = layout(b)
    assert (tri[ceiling] == -1).all() and tri[walls[2]] == 0 and tri[walls[7]] == 1 and (tri >= 0).sum() == 2


@pytest.mark.gpu
def test_area_only_to_mixed_and_back(gpu):
    """2. A point, a spot, a distant and a SKYBOX light appended: the plan leaves the area-only kernels and gains the escape queue.  The
    original list set back returns the first render's bits."""
    b = dragon()
    scene = gpu.Scene(b)
    integs = integrators(gpu)
    first = [it.Render(scene, W, H, SPP) for it in integs]
    orig = desc_lights(gpu, b)
    ls = orig + extra_lights()
    scene.set_lights(ls)
    same_everything(gpu, scene, fresh(gpu, b, ls), 6)
    assert not biteq(integs[0].Render(scene, W, H, SPP)[0], first[0][0])
    scene.set_lights(orig)
    for it, (img, st) in zip(integs, first):
        img1, st1 = it.Render(scene, W, H, SPP)
        assert biteq(img1, img) and (st1["rays_closest"], st1["rays_any"]) == (st["rays_closest"], st["rays_any"])
    same_tables(scene, gpu.Scene(b), 2)


@pytest.mark.gpu
def test_mesh_light_of_forty_triangles(gpu):
    """3. More than kGridMaxLights (16) lights: 40 triangles of the model emissive.  The spatial table is k_light_grid_any's.  DirectLighting
    "all" samples n_samples per light and vertex: 40 x 6 = 240 renders, 40 x 7 = 280 is refused by the render, not by set_lights."""
    b = dragon()
    model, _, _ = layout(b)
    scene = gpu.Scene(b)
    tris = model[7::len(model) // 40][:40]
    assert len(tris) == 40
    direct = gpu.DirectLightingIntegrator("all", 5)
    for n_samples in (6, 7):
        ls = [area(t, (3.0 + 0.1 * k, 2.0, 4.0 - 0.05 * k), two_sided=k % 2, n_samples=n_samples) for k, t in enumerate(tris)]
        scene.set_lights(ls)
        new = fresh(gpu, b, ls)
        for integ in (gpu.PathIntegrator(5, 1.0, "spatial"), gpu.PathIntegrator(5, 1.0, "power")):
            assert same_image(gpu, integ, scene, new)[..., :3].any()
        same_tables(scene, new, 40)
        if 40 * n_samples <= 256:
            same_image(gpu, direct, scene, new)
        else:
            for s in (scene, new):
                with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
                    direct.Render(s, W, H, SPP)


@pytest.mark.gpu
def test_zero_lights_and_back(gpu):
    """4. An empty list renders what a scene created without lights renders; the original list restores the original bits."""
    b = dragon()
    scene = gpu.Scene(b)
    integs = integrators(gpu)
    first = [it.Render(scene, W, H, SPP)[0] for it in integs]
    scene.set_lights([])
    assert scene.n_lights == 0
    same_everything(gpu, scene, fresh(gpu, b, []), 0)
    scene.set_lights(desc_lights(gpu, b))
    for it, img in zip(integs, first):
        assert biteq(it.Render(scene, W, H, SPP)[0], img)
    same_tables(scene, gpu.Scene(b), 2)


@pytest.mark.gpu
def test_environment_scene(gpu):
    """5. The INFINITE record moves to index 0 and one area triangle goes; update_environment still works afterwards.  A changed INFINITE
    record, a second one, none, or a SKYBOX record in front of it are refused and leave the scene as it was."""
    b = dragon(env=ENV)
    orig = desc_lights(gpu, b)
    assert [l.type for l in orig] == [AREA, AREA, INFINITE]
    scene = gpu.Scene(b)
    ls = [orig[2], orig[1]]
    scene.set_lights(ls)
    same_everything(gpu, scene, fresh(gpu, b, ls), 2)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    img0, rec0 = path.Render(scene, W, H, SPP)[0], scene.light_tables()
    sky = extra_lights()[3]
    changed = copy_of(orig[2])
    changed.le[:] = [0.5, 0.5, 0.5]
    for bad in ([changed, orig[1]], [orig[2], orig[1], orig[2]], [orig[1]], [sky, orig[2], orig[1]], []):
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}") as e:
            scene.set_lights(bad)
        assert "gnxr_scene_update_environment" in str(e.value)
        assert scene.n_lights == 2 and all(np.array_equal(x, y) for x, y in zip(scene.light_tables(), rec0))
        assert biteq(path.Render(scene, W, H, SPP)[0], img0)
    rot = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    scene.update_environment(light_to_world=rot)
    ls[0] = copy_of(orig[2])
    ls[0].light_to_world[:] = rot
    new = fresh(gpu, b, ls)
    same_everything(gpu, scene, new, 2)
    assert not biteq(path.Render(scene, W, H, SPP)[0], img0)
    scene.set_lights(ls[::-1] + extra_lights()[:1])   # (the rotated record is the current one now)
    same_image(gpu, path, scene, fresh(gpu, b, ls[::-1] + extra_lights()[:1]))


@pytest.mark.gpu
def test_refusals_leave_the_scene_alone(gpu):
    """6. tri out of range, a duplicate tri, an unknown type (GNXR_ERR_INVALID), an INFINITE record on a scene without one
    (GNXR_ERR_UNSUPPORTED), a negative count and a null array with a live handle: a render and light_tables() keep their bits, also when
    acceptable records precede the refused one."""
    b = dragon()
    nt = b.desc().n_triangles
    scene = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "power")
    img0, rec0 = path.Render(scene, W, H, SPP)[0], scene.light_tables()

    def unchanged():
        assert scene.n_lights == 2 and all(np.array_equal(x, y) for x, y in zip(scene.light_tables(), rec0))
        assert biteq(path.Render(scene, W, H, SPP)[0], img0)

    good = moved_emission(gpu, b)
    unknown = copy_of(good[0])
    unknown.type = 77
    env = delta(INFINITE, (1.0, 1.0, 1.0))
    for bad, code in (([area(nt, (1, 1, 1))], ERR_INVALID), ([area(-1, (1, 1, 1))], ERR_INVALID), (good + [area(good[0].tri, (1, 1, 1))], ERR_INVALID),
                      (good + [unknown], ERR_INVALID), (good + [env], ERR_UNSUPPORTED)):
        with pytest.raises(gpu.GnxrError, match=f"error {code}"):
            scene.set_lights(bad)
        unchanged()
    arr = (gpu.Light * 2)(*good)
    assert gpu.lib().gnxr_scene_set_lights(scene._h, arr, -1, None) == ERR_INVALID
    assert gpu.lib().gnxr_scene_set_lights(scene._h, None, 2, None) == ERR_INVALID
    unchanged()


@pytest.mark.gpu
def test_triangle_with_normals_cannot_become_emissive(gpu, tmp_path):
    """As at creation: a triangle with per-vertex normals is refused as an emissive one.  The check runs on the device after DTri::light
    was written, so this is also the path that puts the old values back."""
    tex = str(tmp_path / "t.hdr")
    scenes.write_rgbe(tex, np.full((8, 8, 3), 0.5, np.float32), rle=False)
    b = scenes.smooth_cornell(tex, medium_ball=False)
    d = b.desc()
    normals = np.ctypeslib.as_array(d.tri_n, shape=(d.n_triangles, 9))
    tangents = np.ctypeslib.as_array(d.tri_s, shape=(d.n_triangles, 9))
    smooth = int(np.flatnonzero(np.abs(normals).sum(1) > 0)[0])
    panel = int(np.flatnonzero((np.abs(normals).sum(1) == 0) & (np.abs(tangents).sum(1) > 0))[0])   # tangents without normals
    scene = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    img0, rec0 = path.Render(scene, W, H, SPP)[0], scene.light_tables()
    keep = desc_lights(gpu, b)
    for tri in (smooth, panel):
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
            scene.set_lights(keep + [area(tri, (2, 2, 2))])
        assert scene.n_lights == len(keep) and all(np.array_equal(x, y) for x, y in zip(scene.light_tables(), rec0))
        assert biteq(path.Render(scene, W, H, SPP)[0], img0)
        with pytest.raises(gpu.GnxrError):
            fresh(gpu, b, keep + [area(tri, (2, 2, 2))])
    scene.set_lights(keep + [area(0, (2, 2, 2))])   # (a wall triangle: no normals, no tangents)
    same_image(gpu, path, scene, fresh(gpu, b, keep + [area(0, (2, 2, 2))]))


@pytest.mark.gpu
def test_later_edits_see_the_new_list(gpu):
    """7. update_lights counts the new list; a newly emissive triangle moves only with move_lights; rebuild_bvh keeps the lights; and
    set_lights after rebuild_bvh, with no host sync in between, binds to the device's leaf order."""
    b = dragon()
    scene = gpu.Scene(b)
    path = gpu.PathIntegrator(5, 1.0, "spatial")
    ls = moved_emission(gpu, b) + extra_lights()[:1]
    scene.set_lights(ls)
    n = len(ls)
    ls[n - 1].le[:] = [9.0, 1.0, 2.0]
    ls[0].le[:] = [2.0, 8.0, 3.0]
    scene.update_lights(ls[n - 1:], first_light=n - 1)
    scene.update_lights(ls[:1])
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.update_lights(ls[:1], first_light=n)
    same_everything(gpu, scene, fresh(gpu, b, ls), n)
    # a newly emissive wall triangle
    lv = np.unique(indices(b)[[ls[0].tri, ls[1].tri]])
    v2 = move_light(vertices(b), lv)
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        scene.update_vertices(v2)
    scene.update_vertices(v2, move_lights=True)
    moved = fresh(gpu, b, ls, verts=v2)
    same_image(gpu, path, scene, moved)
    same_tables(scene, moved, n, records=False)   # (a refitted tree and a new one: tri_leaf may differ)
    # the old ceiling triangles are ordinary triangles now: they move without the flag
    _, _, ceiling = layout(b)
    cv = np.unique(indices(b)[ceiling])
    v3 = v2.copy()
    v3[cv] += np.float32(-0.05)
    scene.update_vertices(v3[cv.min():cv.max() + 1], first_vertex=int(cv.min()))
    scene.rebuild_bvh()
    rebuilt = fresh(gpu, b, ls, verts=v3, split="hlbvh")
    same_image(gpu, path, scene, rebuilt)
    same_tables(scene, rebuilt, n)
    # no bvh() / host sync between the rebuild and this call
    scene.rebuild_bvh()
    ls2 = desc_lights(gpu, b) + moved_emission(gpu, b) + extra_lights()[1:3]
    scene.set_lights(ls2)
    same_everything(gpu, scene, fresh(gpu, b, ls2, verts=v3, split="hlbvh"), len(ls2))


@pytest.mark.gpu
def test_mesh_and_lights_together(gpu):
    """8. The three-call recipe: set_lights with the non-area lights, set_geometry (device tensors) with a mesh that has another triangle
    count and no emissive triangle, set_lights with the full list on the new triangles -- five emissive triangles instead of two."""
    b = dragon(env=ENV)
    orig = desc_lights(gpu, b)
    g = geometry_of(b)
    nt = len(g["indices"])
    keep = np.ones(nt, bool)
    keep[np.arange(0, nt - 12)[::3]] = False
    g2 = {k: (v if v is None or k == "vertices" else np.ascontiguousarray(v[keep])) for k, v in g.items()}
    g2["tri_light"] = None
    n2 = int(keep.sum())
    new_of_old = np.cumsum(keep) - 1
    ceiling = [int(new_of_old[l.tri]) for l in orig if l.type == AREA]
    ls = [orig[2]] + [area(t, (5.0, 5.0, 4.0)) for t in ceiling] + [area(n2 - 12 + k, (0.5 + k, 2.0, 3.0 - k), two_sided=1) for k in (1, 4, 8)]
    scene = gpu.Scene(b)
    gpu.PathIntegrator(5, 1.0, "spatial").Render(scene, 16, 12, 1)
    scene.set_lights([orig[2]])
    scene.set_geometry(**on_device(g2))
    assert scene.n_triangles == n2 and (scene.light_tables()[1] == -1).all()
    scene.set_lights(ls)
    same_everything(gpu, scene, fresh(gpu, b, ls, geom=g2, split="hlbvh"), len(ls))


@pytest.mark.gpu
def test_set_lights_on_replicas(gpu):
    """9. Device 0 listed twice: a shortened sequence of cases 1, 2 and 7 leaves the replicated scene where it leaves a scene on one
    device (rows are dealt over the copies, so a list that stayed behind on the second copy shows in every other row)."""
    b = dragon()
    ls1 = moved_emission(gpu, b)
    ls2 = desc_lights(gpu, b) + extra_lights()
    ls3 = [copy_of(l) for l in ls2]
    ls3[-2].le[:] = [4.0, 1.0, 0.5]
    lv = np.unique(indices(b)[[ls1[0].tri, ls1[1].tri]])
    v2 = move_light(vertices(b), lv)
    path, direct = gpu.PathIntegrator(5, 1.0, "spatial"), gpu.DirectLightingIntegrator("all", 5)
    steps = [lambda s: path.Render(s, 16, 12, 1),
             lambda s: s.set_lights(ls1),
             lambda s: s.update_vertices(v2, move_lights=True),
             lambda s: s.rebuild_bvh(),
             lambda s: s.set_lights(ls2),
             lambda s: s.update_lights(ls3[-2:], first_light=len(ls3) - 2),
             lambda s: s.set_lights([])]
    single = gpu.Scene(b)
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        for k, step in enumerate(steps, 1):
            step(single)
            step(multi)
            if k in (2, 3, 5, 6, 7):
                for integ in (path, direct):
                    same_image(gpu, integ, multi, single)
                assert all(np.array_equal(x, y) for x, y in zip(single.light_tables(), multi.light_tables()))
        for x, y in zip(single.bvh() + single.bvh4(), multi.bvh() + multi.bvh4()):
            assert biteq(x, y) if getattr(x, "dtype", None) == np.float32 else np.array_equal(x, y)
        single.set_lights(ls3)
        multi.set_lights(ls3)
        assert biteq(light_records(single, len(ls3)), light_records(multi, len(ls3)))
        assert same_image(gpu, path, multi, single)[..., :3].any()
    finally:
        gpu.init(0)
