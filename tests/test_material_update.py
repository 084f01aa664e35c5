"""Materials of a live scene edited in place: gnxr_scene_update_materials (material records, the type included) and
gnxr_scene_set_triangle_materials (per-triangle assignment), csrc/material_kernel.hip.h and csrc/api_edit.hip.h.

Every comparison is bit for bit.  The reference of every case is a FRESH Scene created from the description carrying the edited records /
ids (code the other suites pin to the compiled reference); the first case is also compared with the oracle on that description walking
the device's exported tree.  The 2 k-triangle Cornell scene of the refit tests, 64 x 48 at 4 spp."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
import test_hlbvh_build as thb
from gnxraytracer_amd import _abi as A
from test_aov import TEX
from test_light_update import light_records
from test_li_device import cam_batch
from test_scene_update import ENV, MESH2K, biteq, deform, emissive_vertices, model_vertex_count, same_render, vertices

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W, H, SPP = 64, 48, 4


# ---------------------------------------------------------------- helpers
class Edited:
    """The builder's description with other vertices, material records and / or tri_material (all kept alive here)."""

    def __init__(self, builder, verts=None, materials=None, tri_material=None):
        self.builder = builder
        d = builder.desc()
        self.verts = None if verts is None else np.ascontiguousarray(verts, np.float32)
        assert self.verts is None or self.verts.shape == (d.n_vertices, 3)
        self.materials = None
        if materials is not None:
            assert len(materials) == d.n_materials
            self.materials = (A.Material * len(materials))(*materials)
        self.tri_material = None if tri_material is None else np.ascontiguousarray(tri_material, np.int32)
        assert self.tri_material is None or self.tri_material.shape == (d.n_triangles,)

    def desc(self):
        d = self.builder.desc()
        if self.verts is not None:
            d.vertices = self.verts.ctypes.data_as(C.POINTER(C.c_float))
        if self.materials is not None:
            d.materials = C.cast(self.materials, C.POINTER(A.Material))
        if self.tri_material is not None:
            d.tri_material = self.tri_material.ctypes.data_as(C.POINTER(C.c_int32))
        return d


def fresh_scene(gx, b, verts=None, materials=None, tri_material=None, split=None):
    if split:
        b.set_bvh_split_method(split)
    e = Edited(b, verts, materials, tri_material)
    s = gx.Scene(e.desc())
    s._keep = e
    return s


def desc_materials(gx, b):
    """copies of the description's material records"""
    d = b.desc()
    out = []
    for i in range(d.n_materials):
        m = gx.Material()
        C.memmove(C.byref(m), C.byref(d.materials[i]), C.sizeof(gx.Material))
        out.append(m)
    return out


def tri_materials(b):
    d = b.desc()
    return np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,)).copy()


def with_record(mats, index, record):
    out = list(mats)
    out[index] = record
    return out


def integrators(gx, names):
    table = {"path": lambda: gx.PathIntegrator(5, 1.0, "spatial"), "whitted": lambda: gx.WhittedIntegrator(5),
             "direct": lambda: gx.DirectLightingIntegrator("all", 5), "volpath": lambda: gx.VolPathIntegrator(5, 1.0, "spatial")}
    return [table[n]() for n in names]


def same_aov(gx, a, b, spp=SPP):
    it = gx.PathIntegrator(5, 1.0, "spatial")
    fa, _ = it.RenderAOV(a, W, H, spp)
    fb, _ = it.RenderAOV(b, W, H, spp)
    for c in fa:
        assert torch.equal(fa[c].view(torch.int32), fb[c].view(torch.int32)), c
    return fa


def same_triangle_materials(a, b, expect=None):
    (ma, ca), (mb, cb) = a.triangle_materials(), b.triangle_materials()
    assert np.array_equal(ma, mb) and np.array_equal(ca, cb)
    if expect is not None:
        assert np.array_equal(ma, expect)
    return ma, ca


def same_everything(gx, scene, fresh, names=("path",), expect=None):
    """renders (image and both ray counts), the feature buffers with ids and albedo, and the per-triangle state"""
    for it in integrators(gx, names):
        same_render(gx, it, scene, fresh, W, H, SPP)
    same_aov(gx, scene, fresh)
    return same_triangle_materials(scene, fresh, expect)


def all_matte_dragon(gx):
    """the Cornell dragon with one Matte material on the whole model: every material of the scene is class 0.  Returns (builder, the
    dragon's material index)"""
    b = gx.SceneBuilder()
    white, red, blue = (b.MatteMaterial(c, 60.0) for c in (scenes.WHITE, scenes.RED, scenes.BLUE))
    green = b.MatteMaterial(scenes.DRAGON_GREEN, 60.0)
    b.AddModel(MESH2K, green)
    b.AddCornell(red, blue, white)
    b.AddAreaLight(white)
    return b, green


def class_steps(gx):
    """Plastic, Glass, Disney: the records the dragon's material becomes in turn"""
    return [gx.material(type=A.MAT_PLASTIC, kd=(0.3, 0.1, 0.6), ks=(0.5, 0.5, 0.5), urough=0.1, vrough=0.1, remap_roughness=1),
            gx.material(type=A.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0),
            gx.material(type=A.MAT_DISNEY, kd=(0.8, 0.5, 0.2), eta=(1.5, 0, 0), disney_metallic=0.4, disney_roughness=0.4, disney_clearcoat=0.6,
                        disney_clearcoat_gloss=0.9, disney_sheen=0.3, disney_spec_trans=0.0, disney_diff_trans=1.0)]


def every_other(ids, n_model, to):
    out = ids.copy()
    out[0:n_model:2] = to
    return out


def model_triangle_count(gx):
    b = gx.SceneBuilder()
    b.AddModel(MESH2K, b.MatteMaterial(scenes.WHITE, 60.0))
    return b.desc().n_triangles


# ---------------------------------------------------------------- CPU
def test_entry_points_exported(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_scene_update_materials", "gnxr_scene_set_triangle_materials", "gnxr_scene_triangle_materials"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES, name
    assert gx.lib().gnxr_abi_version() == 5 and gx._abi.GNXR_ABI_VERSION == 5


def test_null_scene_is_invalid(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    m = (gx.Material * 1)()
    ids = np.zeros(4, np.int32)
    assert gx.lib().gnxr_scene_update_materials(None, 0, 1, m) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_materials(None, 0, 0, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_set_triangle_materials(None, 0, 4, C.c_void_p(ids.ctypes.data), None) == ERR_INVALID
    assert gx.lib().gnxr_scene_set_triangle_materials(None, 0, 0, None, None) == ERR_INVALID
    assert gx.lib().gnxr_scene_triangle_materials(None, None, None, 0) == ERR_INVALID


def test_python_layer_rejects_other_inputs_before_the_library(gx):
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_triangles = None, 0, 8
    for bad in (np.zeros(4, np.int64), np.zeros(4, np.float32), np.zeros((4, 1), np.int32), np.zeros((2, 2), np.int32), [0, 1, 2], 3):
        with pytest.raises(ValueError):
            s.set_triangle_materials(bad)
    with pytest.raises(ValueError):
        s.update_materials([1, 2])
    with pytest.raises(ValueError):
        s.update_materials([gx.Light()])
    m = gx.material(type=A.MAT_MATTE, kd=(0.1, 0.2, 0.3), sigma=20.0)
    assert isinstance(m, gx.Material) and m.type == A.MAT_MATTE and list(m.kd) == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    assert biteq(gx.material_albedo(type=A.MAT_MATTE, kd=(0.1, 0.2, 0.3)), np.array([0.1, 0.2, 0.3], np.float32))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_parameter_edit_inside_a_class(gpu):
    """kd and sigma of the dragon's Matte change: path render == fresh scene == the oracle on the edited description (device tree)"""
    b, green = all_matte_dragon(gpu)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = integ.Render(scene, W, H, SPP)
    mats = with_record(desc_materials(gpu, b), green, gpu.material(type=A.MAT_MATTE, kd=(0.7, 0.3, 0.15), sigma=20.0))
    scene.update_materials([mats[green]], first_material=green)
    after = same_render(gpu, integ, scene, fresh_scene(gpu, b, materials=mats), W, H, SPP)
    o = ol.OracleScene(Edited(b, materials=mats))
    o.set_bvh(*scene.bvh())
    same_render(gpu, integ, scene, o, W, H, SPP)
    assert not biteq(after, before)


ALL_FOUR = ("path", "whitted", "direct", "volpath")


def class_changing_edits(gx, b, green, scene, fresh_of):
    """The dragon's Matte becomes Plastic, Glass, Disney: every step is fresh_of(materials=...) under all four integrators, and the original
    record brings the bits of the handle's first renders back"""
    its = integrators(gx, ALL_FOUR)
    first = [it.Render(scene, W, H, SPP)[0] for it in its]
    mats0 = desc_materials(gx, b)
    classes = []
    for rec in class_steps(gx):
        scene.update_materials([rec], green)
        fresh = fresh_of(materials=with_record(mats0, green, rec))
        _, cls = same_everything(gx, scene, fresh, ALL_FOUR, expect=tri_materials(b))
        classes.append(int(cls[0]))
    assert all(c != 0 for c in classes) and len(set(classes)) >= 2, classes   # (the classes themselves are the fresh scene's, checked above)
    scene.update_materials([mats0[green]], green)
    for it, img in zip(its, first):
        assert biteq(it.Render(scene, W, H, SPP)[0], img)
    assert (scene.triangle_materials()[1] == 0).all()


@pytest.mark.gpu
def test_class_changing_edits(gpu):
    """all-Matte scene (class mask 1); the dragon becomes Plastic, Glass, Disney: every step is the fresh scene under all four integrators,
    and the original record brings the original bits back"""
    b, green = all_matte_dragon(gpu)
    class_changing_edits(gpu, b, green, gpu.Scene(b), lambda **kw: fresh_scene(gpu, b, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["volume", "smooth"])
def test_none_and_back(gpu, which):
    """A GNXR_MAT_NONE material (the medium boundaries) becomes Matte, a Matte one (walls) becomes NONE, under VolPath; ids and albedo of
    RenderAOV are the fresh scene's (-1 and 0 where the surface lost its material)"""
    b = scenes.volume_cornell() if which == "volume" else scenes.smooth_cornell(TEX)
    none = b.add_material(type=A.MAT_NONE)
    d = b.desc()
    ids = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
    boundary = ids < 0
    assert boundary.any()
    ids[boundary] = none
    ids0 = tri_materials(b)
    wall = int(ids0[0])   # a Cornell wall's Matte (the box comes first)
    mats0 = desc_materials(gpu, b)
    assert mats0[wall].type == A.MAT_MATTE
    scene = gpu.Scene(b)
    vol = gpu.VolPathIntegrator(5, 1.0, "spatial")
    img0, _ = vol.Render(scene, W, H, SPP)
    # boundary -> Matte
    mats = with_record(mats0, none, gpu.material(type=A.MAT_MATTE, kd=(0.2, 0.6, 0.7), sigma=0.0))
    scene.update_materials([mats[none]], none)
    fresh = fresh_scene(gpu, b, materials=mats)
    shown, _ = same_everything(gpu, scene, fresh, ("volpath", "path"))
    assert (shown[boundary] == none).all()
    # and a wall -> NONE in the same scene
    mats = with_record(mats, wall, gpu.material(type=A.MAT_NONE))
    scene.update_materials([mats[wall]], wall)
    fresh = fresh_scene(gpu, b, materials=mats)
    shown, cls = same_everything(gpu, scene, fresh, ("volpath",))
    assert (shown[ids0 == wall] == -1).all() and (cls[ids0 == wall] == 0).all()
    f = same_aov(gpu, scene, fresh, spp=1)   # one sample per pixel: the albedo is that sample's, as the ids are
    lost = (f["ids"][..., 0] >= 0) & (f["ids"][..., 1] == -1)
    assert lost.any() and (f["albedo"][..., :3][lost] == 0).all()
    # back
    scene.update_materials([mats0[none]], none)
    scene.update_materials([mats0[wall]], wall)
    assert biteq(vol.Render(scene, W, H, SPP)[0], img0)


HOWS = ["numpy", "tensor_on_stream", "sub_range"]


def reassign(scene, how, ids0, nm):
    """every other dragon triangle moves to material 1: from numpy, from a device tensor written on a non-default stream passed as stream,
    or over a sub-range with first_triangle > 0.  Returns the scene's tri_material afterwards."""
    ids = every_other(ids0, nm, 1)
    if how == "numpy":
        scene.set_triangle_materials(ids)
    elif how == "tensor_on_stream":
        dev = torch.device("cuda", scene.device)
        st = torch.cuda.Stream(dev)
        host = torch.from_numpy(ids).pin_memory()
        with torch.cuda.stream(st):
            t = torch.empty(len(ids), dtype=torch.int32, device=dev)
            t.copy_(host, non_blocking=True)
        scene.set_triangle_materials(t, stream=st)
    else:
        first = 301
        ids = ids0.copy()
        ids[first:nm:2] = 1
        scene.set_triangle_materials(ids[first:nm], first_triangle=first)
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("how", HOWS)
def test_reassignment(gpu, how):
    """every other dragon triangle moves to another material (the red Matte): from numpy, from a device tensor written on a non-default
    stream, over a sub-range with first_triangle > 0"""
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = integ.Render(scene, W, H, SPP)
    ids = reassign(scene, how, tri_materials(b), model_triangle_count(gpu))
    same_everything(gpu, scene, fresh_scene(gpu, b, tri_material=ids), ("path",), expect=ids)
    assert not biteq(integ.Render(scene, W, H, SPP)[0], before)


def same_tree(scene, fresh):
    diff = thb.first_difference(scene.bvh(), fresh.bvh())
    assert diff is None, diff
    (na, ra, sa), (nb, rb, sb) = scene.bvh4(), fresh.bvh4()
    assert (ra, sa) == (rb, sb) and np.array_equal(na, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["classes"] + HOWS)
def test_after_rebuild(gpu, what):
    """deform, rebuild (the leaf order now exists only on the device), then the class-changing edits of test_class_changing_edits or one of
    the reassignments of test_reassignment on the rebuilt handle: a fresh HLBVH scene over the same vertices and edits, the tree included"""
    b, green = all_matte_dragon(gpu)
    nv, nm = model_vertex_count(gpu, MESH2K), model_triangle_count(gpu)
    v2 = deform(vertices(b), nv, seed=5, amount=0.05)
    scene = gpu.Scene(b)
    scene.update_vertices(v2[:nv])
    scene.rebuild_bvh()
    fresh_of = lambda **kw: fresh_scene(gpu, b, verts=v2, split="hlbvh", **kw)
    if what == "classes":
        class_changing_edits(gpu, b, green, scene, fresh_of)
        fresh = fresh_of()
    else:
        ids = reassign(scene, what, tri_materials(b), nm)
        fresh = fresh_of(tri_material=ids)
        same_everything(gpu, scene, fresh, ("path",), expect=ids)
    same_tree(scene, fresh)


def bsdf_rows(scene, seed=3, n=4096):
    dev = torch.device("cuda", scene.device)
    rng = np.random.default_rng(seed)
    rays = torch.from_numpy(scenes.random_rays(n, seed=seed)).to(dev)
    wi = rng.normal(size=(n, 3)).astype(np.float32)
    wi /= np.linalg.norm(wi, axis=1, keepdims=True).astype(np.float32)
    u = rng.random((n, 2), dtype=np.float32)
    out = scene.bsdf(rays, torch.from_numpy(wi).to(dev), torch.from_numpy(u).to(dev))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@pytest.mark.gpu
def test_attribute_copies(gpu):
    """smooth_cornell (per-corner normals, uvs, tangents): the material a smooth mesh uses is edited, then its triangles move to a
    material no triangle with attributes of its own used before"""
    b = scenes.smooth_cornell(TEX)
    d = b.desc()
    ids0 = tri_materials(b)
    mats0 = desc_materials(gpu, b)
    mirror = next(i for i, m in enumerate(mats0) if m.type == A.MAT_MIRROR)
    red = 1
    assert mats0[red].type == A.MAT_MATTE and d.tri_n
    scene = gpu.Scene(b)

    def check(fresh, expect):
        same_everything(gpu, scene, fresh, ("path", "whitted"), expect=expect)
        rows = bsdf_rows(scene)
        assert biteq(rows, bsdf_rows(fresh)) and (rows[:, 13] == 1).any()

    shown0, cls0 = scene.triangle_materials()
    assert (cls0[ids0 == mirror] == 3).all() and (cls0[ids0 == red] == 0).all()
    mats = with_record(mats0, mirror, gpu.material(type=A.MAT_PLASTIC, kd=(0.6, 0.2, 0.2), ks=(0.4, 0.4, 0.4), urough=0.2, vrough=0.2, remap_roughness=1))
    scene.update_materials([mats[mirror]], mirror)
    check(fresh_scene(gpu, b, materials=mats), ids0)
    ids = ids0.copy()
    ids[ids0 == mirror] = red   # the red wall's Matte gets its first attribute copy
    scene.set_triangle_materials(ids)
    check(fresh_scene(gpu, b, materials=mats, tri_material=ids), ids)
    assert (scene.triangle_materials()[1][ids0 == mirror] == 3).all()


@pytest.mark.gpu
def test_textures(gpu):
    """textured_cornell: a Matte gains and loses kd_texture, under Path and Whitted; Li's GNXR_ERR_UNSUPPORTED rule for Whitted on a textured
    scene follows the edited scene as it follows a fresh one"""
    b = scenes.textured_cornell(TEX, glass_sheet=False)
    mats0 = desc_materials(gpu, b)
    textured = [i for i, m in enumerate(mats0) if m.kd_texture or m.ks_texture]
    plain = [m for m in mats0]
    for i in textured:   # the scene without any textured material: same records, references cleared
        m = gpu.Material()
        C.memmove(C.byref(m), C.byref(mats0[i]), C.sizeof(gpu.Material))
        m.kd_texture = m.ks_texture = 0
        plain[i] = m
    floor = next(i for i in textured if mats0[i].type == A.MAT_MATTE)
    scene = gpu.Scene(b)
    wh = gpu.WhittedIntegrator(5)
    rays, samples = cam_batch(b.desc().camera, 1, b.desc().camera_medium, w=16, h=12)

    def li_ok(s):
        try:
            wh.Li(s, rays, samples, 16, 12, 1)
            torch.cuda.synchronize()
            return True
        except gpu.GnxrError as e:
            assert f"error {ERR_UNSUPPORTED}" in str(e)
            return False

    assert not li_ok(scene)
    scene.update_materials([plain[i] for i in range(len(plain))])     # loses every texture
    fresh = fresh_scene(gpu, b, materials=plain)
    same_everything(gpu, scene, fresh, ("path", "whitted"))
    assert li_ok(scene) and li_ok(fresh)
    gains = with_record(plain, floor, mats0[floor])                      # the floor's Matte gains its kd_texture again
    scene.update_materials([gains[floor]], floor)
    fresh = fresh_scene(gpu, b, materials=gains)
    same_everything(gpu, scene, fresh, ("path", "whitted"))
    assert not li_ok(scene) and not li_ok(fresh)
    scene.update_materials(mats0)
    same_everything(gpu, scene, gpu.Scene(b), ("path", "whitted"))


@pytest.mark.gpu
def test_sphere_material_changes_class(gpu):
    b = scenes.cornell_sphere("matte")
    mats0 = desc_materials(gpu, b)
    ball = len(mats0) - 1
    scene = gpu.Scene(b)
    for rec in class_steps(gpu)[:2] + [gpu.material(type=A.MAT_NONE)]:
        mats = with_record(mats0, ball, rec)
        scene.update_materials([rec], ball)
        fresh = fresh_scene(gpu, b, materials=mats)
        for it in integrators(gpu, ("path", "whitted", "volpath")):
            same_render(gpu, it, scene, fresh, W, H, SPP)
        same_aov(gpu, scene, fresh)


@pytest.mark.gpu
def test_refusals(gpu):
    """GNXR_ERR_INVALID, and a render afterwards has the bits of a render before"""
    b = scenes.textured_cornell(TEX, glass_sheet=False)
    d = b.desc()
    nm, nt, ntex = d.n_materials, d.n_triangles, d.n_textures
    mats0 = desc_materials(gpu, b)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    img0, _ = integ.Render(scene, W, H, SPP)
    tm0 = scene.triangle_materials()
    ok = gpu.material(type=A.MAT_GLASS, kr=(0.9,) * 3, kt=(0.9,) * 3, eta=(1.5, 0, 0))
    lib, h = gpu.lib(), scene._h
    arr = lambda ms: (gpu.Material * len(ms))(*ms)
    for first, n in ((nm, 1), (nm - 1, 2), (-1, 1), (0, -1)):
        assert lib.gnxr_scene_update_materials(h, first, n, arr([ok, ok])) == ERR_INVALID
    assert lib.gnxr_scene_update_materials(h, 0, 1, None) == ERR_INVALID
    # a refusal in the middle of a multi-record update leaves all records old
    assert lib.gnxr_scene_update_materials(h, 0, 3, arr([ok, gpu.material(type=99), ok])) == ERR_INVALID
    assert lib.gnxr_scene_update_materials(h, 0, 3, arr([ok, ok, gpu.material(type=A.MAT_MATTE, kd=(0.5,) * 3, kd_texture=ntex + 1)])) == ERR_INVALID
    ids = np.zeros(nt, np.int32)
    p = C.c_void_p(ids.ctypes.data)
    for first, n in ((nt, 1), (1, nt), (-1, 1), (0, -1)):
        assert lib.gnxr_scene_set_triangle_materials(h, first, n, p, None) == ERR_INVALID
    assert lib.gnxr_scene_set_triangle_materials(h, 0, 1, None, None) == ERR_INVALID
    bad = np.zeros(nt, np.int32)
    bad[nt // 2] = nm   # hidden in the middle of a device tensor
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.set_triangle_materials(torch.from_numpy(bad).to(f"cuda:{scene.device}"))
    bad[nt // 2] = -2
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        scene.set_triangle_materials(bad)
    assert lib.gnxr_scene_update_materials(h, 0, 0, None) == 0 and lib.gnxr_scene_set_triangle_materials(h, 0, 0, None, None) == 0
    img1, _ = integ.Render(scene, W, H, SPP)
    assert biteq(img1, img0)
    for x, y in zip(scene.triangle_materials(), tm0):
        assert np.array_equal(x, y)
    same_everything(gpu, scene, gpu.Scene(b), ("path",))
    assert len(mats0) == nm


@pytest.mark.gpu
def test_identity(gpu):
    """re-sending the current records and the current tri_material changes no bit"""
    b = scenes.smooth_cornell(TEX)
    scene = gpu.Scene(b)
    its = integrators(gpu, ("path", "volpath"))
    img0 = [it.Render(scene, W, H, SPP) for it in its]
    tm0 = scene.triangle_materials()
    scene.update_materials(desc_materials(gpu, b))
    scene.set_triangle_materials(tri_materials(b))
    for it, (img, st) in zip(its, img0):
        img1, st1 = it.Render(scene, W, H, SPP)
        assert biteq(img1, img) and (st["rays_closest"], st["rays_any"]) == (st1["rays_closest"], st1["rays_any"])
    for x, y in zip(scene.triangle_materials(), tm0):
        assert np.array_equal(x, y)
    same_aov(gpu, scene, gpu.Scene(b))


@pytest.mark.gpu
def test_reserved_state_and_light_table_stay(gpu):
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    mats0 = desc_materials(gpu, b)
    glass = next(i for i, m in enumerate(mats0) if m.type == A.MAT_GLASS)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "power")
    integ.Reserve(scene, W, H, SPP)
    _, st0 = integ.Render(scene, W, H, SPP)
    table0 = scene.light_grid_table("power")
    rec0 = light_records(scene, b.desc().n_lights)
    # another smooth glass: the same kernel classes
    scene.update_materials([gpu.material(type=A.MAT_GLASS, kr=(0.7, 0.9, 0.8), kt=(0.9, 0.8, 0.7), eta=(1.33, 0, 0), urough=0.0, vrough=0.0)], glass)
    scene.set_triangle_materials(every_other(tri_materials(b), model_triangle_count(gpu), glass))
    _, st1 = integ.Render(scene, W, H, SPP)
    assert st1["state_bytes"] == st0["state_bytes"]
    assert biteq(scene.light_grid_table("power"), table0) and biteq(light_records(scene, b.desc().n_lights), rec0)


@pytest.mark.gpu
def test_edit_sequence_on_replicas(gpu):
    """Device 0 listed twice: material type change, reassignment, vertex update, rebuild, material change; the sharded render (rows are dealt
    over both copies) equals a fresh scene"""
    b, green = all_matte_dragon(gpu)
    nv, nm = model_vertex_count(gpu, MESH2K), model_triangle_count(gpu)
    steps = class_steps(gpu)
    mats0 = desc_materials(gpu, b)
    ids = every_other(tri_materials(b), nm, 1)
    v2 = deform(vertices(b), nv, seed=8, amount=0.05)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        integ.Render(multi, 16, 12, 1)
        multi.update_materials([steps[1]], green)
        multi.set_triangle_materials(ids)
        same_render(gpu, integ, multi, fresh_scene(gpu, b, materials=with_record(mats0, green, steps[1]), tri_material=ids), W, H, SPP)
        multi.update_vertices(v2[:nv])
        multi.rebuild_bvh()
        multi.update_materials([steps[0]], green)
        fresh = fresh_scene(gpu, b, verts=v2, materials=with_record(mats0, green, steps[0]), tri_material=ids, split="hlbvh")
        same_render(gpu, integ, multi, fresh, W, H, SPP)
        same_triangle_materials(multi, fresh, ids)
    finally:
        gpu.init(0)
