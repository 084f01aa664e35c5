"""Editing a scene in place: gnxr_scene_update_vertices (device refit of the BVH over moved vertices) and gnxr_scene_set_camera.

A refit keeps the tree's topology and primitive order and recomputes its boxes as unions of primitive bounds, which is exactly the
LinearBVHNode[] BVHAccel holds for that topology over the new vertices.  The oracle is therefore handed the deformed description and
the device's exported tree (OracleScene.set_bvh) and must agree bit for bit: hit records, images and ray counts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import GOLDEN

MESH2K = os.path.join(GOLDEN, "mesh_2k.3d")
ENV = os.path.join(GOLDEN, "env_100x50.hdr")
ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


# ---------------------------------------------------------------- helpers
class Deformed:
    """The builder's description with `vertices` pointing at another array of the same length (kept alive here)."""

    def __init__(self, builder, verts):
        self.builder = builder
        self.verts = np.ascontiguousarray(verts, np.float32)
        assert self.verts.shape == (builder.desc().n_vertices, 3)

    def desc(self):
        d = self.builder.desc()
        d.vertices = self.verts.ctypes.data_as(C.POINTER(C.c_float))
        return d


def vertices(b):
    d = b.desc()
    return np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).copy()


def indices(b):
    d = b.desc()
    return np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).copy()


def emissive_vertices(b):
    d = b.desc()
    light = np.ctypeslib.as_array(d.tri_light, shape=(d.n_triangles,))
    return np.unique(indices(b)[light >= 0])


def model_vertex_count(gx, path):
    b = gx.SceneBuilder()
    b.AddModel(path, b.MatteMaterial(scenes.WHITE, 60.0))
    return b.desc().n_vertices


def deform(v, n, seed, amount=0.03, shift=(0.11, -0.07, 0.09)):
    """Vertices [0, n) displaced by seeded noise of `amount` x the extent of the set, plus a translation."""
    rng = np.random.default_rng(seed)
    out = v.copy()
    ext = float((v[:n].max(0) - v[:n].min(0)).max())
    out[:n] += (rng.normal(size=(n, 3)) * amount * ext + np.asarray(shift)).astype(np.float32)
    return out.astype(np.float32)


def oracle_on(b, verts, scene):
    o = ol.OracleScene(Deformed(b, verts))
    o.set_bvh(*scene.bvh())
    return o


def numpy_refit(meta, order, tri_verts):
    """Bounds of every node of a flattened BVH over triangles tri_verts [n_tris, 3, 3] (authoring order): leaves are the min / max of their
    triangles' corners, interior nodes the union of their two children (node i + 1 and meta[i, 0])."""
    tlo, thi = tri_verts.min(axis=1), tri_verts.max(axis=1)
    out = np.zeros((len(meta), 6), np.float32)
    for i in range(len(meta) - 1, -1, -1):   # children come after their parent in the depth-first layout
        off, n = meta[i, 0], meta[i, 1]
        if n > 0:
            prims = order[off:off + n]
            out[i, :3], out[i, 3:] = tlo[prims].min(0), thi[prims].max(0)
        else:
            a, c = out[i + 1], out[off]
            out[i, :3], out[i, 3:] = np.minimum(a[:3], c[:3]), np.maximum(a[3:], c[3:])
    return out


def same_render(gx, integ, s1, s2, W, H, spp):
    i1, st1 = integ.Render(s1, W, H, spp)
    i2, st2 = integ.Render(s2, W, H, spp) if isinstance(s2, gx.Scene) else s2.render(integ, W, H, spp)
    assert (st1["rays_closest"], st1["rays_any"]) == (st2["rays_closest"], st2["rays_any"])
    assert biteq(i1[..., :3], i2[..., :3]) and i1[..., :3].any()
    return i1


def dragon(gx, split="sah", env=None):
    b = scenes.dragon_cornell(2000, "glass+metal", env=env, mesh_path=MESH2K)
    b.set_bvh_split_method(split)
    return b, model_vertex_count(gx, MESH2K)


# ---------------------------------------------------------------- CPU
def test_update_entry_points_exported(gx):
    lib = C.CDLL(gx.LIB_PATH)
    assert hasattr(lib, "gnxr_scene_update_vertices") and hasattr(lib, "gnxr_scene_set_camera")


def test_update_entry_points_reject_null_scene(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    xyz = np.zeros((4, 3), np.float32)
    assert gx.lib().gnxr_scene_update_vertices(None, 0, 4, C.c_void_p(xyz.ctypes.data), None) == ERR_INVALID
    assert gx.lib().gnxr_scene_update_vertices(None, 0, 0, None, None) == ERR_INVALID
    cam = gx.Camera((C.c_float * 3)(0, 0, 5), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, 1, 0), 60.0, 0.0, 3.0, 0)
    assert gx.lib().gnxr_scene_set_camera(None, C.byref(cam), -1) == ERR_INVALID


def test_update_vertices_rejects_other_inputs_before_the_library(gx):
    """Only float32 (n, 3) numpy arrays and device tensors are accepted; anything else raises ValueError before a library call (the
    handle here is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_vertices = None, 0, 8
    for bad in ([[0.0, 0.0, 0.0]], np.zeros((2, 3), np.float64), np.zeros(6, np.float32), np.zeros((2, 4), np.float32), "xyz"):
        with pytest.raises(ValueError):
            s.update_vertices(bad)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh"])
def test_refit_boxes_exact(gpu, split):
    """After an update the tree keeps its nodes' meta and the primitive order; its bounds are the numpy recomputation over the new vertices."""
    b, nv = dragon(gpu, split)
    scene = gpu.Scene(b)
    b0, m0, o0 = scene.bvh()
    v = vertices(b)
    v2 = deform(v, nv, seed=1)
    scene.update_vertices(v2[:nv])
    b1, m1, o1 = scene.bvh()
    assert (m1 == m0).all() and (o1 == o0).all()
    ref = numpy_refit(m1, o1, v2[indices(b)])
    assert np.array_equal(b1, ref)
    assert not np.array_equal(b1, b0)
    # re-sending the original vertices gives back the tree the build made
    scene.update_vertices(v[:nv])
    b2, _, _ = scene.bvh()
    assert np.array_equal(b2, b0) and (biteq(b2, b0) or split == "hlbvh")   # (the HLBVH build takes fminf / fmaxf: only a zero's sign may differ)


@pytest.mark.gpu
def test_refit_ray_queries_match_oracle(gpu):
    b, nv = dragon(gpu)
    scene = gpu.Scene(b)
    v2 = deform(vertices(b), nv, seed=2)
    scene.update_vertices(v2[:nv])
    o = oracle_on(b, v2, scene)
    rays = scenes.random_rays(1 << 20, seed=11)
    gh, oh = scene.Intersect(rays), o.Intersect(rays)
    assert (gh["prim"] == oh["prim"]).all()
    m = oh["prim"] >= 0
    for f in ("t", "b0", "b1", "b2", "n"):
        assert biteq(gh[f][m], oh[f][m]), f
    assert (scene.IntersectP(rays) == o.IntersectP(rays)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["path", "whitted", "direct"])
def test_refit_render_matches_oracle(gpu, integ):
    b, nv = dragon(gpu)
    scene = gpu.Scene(b)
    it = {"path": gpu.PathIntegrator(5, 1.0, "spatial"), "whitted": gpu.WhittedIntegrator(5), "direct": gpu.DirectLightingIntegrator("all", 5)}[integ]
    before, _ = it.Render(scene, 64, 48, 4)
    v2 = deform(vertices(b), nv, seed=3)
    scene.update_vertices(v2[:nv])
    after = same_render(gpu, it, scene, oracle_on(b, v2, scene), 64, 48, 4)
    assert not biteq(after, before)


@pytest.mark.gpu
def test_refit_volpath_moved_medium_boundary(gpu):
    """volume_cornell: the HomogeneousMedium's null-material box (its last 8 vertices) moved by a sub-range update."""
    b = scenes.volume_cornell()
    scene = gpu.Scene(b)
    v = vertices(b)
    n = len(v)
    v2 = v.copy()
    v2[n - 8:] += np.array([-0.35, 0.2, 0.15], np.float32)
    scene.update_vertices(v2[n - 8:], first_vertex=n - 8)
    same_render(gpu, gpu.VolPathIntegrator(5, 1.0, "spatial"), scene, oracle_on(b, v2, scene), 64, 48, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["power", "spatial"])
def test_refit_grows_world_bound_env_and_distant_light(gpu, strategy):
    """An infinite and a distant light: the model is moved partly out of the box so that the world bound grows.  A stale environment
    radius, distant-light radius or light-selection table would change the image."""
    b, nv = dragon(gpu, env=ENV)
    b.AddDistLight()
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, strategy)
    integ.Render(scene, 16, 12, 1)   # the light table of the old bound exists before the update
    lo0, hi0 = scene.bvh()[0][0, :3].copy(), scene.bvh()[0][0, 3:].copy()
    v2 = deform(vertices(b), nv, seed=4, shift=(0.5, 0.8, 3.0))
    scene.update_vertices(v2[:nv])
    root = scene.bvh()[0][0]
    assert (root[:3] < lo0).any() or (root[3:] > hi0).any()
    same_render(gpu, integ, scene, oracle_on(b, v2, scene), 64, 48, 4)


@pytest.mark.gpu
def test_refit_cfg3_size(gpu):
    """The 100 k-triangle cfg 3 scene deformed, 256 x 144 at 2 spp."""
    b = scenes.dragon_cornell(100000, "glass+metal")
    nv = model_vertex_count(gpu, scenes.synthetic_mesh_path(100000))
    scene = gpu.Scene(b)
    v2 = deform(vertices(b), nv, seed=5, amount=0.02)
    scene.update_vertices(v2[:nv])
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), scene, oracle_on(b, v2, scene), 256, 144, 2)


@pytest.mark.gpu
def test_refit_sequence(gpu):
    """Three successive updates (a refit of a refit of a refit) against the oracle on the last vertices."""
    b, nv = dragon(gpu)
    scene = gpu.Scene(b)
    v = vertices(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    for k in range(3):
        v = deform(v, nv, seed=10 + k, amount=0.02, shift=(0.05 * k, -0.04, 0.03))
        scene.update_vertices(v[:nv])
        integ.Render(scene, 16, 12, 1)
    bounds, meta, order = scene.bvh()
    assert np.array_equal(bounds, numpy_refit(meta, order, v[indices(b)]))
    same_render(gpu, integ, scene, oracle_on(b, v, scene), 64, 48, 4)


@pytest.mark.gpu
def test_refit_from_device_tensor(gpu):
    """A float32 tensor on the scene's device (read on the current torch stream) gives the tree and image of the same values from numpy."""
    b, nv = dragon(gpu)
    v2 = deform(vertices(b), nv, seed=6)
    s_np, s_dev = gpu.Scene(b), gpu.Scene(b)
    s_np.update_vertices(v2[:nv])
    t = torch.from_numpy(v2[:nv]).to("cuda:0")
    s_dev.update_vertices(t)
    for x, y in zip(s_np.bvh(), s_dev.bvh()):
        assert biteq(x, y) if x.dtype == np.float32 else (x == y).all()
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s_np, s_dev, 64, 48, 4)
    with pytest.raises(ValueError):
        s_dev.update_vertices(t.double())
    with pytest.raises(ValueError):
        s_dev.update_vertices(t.t().contiguous().t())   # (n, 3) but not contiguous


@pytest.mark.gpu
def test_refit_sub_range_equals_full_update(gpu):
    b, nv = dragon(gpu)
    v = vertices(b)
    v2 = deform(v, nv, seed=7)
    lo, hi = nv // 3, 2 * nv // 3
    full = v.copy()
    full[lo:hi] = v2[lo:hi]
    s_full, s_sub = gpu.Scene(b), gpu.Scene(b)
    s_full.update_vertices(full)   # every vertex, the light's with their own values
    s_sub.update_vertices(v2[lo:hi], first_vertex=lo)
    assert biteq(s_full.bvh()[0], s_sub.bvh()[0])
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s_full, s_sub, 64, 48, 4)
    same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s_sub, oracle_on(b, full, s_sub), 64, 48, 4)


@pytest.mark.gpu
def test_refit_identity(gpu):
    """Re-sending the current vertices leaves the tree and the image bit-identical."""
    b, _ = dragon(gpu)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    before, st0 = integ.Render(scene, 64, 48, 4)
    b0 = scene.bvh()[0]
    scene.update_vertices(vertices(b))
    assert biteq(scene.bvh()[0], b0)
    after, st1 = integ.Render(scene, 64, 48, 4)
    assert biteq(after, before) and (st0["rays_closest"], st0["rays_any"]) == (st1["rays_closest"], st1["rays_any"])


@pytest.mark.gpu
def test_refit_refusals(gpu):
    """A moved vertex of the area light is refused (GNXR_ERR_UNSUPPORTED) and leaves the scene as it was; ranges outside the vertex
    array are GNXR_ERR_INVALID."""
    b, nv = dragon(gpu)
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    before, _ = integ.Render(scene, 64, 48, 4)
    b0 = scene.bvh()[0]
    v = vertices(b)
    v2 = deform(v, nv, seed=8)
    lv = emissive_vertices(b)
    assert len(lv) and lv.min() >= nv
    v2[lv[0], 1] -= 0.25
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        scene.update_vertices(v2)
    assert biteq(scene.bvh()[0], b0)
    after, _ = integ.Render(scene, 64, 48, 4)
    assert biteq(after, before)
    n = len(v)
    for first, cnt in ((-1, 4), (n - 2, 4), (n, 1)):
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
            scene.update_vertices(v[:cnt], first_vertex=first)
    assert gpu.lib().gnxr_scene_update_vertices(scene._h, 0, 4, None, None) == ERR_INVALID


CAMERAS = {"moved": dict(eye=(1.2, 0.6, 4.4), look=(-0.2, -0.4, 0.0), fov=55.0),
           "lens": dict(eye=(0.3, 0.2, 4.8), look=(0.0, -0.5, 0.0), fov=50.0, lens_radius=0.08, focal_distance=4.5),
           "ortho": dict(eye=(0.0, 0.4, 5.0), look=(0.0, 0.0, 0.0), orthographic=True),
           "fog": dict(eye=(-0.8, 0.3, 4.6), look=(0.2, -0.2, 0.0), fov=65.0),
           "fog_out": dict(eye=(-0.8, 0.3, 4.6), look=(0.2, -0.2, 0.0), fov=65.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["moved", "lens", "ortho", "fog", "fog_out"])
def test_set_camera_equals_fresh_scene(gpu, kind):
    """After set_camera the render is that of a scene created with that camera."""
    cam = CAMERAS[kind]
    fog = kind.startswith("fog")
    b = scenes.cornell_in_fog() if fog else scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    medium = -1 if kind == "fog_out" else (0 if fog else -1)
    scene = gpu.Scene(b)
    scene.set_camera(**cam, medium=medium)
    b.set_camera(**cam)
    if fog:
        b.set_camera_medium(medium)
    integ = gpu.VolPathIntegrator(5, 1.0, "spatial") if fog else gpu.PathIntegrator(5, 1.0, "spatial")
    same_render(gpu, integ, scene, gpu.Scene(b), 64, 48, 4)
    if fog:
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
            scene.set_camera(**cam, medium=5)


@pytest.mark.gpu
def test_refit_on_replicas(gpu):
    """Device 0 listed twice (every scene is replicated, rows are dealt over the replicas): an update reaches both copies."""
    b, nv = dragon(gpu, env=ENV)
    v2 = deform(vertices(b), nv, seed=9, shift=(0.3, 0.2, 2.5))
    integ, (W, H, spp) = gpu.PathIntegrator(5, 1.0, "spatial"), (64, 48, 4)
    single = gpu.Scene(b)
    single.update_vertices(v2[:nv])
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        integ.Render(multi, 16, 12, 1)
        multi.update_vertices(v2[:nv])
        same_render(gpu, integ, multi, single, W, H, spp)
    finally:
        gpu.init(0)


@pytest.mark.gpu
def test_edit_sequence_on_replicas(gpu):
    """Device 0 listed twice: every editing call, one after the other, leaves the replicated scene where it leaves a scene on one device.
    Both copies render (rows are dealt over them), so a camera, a light record or a tree that stayed behind on the second copy shows as
    every other row differing; the host scene the copies share must end as the single scene's."""
    from test_light_update import desc_lights, light_records, move_light   # (that module imports this one)
    b, nv = dragon(gpu, env=ENV)
    v2 = move_light(deform(vertices(b), nv, seed=21, shift=(0.3, 0.2, 2.5)), emissive_vertices(b))
    v3 = deform(v2, nv, seed=22)
    ls = desc_lights(gpu, b)
    for l in ls[:2]:
        l.le[:] = [2.0, 6.0, 3.0]
    integ, (W, H, spp) = gpu.PathIntegrator(5, 1.0, "spatial"), (64, 48, 4)
    steps = [lambda s: integ.Render(s, 16, 12, 1),
             lambda s: s.set_camera(**CAMERAS["moved"]),
             lambda s: s.update_lights(ls[:2]),
             lambda s: s.update_vertices(v2, move_lights=True),
             lambda s: s.rebuild_bvh(),
             lambda s: s.update_vertices(v3[:nv]),
             lambda s: s.set_camera(**CAMERAS["lens"])]
    single = gpu.Scene(b)
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        for k, step in enumerate(steps, 1):
            step(single)
            step(multi)
            if k in (2, 4, 5, 7):
                same_render(gpu, integ, multi, single, W, H, spp)
        for x, y in zip(single.bvh() + single.bvh4(), multi.bvh() + multi.bvh4()):
            assert biteq(x, y) if getattr(x, "dtype", None) == np.float32 else np.array_equal(x, y)
        assert biteq(light_records(single, len(ls)), light_records(multi, len(ls)))
    finally:
        gpu.init(0)
