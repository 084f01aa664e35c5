"""gnxr_scene_rebuild_bvh: the BVH of a live scene rebuilt on the device over the vertices it holds (csrc/rebuild_kernel.hip.h,
csrc/api_rebuild.hip.h).

The reference of every case is a FRESH scene: the same builder with set_bvh_split_method("hlbvh") and the moved vertices as its
vertices -- code the existing suites pin to the compiled reference.  The small cases are also compared with the numpy restatement
(tests/hlbvh_reference.py).  There are no tolerances: trees, 4-wide node tables, hit records, images, ray counts and traversal counters
are compared bit for bit (binary bounds up to the sign of a zero, the rule of tests/test_hlbvh_build.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded, as in test_scene_update.py)

import hlbvh_reference as hr
import scenes
import test_hlbvh_build as thb
import test_scene_update as tsu

ERR_INVALID = -1
W, H, SPP = 48, 40, 4


# ---------------------------------------------------------------- CPU
def test_rebuild_entry_points_exported(gx):
    lib = C.CDLL(gx.LIB_PATH)
    assert hasattr(lib, "gnxr_scene_rebuild_bvh") and hasattr(lib, "gnxr_scene_bvh4")
    assert "gnxr_scene_rebuild_bvh" in gx._abi.PROTOTYPES and "gnxr_scene_bvh4" in gx._abi.PROTOTYPES


def test_rebuild_rejects_null_scene(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    assert gx.lib().gnxr_scene_rebuild_bvh(None, None) == ERR_INVALID
    n = C.c_int64(0)
    assert gx.lib().gnxr_scene_bvh4(None, None, 0, C.byref(n), None, None) == ERR_INVALID


def test_rebuild_rejects_a_bad_stream_before_the_library(gx):
    """None, a torch stream or a non-negative integer; another type raises TypeError, a negative handle ValueError, before a library
    call (the handle here is empty).  update_vertices takes its stream through the same helper."""
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_vertices = None, 0, 8
    for bad, exc in (("stream", TypeError), (1.5, TypeError), (True, TypeError), ([0], TypeError), (object(), TypeError), (-1, ValueError), (np.int64(-3), ValueError)):
        with pytest.raises(exc):
            s.rebuild_bvh(stream=bad)
        with pytest.raises(exc):
            s.update_vertices(np.zeros((2, 3), np.float32), stream=bad)
    assert gx._stream_handle("t", np.int64(7)) == 7 and gx._stream_handle("t", None) == 0


# ---------------------------------------------------------------- helpers
def soup_builder(gx, v, i, split):
    b = gx.SceneBuilder()
    b.add_mesh(v, i, b.MatteMaterial(scenes.WHITE, 60.0))
    b.set_bvh_split_method(split)
    return b


def fresh_scene(gx, b, verts):
    """the reference: the builder's description with HLBVH and `verts` as its vertices"""
    b.set_bvh_split_method("hlbvh")
    d = tsu.Deformed(b, verts)
    return gx.Scene(d.desc())


def same_tree(got, want):
    diff = thb.first_difference(got, want)
    assert diff is None, diff


def same_scene_tables(a, b):
    """bvh() under the zero-sign rule; bvh4(), root4, stack_need and info() exactly"""
    same_tree(a.bvh(), b.bvh())
    (na, ra, sa), (nb, rb, sb) = a.bvh4(), b.bvh4()
    assert (ra, sa) == (rb, sb), ((ra, sa), (rb, sb))
    assert na.shape == nb.shape and np.array_equal(na, nb), f"4-wide tables differ first at node {int(np.flatnonzero((na != nb).any(axis=1))[0]) if na.shape == nb.shape else -1}"
    assert a.info() == b.info()


def moved(b, seed, amount=0.03):
    """every vertex displaced except those of emissive triangles"""
    v = tsu.vertices(b)
    v2 = tsu.deform(v, len(v), seed, amount=amount)
    ev = tsu.emissive_vertices(b)
    v2[ev] = v[ev]
    return v2


def rebuilt_and_fresh(gx, b, v2, split="sah"):
    """(scene created with `split`, updated to v2 and rebuilt; fresh HLBVH scene over v2)"""
    b.set_bvh_split_method(split)
    s = gx.Scene(b)
    s.update_vertices(v2)
    s.rebuild_bvh()
    return s, fresh_scene(gx, b, v2)


def integrators(gx, names):
    table = {"path": lambda: gx.PathIntegrator(5, 1.0, "spatial"), "whitted": lambda: gx.WhittedIntegrator(5),
             "direct": lambda: gx.DirectLightingIntegrator("all", 5), "volpath": lambda: gx.VolPathIntegrator(5, 1.0, "spatial")}
    return [(n, table[n]()) for n in names]


def same_results(gx, a, b, names=("path", "whitted", "direct", "volpath")):
    """20 000 random rays, a small render per integrator (image and both ray counts) and one RenderAOV with ids"""
    rays = torch.from_numpy(scenes.random_rays(20000, seed=21)).to(f"cuda:{a.device}")
    ha, hb = a.intersect(rays), b.intersect(rays)
    assert torch.equal(ha.hits.view(torch.int32), hb.hits.view(torch.int32))
    assert (ha.prim >= 0).any()
    assert torch.equal(a.occluded(rays), b.occluded(rays))
    for name, it in integrators(gx, names):
        tsu.same_render(gx, it, a, b, W, H, SPP)
    it = gx.PathIntegrator(5, 1.0, "spatial")
    fa, _ = it.RenderAOV(a, W, H, SPP)
    fb, _ = it.RenderAOV(b, W, H, SPP)
    for c in fa:
        assert torch.equal(fa[c].view(torch.int32), fb[c].view(torch.int32)), c
    assert (fa["ids"][..., 0] >= 0).any()


# ---------------------------------------------------------------- GPU: tree equality
# name -> what it is there for (test_hlbvh_build.make_case generates the triangles)
TREE_CASES = {"tiny1": "the root is a leaf, root4 a leaf reference", "tiny2": "one partial DNode4", "tiny3": "partial DNode4", "tiny4": "partial / full DNode4",
              "tiny5": "two levels of DNode4", "tiny3shared": "a multi-primitive leaf", "uniform2047": "sort tile edge", "uniform2048": "sort tile edge",
              "uniform2049": "sort tile edge", "stability": "sort stability, big leaves", "uniform6000": "more than 1024 4-wide nodes",
              "uniform70000": "all 4096 treelets, the second scan tile"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TREE_CASES))
def test_rebuilt_tree_equals_fresh_scene(gpu, name):
    """Created with SAH somewhere else, moved onto the case's vertices, rebuilt: the tree of a fresh HLBVH scene over those vertices, and
    (up to 6000 triangles) the numpy reference's."""
    v2, idx = thb.make_case(name)
    v0 = tsu.deform(v2, len(v2), seed=31, amount=0.05)
    b = soup_builder(gpu, v0, idx, "sah")
    s, fresh = rebuilt_and_fresh(gpu, b, v2)
    same_scene_tables(s, fresh)
    nodes4, root4, need = s.bvh4()
    n = len(idx)
    if name in ("tiny1", "tiny3shared"):
        assert root4 == ~(0 | (n << 24)) and nodes4.shape == (1, 32) and not nodes4.any() and need == 1
    else:
        assert root4 == 0
    if name == "uniform6000":
        assert len(nodes4) > 1024
    if n <= 6000:
        same_tree(s.bvh(), hr.hlbvh_reference(v2, idx))


# ---------------------------------------------------------------- GPU: results
MESH_SEED = 41


@pytest.mark.gpu
def test_rebuilt_dragon_results_equal_fresh_scene(gpu):
    b, nv = tsu.dragon(gpu)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=MESH_SEED, amount=0.2)
    s = gpu.Scene(b)
    s.update_vertices(v2[:nv])
    s.rebuild_bvh()
    fresh = fresh_scene(gpu, b, v2)
    same_scene_tables(s, fresh)
    same_results(gpu, s, fresh, names=("path", "whitted", "direct", "volpath"))


def attr_scene():
    return scenes.smooth_cornell(tsu.os.path.join(tsu.GOLDEN, "tex_smile_96x80.hdr"))


def emissive_scene():
    """the dragon scene plus two emissive meshes (their vertices stay): DLight::tri_leaf read by NEE and by a light hit"""
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=tsu.MESH2K)
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    white = b.MatteMaterial(scenes.WHITE, 60.0)
    b.add_emissive_mesh(np.array([[-2.3, -1.0, -1.0], [-2.3, -1.0, 0.0], [-2.3, 0.0, 0.0], [-2.3, 0.0, -1.0]], np.float32), quad, white, (6.0, 3.0, 1.0))
    b.add_emissive_mesh(np.array([[1.0, -2.3, 1.0], [2.0, -2.3, 1.0], [2.0, -2.3, 2.0], [1.0, -2.3, 2.0]], np.float32), quad[:, ::-1].copy(), white, (1.0, 4.0, 8.0))
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["attributes", "medium", "spheres", "emissive"])
def test_rebuilt_results_with_other_leaf_order_tables(gpu, kind):
    """per-corner uvs / normals / tangents with an image texture; tri_media under VolPath; spheres; two emissive meshes"""
    b = {"attributes": attr_scene, "medium": scenes.volume_cornell, "spheres": lambda: scenes.cornell_sphere("glass"), "emissive": emissive_scene}[kind]()
    v2 = moved(b, seed=43)
    s, fresh = rebuilt_and_fresh(gpu, b, v2)
    same_scene_tables(s, fresh)
    same_results(gpu, s, fresh, names=("path", "volpath") if kind == "medium" else ("path", "whitted", "direct", "volpath"))


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [2, 4])
def test_rebuilt_traversal_work_equals_fresh_scene(gpu, flag):
    """gnxr_set_profiling bit 1 (binary walk) and bit 2 (the 4-wide walk), in runs of their own: a 4-wide tree with the right hits in
    another order or numbering would change the counts"""
    b, nv = tsu.dragon(gpu)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=MESH_SEED, amount=0.2)
    s = gpu.Scene(b)
    s.update_vertices(v2[:nv])
    s.rebuild_bvh()
    fresh = fresh_scene(gpu, b, v2)
    it = gpu.PathIntegrator(5, 1.0, "spatial")
    try:
        gpu.lib().gnxr_set_profiling(flag)
        _, sa = it.Render(s, W, H, SPP)
        _, sb = it.Render(fresh, W, H, SPP)
    finally:
        gpu.lib().gnxr_set_profiling(0)
    keys = ("nodes_visited", "tris_tested", "leaf_retests", "nodes_from_memory")
    print({k: (sa[k], sb[k]) for k in keys})
    assert [sa[k] for k in keys] == [sb[k] for k in keys]
    assert sa["nodes_visited"] > 0 and sa["tris_tested"] > 0


# ---------------------------------------------------------------- GPU: sequences
@pytest.mark.gpu
def test_rebuild_then_update_follows_the_new_tree(gpu):
    """rebuild -> update_vertices -> render == the fresh scene refitted the same way: the refit tables are those of the new tree"""
    b, nv = tsu.dragon(gpu)
    v = tsu.vertices(b)
    v2 = tsu.deform(v, nv, seed=51, amount=0.2)
    v3 = tsu.deform(v2, nv, seed=52)
    s = gpu.Scene(b)
    s.update_vertices(v2[:nv])
    s.rebuild_bvh()
    s.update_vertices(v3[:nv])
    fresh = fresh_scene(gpu, b, v2)
    fresh.update_vertices(v3[:nv])
    same_scene_tables(s, fresh)
    tsu.same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s, fresh, W, H, SPP)


@pytest.mark.gpu
def test_rebuild_is_idempotent(gpu):
    b, nv = tsu.dragon(gpu)
    s = gpu.Scene(b)
    s.update_vertices(tsu.deform(tsu.vertices(b), nv, seed=53, amount=0.2)[:nv])
    s.rebuild_bvh()
    t1, w1 = s.bvh(), s.bvh4()
    s.rebuild_bvh()
    t2, w2 = s.bvh(), s.bvh4()
    for x, y in zip(t1, t2):
        assert x.tobytes() == y.tobytes()
    assert w1[0].tobytes() == w2[0].tobytes() and w1[1:] == w2[1:]


@pytest.mark.gpu
def test_rebuild_after_device_update_on_another_stream(gpu):
    """a device tensor written, sent and rebuilt on one non-default stream, with no synchronisation from the caller in between"""
    b, nv = tsu.dragon(gpu)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=54, amount=0.2)
    s = gpu.Scene(b)
    st = torch.cuda.Stream()
    host = torch.from_numpy(v2[:nv]).pin_memory()
    with torch.cuda.stream(st):
        t = host.to("cuda:0", non_blocking=True)
        s.update_vertices(t)
        s.rebuild_bvh(stream=st)
    fresh = fresh_scene(gpu, b, v2)
    same_scene_tables(s, fresh)
    tsu.same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s, fresh, W, H, SPP)


@pytest.mark.gpu
def test_rebuild_keeps_the_reserved_state(gpu):
    b, nv = tsu.dragon(gpu)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=55, amount=0.2)
    s = gpu.Scene(b)
    it = gpu.PathIntegrator(5, 1.0, "spatial")
    it.Reserve(s, W, H, SPP)
    _, st0 = it.Render(s, W, H, SPP)
    s.update_vertices(v2[:nv])
    s.rebuild_bvh()
    img, st1 = it.Render(s, W, H, SPP)
    assert st1["state_bytes"] == st0["state_bytes"] > 0
    fresh = fresh_scene(gpu, b, v2)
    ref, _ = it.Render(fresh, W, H, SPP)
    assert tsu.biteq(img[..., :3], ref[..., :3])


# ---------------------------------------------------------------- GPU: refusal
@pytest.mark.gpu
def test_rebuild_refusal_leaves_the_scene_untouched(gpu):
    """65 536 triangles moved onto one Morton code (the input check of the build itself, no fault): the error comes back, the scene
    still gives the bits it gave before; moved apart again, the rebuild succeeds and matches a fresh scene"""
    v_bad, idx = thb.make_case("oversized")
    v_ok, _ = thb.uniform(len(idx), 77)
    b = soup_builder(gpu, v_ok, idx, "hlbvh")
    s = gpu.Scene(b)
    s.update_vertices(v_bad)
    it = gpu.PathIntegrator(3, 1.0, "spatial")
    tree0, wide0 = s.bvh(), s.bvh4()
    img0, _ = it.Render(s, 16, 12, 1)
    with pytest.raises(gpu.GnxrError, match="a leaf exceeds 65535 primitives") as e:
        s.rebuild_bvh()
    assert f"error {ERR_INVALID}" in str(e.value)
    tree1, wide1 = s.bvh(), s.bvh4()
    for x, y in zip(tree0, tree1):
        assert x.tobytes() == y.tobytes()
    assert wide0[0].tobytes() == wide1[0].tobytes() and wide0[1:] == wide1[1:]
    img1, _ = it.Render(s, 16, 12, 1)
    assert tsu.biteq(img0, img1)
    v3 = tsu.deform(v_ok, len(v_ok), seed=56, amount=0.01)
    s.update_vertices(v3)
    s.rebuild_bvh()
    same_scene_tables(s, fresh_scene(gpu, b, v3))


# ---------------------------------------------------------------- GPU: replicas
@pytest.mark.gpu
def test_rebuild_on_replicas(gpu):
    """Device 0 listed twice, the way test_scene_update.test_refit_on_replicas runs it: the rebuild reaches both copies"""
    b, nv = tsu.dragon(gpu, env=tsu.ENV)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=57, amount=0.2)
    it = gpu.PathIntegrator(5, 1.0, "spatial")
    single = gpu.Scene(b)
    single.update_vertices(v2[:nv])
    single.rebuild_bvh()
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        it.Render(multi, 16, 12, 1)
        multi.update_vertices(v2[:nv])
        multi.rebuild_bvh()
        tsu.same_render(gpu, it, multi, single, W, H, SPP)
        same_scene_tables(multi, single)
    finally:
        gpu.init(0)
