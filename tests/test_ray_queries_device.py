"""Batched ray queries on device memory: gnxr_trace_closest_device / gnxr_trace_any_device and Scene.intersect / Scene.occluded.

The device calls run the caller's rays through k_trace4 (the render's 4-wide walk) on the caller's stream; per ray their results must be
exactly those of the host entry points gnxr_trace_closest / gnxr_trace_any, which the reference's recorded hits and the oracle pin.
Every comparison here is bit for bit, on whole gnxr_hit records."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import GOLDEN, golden

MESH2K = os.path.join(GOLDEN, "mesh_2k.3d")
ERR_INVALID = -1


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def records(hits):
    """(n, 8) float32 tensor of Scene.intersect -> the structured gnxr_hit records of Scene.Intersect (same bytes)"""
    import gnxraytracer_amd as gx
    return np.ascontiguousarray(hits.cpu().numpy()).view(gx.HIT_DTYPE).reshape(-1)


def same_records(a, b):
    """two gnxr_hit arrays are the same bytes (every field, misses included)"""
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def dquery(scene, rays):
    """closest and any-hit answers of the device path for numpy rays, after the stream has finished"""
    r = dev(rays)
    h = scene.intersect(r)
    o = scene.occluded(r)
    torch.cuda.synchronize()
    return records(h.hits), o.cpu().numpy()


def check_host(scene, rays):
    """device results == the host entry points' on the same rays; returns them"""
    h, o = dquery(scene, rays)
    assert same_records(h, scene.Intersect(rays))
    assert (o == scene.IntersectP(rays)).all()
    return h, o


def check_oracle(h, o, osc, rays):
    """device results == the oracle's Intersect / IntersectP, every field of a hit bit-exact (barycentrics included)"""
    oh = osc.Intersect(rays)
    assert (h["prim"] == oh["prim"]).all()
    m = oh["prim"] >= 0
    for f in ("t", "b0", "b1", "b2", "n"):
        assert biteq(h[f][m], oh[f][m]), f
    assert (o == osc.IntersectP(rays)).all()


def dragon(split="sah"):
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K)
    b.set_bvh_split_method(split)
    return b


def chain_scene(gx, n=36):
    """n small triangles facing +x at x = 2^-k on the x axis: the middle split peels one off per level, so the binary tree is a chain
    n - 1 deep and the 4-wide walk of a ray along the axis keeps a sibling on its stack at every level (k_trace4's SPILL instantiation)."""
    v, idx = [], []
    for k in range(n):
        x, s = 2.0 ** -k, 0.3 * 2.0 ** -k
        v += [(x, -s, -s), (x, s, -s), (x, 0.0, 2 * s)]
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    b = gx.SceneBuilder()
    b.add_mesh(np.array(v, np.float32), np.array(idx, np.int32), b.MatteMaterial(scenes.WHITE, 60.0))
    b.set_bvh_split_method("middle")
    return b


def lds_stack_levels(spheres, blocks_per_cu=5):
    """LDS levels of k_trace4's traversal stack (trace_launch in csrc/api_render.hip.h; the default 5 blocks per CU): the deeper levels spill"""
    fixed = (11 + (1 if spheres else 0)) * 256 * 4 + 64 * 128 + 128   # ray records, top-of-tree cache, order table
    return min(64, max(2, ((160 * 1024) // blocks_per_cu - 1024 - fixed) // (256 * 4)))


def chain_rays(n, seed):
    """rays from near the deep end of chain_scene along and around the axis (some exactly along it: zero direction components)"""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = -(2.0 ** -rng.uniform(0, 40, n))
    o[:, 1:] = rng.normal(size=(n, 2)) * 1e-3 * (2.0 ** -rng.uniform(0, 30, (n, 1)))
    d = np.zeros((n, 3), np.float32)
    d[:, 0] = 1
    d[n // 2:, 1:] = rng.normal(size=(n - n // 2, 2)) * 0.02
    d[n // 4:n // 2, 0] = rng.choice([-1.0, 1.0], n // 2 - n // 4)
    import gnxraytracer_amd as gx
    return gx.make_rays(o, d)


# ---------------------------------------------------------------- CPU
def test_device_query_symbols_exported(gx):
    lib = C.CDLL(gx.LIB_PATH)
    assert hasattr(lib, "gnxr_trace_closest_device") and hasattr(lib, "gnxr_trace_any_device")


def test_device_query_rejects_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0 and n < 0 are refused before anything is looked at (the handle below is a dummy that a
    call must not touch: these checks come first)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    dummy = C.c_void_p(C.addressof(buf))
    for fn in (L.gnxr_trace_closest_device, L.gnxr_trace_any_device):
        assert fn(None, p, 1, p, None) == ERR_INVALID
        assert fn(None, p, 0, p, None) == ERR_INVALID
        assert fn(dummy, None, 4, p, None) == ERR_INVALID
        assert fn(dummy, p, 4, None, None) == ERR_INVALID
        assert fn(dummy, p, -1, p, None) == ERR_INVALID


def test_device_query_rejects_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 8) tensors on the scene's device are accepted; anything else raises ValueError before a library call
    (the handle here is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    bad = [np.zeros((4, 8), np.float32), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 7)), torch.zeros((8, 4)).t(),
           torch.zeros((4, 16))[:, ::2], torch.zeros(32), "rays"]
    for b in bad:
        for fn in (s.intersect, s.occluded):
            with pytest.raises(ValueError):
                fn(b)
    # a CPU tensor of the right shape is on the wrong device
    with pytest.raises(ValueError):
        s.intersect(torch.zeros((4, 8)))


def test_rays_tensor_layout(gx):
    o, d = np.random.default_rng(1).normal(size=(2, 5, 3)).astype(np.float32)
    r = gx.rays_tensor(torch.from_numpy(o), torch.from_numpy(d), 7.5)
    assert r.dtype == torch.float32 and r.shape == (5, 8) and r.is_contiguous()
    assert (r.numpy() == gx.make_rays(o, d, 7.5)).all()
    tm = torch.arange(5, dtype=torch.float32)
    assert (gx.rays_tensor(torch.from_numpy(o), torch.from_numpy(d), tm).numpy() == np.concatenate(
        [gx.make_rays(o[i:i + 1], d[i:i + 1], float(i)) for i in range(5)])).all()


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "mesh2k"])
def test_reference_goldens_through_device_tensors(gpu, name):
    b = scenes.cornell() if name == "cornell" else dragon()
    scene = gpu.Scene(b)
    g = golden(f"hits_{name}.npz")
    hits = scene.intersect(dev(g["rays"]))
    occ = scene.occluded(dev(g["srays"]))
    torch.cuda.synchronize()
    prim, t, n = hits.prim.cpu().numpy(), hits.t.cpu().numpy(), hits.n.cpu().numpy()
    assert (prim == g["prim"]).all()
    m = g["prim"] >= 0
    assert biteq(t[m], g["t"][m]) and biteq(n[m], g["n"][m])
    assert (occ.cpu().numpy() == g["occluded"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tmax", [np.inf, 1.7])
def test_oracle_sweep(gpu, tmax):
    b = dragon()
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    rays = scenes.random_rays(300000, seed=21, tmax=tmax)
    h, o = check_host(scene, rays)
    check_oracle(h, o, osc, rays)
    assert (h["prim"] >= 0).mean() > 0.3 and 0 < o.mean() < 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sphere_matte", "sphere_glass", "smooth"])
def test_spheres_normals_tangents(gpu, kind):
    """Spheres (tested before the BVH, hit code -2 - i) and per-vertex normals / tangents (the geometric normal flipped onto the
    shading side) come out of the finishing pass exactly as from the host entry point."""
    b = scenes.smooth_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr")) if kind == "smooth" else scenes.cornell_sphere(kind.split("_")[1])
    scene = gpu.Scene(b)
    rays = np.concatenate([scenes.random_rays(100000, seed=4), scenes.random_rays(50000, seed=5, tmax=1.5)])
    h, o = check_host(scene, rays)
    check_oracle(h, o, ol.OracleScene(b), rays)
    if kind != "smooth":
        assert (h["prim"] == scene.n_triangles).any()   # the sphere is hit


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts"])
def test_split_methods(gpu, split):
    b = dragon(split)
    scene = gpu.Scene(b)
    osc = ol.OracleScene(b)
    osc.set_bvh(*scene.bvh())   # the oracle walks the device's tree
    rays = scenes.random_rays(100000, seed=7)
    h, o = check_host(scene, rays)
    check_oracle(h, o, osc, rays)


@pytest.mark.gpu
def test_spilling_stack(gpu):
    """A chain-shaped tree whose 4-wide stack outgrows the LDS part: a 4-wide node has at least two children, so the walk down the deepest
    path needs at least one stack entry per 4-wide level, ceil(depth / 2) of them, plus the root's: more than the LDS holds."""
    b = chain_scene(gpu)
    scene = gpu.Scene(b)
    depth = scene.info()["bvh_max_depth"]
    assert (depth + 1) // 2 + 2 > lds_stack_levels(spheres=False), depth
    osc = ol.OracleScene(b)
    osc.set_bvh(*scene.bvh())
    rays = chain_rays(200000, seed=3)
    h, o = check_host(scene, rays)
    check_oracle(h, o, osc, rays)
    assert (h["prim"] >= 20).sum() > 1000   # deep triangles are reached


@pytest.mark.gpu
def test_binary_fallback(gpu):
    """GNXR_BINARY_BVH at scene creation: the scene keeps the reference's binary walk, on the caller's device buffers -- same results."""
    b = dragon()
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(b)
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    rays = scenes.random_rays(100000, seed=8)
    h, o = check_host(scene, rays)
    check_oracle(h, o, ol.OracleScene(b), rays)
    h4, o4 = dquery(gpu.Scene(b), rays)
    assert same_records(h, h4) and (o == o4).all()


@pytest.mark.gpu
def test_edge_cases(gpu):
    b = dragon()
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    rng = np.random.default_rng(12)
    n = 4000
    o = rng.uniform(-2.4, 2.4, (n, 3)).astype(np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, -0.6, 0.8], [0.8, 0, -0.6]], np.float32)
    zero_dir = gpu.make_rays(o, axes[rng.integers(0, len(axes), n)])          # exactly zero direction components (the 0 * inf path)
    t0 = gpu.make_rays(o, rng.normal(size=(n, 3)).astype(np.float32), 0.0)    # tmax = 0
    d = b.desc()
    verts = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3))
    tri = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3))
    pick = tri[rng.integers(0, len(tri), n)]
    edge = 0.5 * (verts[pick[:, 0]] + verts[pick[:, 1]])                       # origins on a triangle edge
    on_edge = gpu.make_rays(edge.astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32))
    away = gpu.make_rays(np.tile([[0, 0, 100]], (64, 1)), np.tile([[0, 0, 1]], (64, 1)))   # outside, leaving the scene
    for rays in (zero_dir, t0, on_edge, away):
        h, oc = check_host(scene, rays)
        check_oracle(h, oc, osc, rays)
    assert (dquery(scene, t0)[0]["prim"] == -1).all() and (dquery(scene, away)[1] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 65, (1 << 22) + 7])
def test_batch_sizes(gpu, n):
    scene = gpu.Scene(dragon())
    rays = scenes.random_rays(n, seed=n % 1000)
    h, o = check_host(scene, rays)
    assert len(h) == n and len(o) == n


@pytest.mark.gpu
def test_pointer_checks(gpu):
    """A (n, 8) view at a 16-byte-aligned offset into a larger tensor is accepted; a misaligned raw pointer, host memory (plain or
    registered) are refused before anything is queued; NULL as the stream is the null stream."""
    scene = gpu.Scene(dragon())
    rays = scenes.random_rays(1000, seed=2)
    big = torch.zeros(4 + rays.size + 12, dtype=torch.float32, device="cuda")
    view = big[4:4 + rays.size].view(-1, 8)
    view.copy_(dev(rays))
    h = scene.intersect(view)
    torch.cuda.synchronize()
    assert same_records(records(h.hits), scene.Intersect(rays))
    L = gpu.lib()
    hits = torch.zeros((1000, 8), dtype=torch.float32, device="cuda")
    occ = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    mis = C.c_void_p(big.data_ptr() + 4)   # 4-byte aligned only
    assert L.gnxr_trace_closest_device(scene._h, mis, 999, C.c_void_p(hits.data_ptr()), None) == ERR_INVALID
    assert L.gnxr_trace_any_device(scene._h, mis, 999, C.c_void_p(occ.data_ptr()), None) == ERR_INVALID
    host_rays, host_hits = np.ascontiguousarray(rays), np.zeros((1000, 8), np.float32)
    assert L.gnxr_trace_closest_device(scene._h, C.c_void_p(host_rays.ctypes.data), 1000, C.c_void_p(hits.data_ptr()), None) == ERR_INVALID
    assert L.gnxr_trace_closest_device(scene._h, C.c_void_p(view.data_ptr()), 1000, C.c_void_p(host_hits.ctypes.data), None) == ERR_INVALID
    pinned = torch.from_numpy(host_rays).pin_memory()
    assert L.gnxr_trace_any_device(scene._h, C.c_void_p(pinned.data_ptr()), 1000, C.c_void_p(occ.data_ptr()), None) == ERR_INVALID
    torch.cuda.synchronize()
    assert (hits == 0).all() and (occ == 0).all()   # nothing was queued by the refused calls
    # the null stream
    assert L.gnxr_trace_any_device(scene._h, C.c_void_p(view.data_ptr()), 1000, C.c_void_p(occ.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (occ.cpu().numpy() == scene.IntersectP(rays)).all()


@pytest.mark.gpu
def test_stream_ordering(gpu):
    """Rays written by torch on a side stream, queried there and reduced there; the host only waits at the end."""
    scene = gpu.Scene(dragon())
    rays = scenes.random_rays(500000, seed=13)
    want_h, want_o = scene.Intersect(rays), scene.IntersectP(rays)
    src = dev(rays)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = torch.empty_like(src)
        r[:, 0:3] = src[:, 0:3] * 1.0
        r[:, 3] = src[:, 3]
        r[:, 4:8] = src[:, 4:8]
        h = scene.intersect(r, stream=side)
        o = scene.occluded(r, stream=side)
        hit_count = (h.prim >= 0).sum()
        occ_count = o.to(torch.int64).sum()
        prim_sum = h.prim.to(torch.int64).sum()
    side.synchronize()
    assert int(hit_count) == int((want_h["prim"] >= 0).sum())
    assert int(prim_sum) == int(want_h["prim"].astype(np.int64).sum())
    assert int(occ_count) == int(want_o.astype(np.int64).sum())
    assert same_records(records(h.hits), want_h) and (o.cpu().numpy() == want_o).all()


@pytest.mark.gpu
def test_two_streams_at_once(gpu):
    scene = gpu.Scene(dragon())
    ra, rb = scenes.random_rays(400000, seed=14), scenes.random_rays(300000, seed=15, tmax=2.0)
    da, db = dev(ra), dev(rb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream()); sb.wait_stream(torch.cuda.current_stream())
    ha, hb = scene.intersect(da, stream=sa), scene.intersect(db, stream=sb)
    oa, ob = scene.occluded(da, stream=sa), scene.occluded(db, stream=sb)
    torch.cuda.synchronize()
    assert same_records(records(ha.hits), scene.Intersect(ra)) and same_records(records(hb.hits), scene.Intersect(rb))
    assert (oa.cpu().numpy() == scene.IntersectP(ra)).all() and (ob.cpu().numpy() == scene.IntersectP(rb)).all()


@pytest.mark.gpu
def test_after_update_vertices(gpu):
    """After a refit the device queries equal the oracle given the deformed description and the device's refitted tree."""
    import test_scene_update as tsu
    b, nv = tsu.dragon(gpu)
    scene = gpu.Scene(b)
    v2 = tsu.deform(tsu.vertices(b), nv, seed=5)
    scene.update_vertices(v2[:nv])
    osc = tsu.oracle_on(b, v2, scene)
    rays = scenes.random_rays(200000, seed=16)
    h, o = check_host(scene, rays)
    check_oracle(h, o, osc, rays)


@pytest.mark.gpu
def test_replicas(gpu):
    """init_devices([0, 0]): the handle holds two copies on device 0; the query runs on one of them with the single-device results."""
    b = dragon()
    rays = scenes.random_rays(200000, seed=17)
    h1, o1 = dquery(gpu.Scene(b), rays)
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        h2, o2 = dquery(multi, rays)
    finally:
        gpu.init(0)
    assert same_records(h1, h2) and (o1 == o2).all()


@pytest.mark.gpu
def test_alongside_a_render(gpu):
    """A query on a side stream while a RenderDevice of the same handle is in flight on another stream: both equal their stand-alone results."""
    b = dragon()
    scene = gpu.Scene(b)
    integ, (W, H, spp) = gpu.PathIntegrator(5, 1.0, "spatial"), (128, 96, 8)
    alone, _ = integ.Render(scene, W, H, spp)
    rays = scenes.random_rays(1 << 20, seed=18)
    want_h, want_o = scene.Intersect(rays), scene.IntersectP(rays)
    r = dev(rays)
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rs, qs = torch.cuda.Stream(), torch.cuda.Stream()
    rs.wait_stream(torch.cuda.current_stream()); qs.wait_stream(torch.cuda.current_stream())
    integ.RenderDevice(scene, img.data_ptr(), W, H, spp, stream=rs.cuda_stream)
    h = scene.intersect(r, stream=qs)
    o = scene.occluded(r, stream=qs)
    torch.cuda.synchronize()
    assert biteq(img.cpu().numpy()[..., :3], alone[..., :3]) and alone[..., :3].any()
    assert same_records(records(h.hits), want_h) and (o.cpu().numpy() == want_o).all()
