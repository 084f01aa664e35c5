"""k_trace4 serves the leaves that its LDS copy of the top 64 nodes references -- in a room, the walls -- from LDS as well (csrc/trace4_kernel.hip.h,
"hot leaves"): the block copies their triangles and boxes from the live device tables at every launch and rewrites the cached nodes' leaf
references to slots of that copy.  A hot triangle is the same 96 bits of corners tested by the same instructions against the same tMax, and
an accepted hit reports the triangle's real leaf-order index, so nothing a caller can see may move: every comparison below is bit for bit,
against the host entry points (k_trace_closest_api: the reference's binary walk, no LDS copy of anything), the oracle, or a freshly built scene.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first)

import oracle_lib as ol
import scenes
import test_ray_queries_device as trq
import test_scene_update as tsu
import test_set_geometry as tsg

W, H, SPP, DEPTH = 64, 48, 2, 5
N_RAYS = 4096
HOT_BYTES = 768   # kHotBytes: 48 B per triangle, 32 B per leaf box


def tri_corners(b):
    """[n_tris, 3, 3] corners of the builder's triangles, authoring order"""
    return tsu.vertices(b)[tsu.indices(b)]


def aimed_rays(gx, corners, per_tri, seed, origin_box=2.2, tmax=np.inf):
    """per_tri rays at seeded interior points of each triangle of `corners` from seeded origins inside the room"""
    rng = np.random.default_rng(seed)
    n = len(corners) * per_tri
    tri = np.repeat(corners, per_tri, axis=0)
    u = rng.uniform(0.02, 0.98, (n, 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    target = tri[:, 0] + u[:, :1] * (tri[:, 1] - tri[:, 0]) + u[:, 1:] * (tri[:, 2] - tri[:, 0])
    o = rng.uniform(-origin_box, origin_box, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return gx.make_rays(o.astype(np.float32), d.astype(np.float32), tmax)


def through_rays(gx, near, far, n, seed):
    """n rays that start outside the room behind a point of a `far` triangle's plane side, pass a `near` triangle first and then reach a `far`
    one: the walk has a hit when it pops the far leaf, whose box is then re-tested against the shrunken tMax"""
    rng = np.random.default_rng(seed)

    def points(corners):
        tri = corners[rng.integers(0, len(corners), n)]
        u = rng.uniform(0.05, 0.95, (n, 2))
        flip = u.sum(1) > 1
        u[flip] = 1 - u[flip]
        return tri[:, 0] + u[:, :1] * (tri[:, 1] - tri[:, 0]) + u[:, 1:] * (tri[:, 2] - tri[:, 0])

    a, c = points(near), points(far)
    d = c - a
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = a - d * rng.uniform(0.05, 0.4, (n, 1))
    return gx.make_rays(o.astype(np.float32), d.astype(np.float32))


def axis_rays(gx, corners, n, seed, in_plane=True):
    """n rays with one or two zero direction components (1 / d infinite: the walk's exact comparison sequence), from inside the room; in_plane:
    a quarter of them start in the plane of a wall, where (plane - o) * (1 / d) is 0 * inf"""
    rng = np.random.default_rng(seed)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, -0.6, 0.8], [0.8, 0, -0.6]], np.float32)
    o = rng.uniform(-2.4, 2.4, (n, 3)).astype(np.float32)
    if in_plane:
        on_wall = corners.reshape(-1, 3)[rng.integers(0, corners.size // 3, n // 4)]
        k = rng.integers(0, 3, n // 4)
        o[np.arange(n // 4), k] = on_wall[np.arange(n // 4), k]   # one coordinate exactly a wall's
    return gx.make_rays(o, axes[rng.integers(0, len(axes), n)])


def check_queries(scene, rays, osc=None):
    """gnxr_trace_closest_device / gnxr_trace_any_device (k_trace4) == the host entry points (the binary walk) on whole records and bytes,
    and == the oracle where one is given; returns the records"""
    h, o = trq.check_host(scene, rays)
    if osc is not None:
        trq.check_oracle(h, o, osc, rays)
    return h, o


def check_render(gpu, scene, osc, integ=None):
    """the frame and both ray counts equal the oracle's"""
    integ = integ or gpu.PathIntegrator(DEPTH, 1.0, "spatial")
    img, st = integ.Render(scene, W, H, SPP)
    oimg, ost = osc.render(integ, W, H, SPP)
    assert (st["rays_closest"], st["rays_any"]) == (ost["rays_closest"], ost["rays_any"])
    assert img[..., :3].any() and trq.biteq(img[..., :3], oimg[..., :3])
    return st


def hot_share(gpu, scene, integ=None):
    """(triangles from LDS, triangles loaded) of one small frame through the counting 4-wide walk"""
    integ = integ or gpu.PathIntegrator(DEPTH, 1.0, "spatial")
    gpu.lib().gnxr_set_profiling(4)
    try:
        integ.Render(scene, W, H, SPP)
    finally:
        gpu.lib().gnxr_set_profiling(0)
    hot, loaded = scene.hot_leaf_counts()
    print(f"hot leaves: {hot} of {loaded} triangles from LDS = {hot / max(1, loaded):.3f}")
    return hot, loaded


def cornell_with_mesh():
    """the plain Cornell box (12 large triangles in two-triangle leaves next to the root) plus the 2 k-triangle model"""
    b = scenes.cornell()
    b.AddModel(tsu.MESH2K, b.MatteMaterial(scenes.DRAGON_GREEN, 60.0))
    return b


def leaf_table(scene):
    """(first triangle, count) of every leaf of the binary tree"""
    _, meta, _ = scene.bvh()[:3]
    m = meta[meta[:, 1] > 0]
    return m[:, 0], m[:, 1]


# ---------------------------------------------------------------- CPU
def test_hot_leaf_counts_exported(gx):
    import ctypes as C
    lib = C.CDLL(gx.LIB_PATH)
    assert hasattr(lib, "gnxr_scene_hot_leaf_counts")
    assert gx.lib().gnxr_scene_hot_leaf_counts(None, None, None) == -1
    assert hasattr(lib, "gnxr_scene_trace_plan")
    assert gx.lib().gnxr_scene_trace_plan(None, 1, None) == -1


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_real_index_comes_back(gpu):
    """Rays at every wall and light triangle and at the mesh: prim, t, barycentrics and the any-hit bytes of the 4-wide walk equal the binary
    walk's and the oracle's; so does a frame, ray counts included.  Rays that hit a mesh triangle first and then pop a wall leaf re-test the
    wall's box from LDS (flat boxes: t == tMax ties among them)."""
    b = cornell_with_mesh()
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    tc = tri_corners(b)
    walls, mesh = tc[:12], tc[12:]
    h, _ = check_queries(scene, aimed_rays(gpu, walls, N_RAYS // 12, seed=1), osc)
    assert set(np.unique(h["prim"])) >= set(range(12))   # every wall and light triangle is reported by its own index
    check_queries(scene, aimed_rays(gpu, walls, N_RAYS // 12, seed=2, tmax=3.0), osc)
    h, _ = check_queries(scene, aimed_rays(gpu, mesh[::4], 8, seed=3), osc)
    assert (h["prim"] >= 12).mean() > 0.5
    rays = trq.scenes.random_rays(N_RAYS, seed=4)
    check_queries(scene, rays, osc)
    h, _ = check_queries(scene, through_rays(gpu, mesh, walls, N_RAYS, seed=5), osc)
    assert (h["prim"] >= 12).mean() > 0.5                 # the mesh is hit first: the wall behind it is popped with a hit in hand
    # corners and edges of the room: the rays' hits lie in several walls' flat boxes at once
    corners = walls.reshape(-1, 3)
    rng = np.random.default_rng(6)
    o = rng.uniform(-1.0, 1.0, (N_RAYS, 3))
    d = corners[rng.integers(0, len(corners), N_RAYS)] - o
    check_queries(scene, gpu.make_rays(o.astype(np.float32), d.astype(np.float32)), osc)   # unnormalised: t == 1 at the corner
    check_render(gpu, scene, osc)
    hot, loaded = hot_share(gpu, scene)
    assert 0 < hot <= loaded


@pytest.mark.gpu
def test_overflow_some_leaves_hot_some_not(gpu):
    """40 large overlapping triangles and 300 small ones inside the Cornell box: the cached nodes reference more leaf bytes than the region
    has, so some leaves are served from LDS and the others from memory."""
    rng = np.random.default_rng(11)
    b = scenes.cornell()
    grey = b.MatteMaterial((0.5, 0.5, 0.5), 60.0)
    c = rng.uniform(-1.0, 1.0, (40, 1, 3))
    big = (c + rng.uniform(-1.4, 1.4, (40, 3, 3))).astype(np.float32)
    b.add_mesh(big.reshape(-1, 3), np.arange(120, dtype=np.int32).reshape(-1, 3), grey)
    c = rng.uniform(-2.0, 2.0, (300, 1, 3))
    small = (c + rng.uniform(-0.05, 0.05, (300, 3, 3))).astype(np.float32)
    b.add_mesh(small.reshape(-1, 3), np.arange(900, dtype=np.int32).reshape(-1, 3), grey)
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    tc = tri_corners(b)
    check_queries(scene, aimed_rays(gpu, tc[:52], N_RAYS // 52, seed=12), osc)
    check_queries(scene, aimed_rays(gpu, tc[52:], N_RAYS // 300, seed=13), osc)
    check_queries(scene, scenes.random_rays(N_RAYS, seed=14), osc)
    check_queries(scene, through_rays(gpu, tc[12:52], tc[:52], N_RAYS, seed=15), osc)
    check_queries(scene, axis_rays(gpu, tc[:12], N_RAYS, seed=16), osc)
    check_render(gpu, scene, osc)
    hot, loaded = hot_share(gpu, scene)
    assert 0 < hot < loaded, (hot, loaded)


def coincident_quad(z=0.3, s=0.9):
    """four triangles over one axis-aligned quad (both diagonals): their bounds, hence their centroids, coincide, so no split separates them"""
    v = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3]], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["leaf_of_four", "one_leaf", "spheres", "zero_components"])
def test_shapes_of_leaves(gpu, case):
    """leaf_of_four: a four-triangle leaf next to the root of a tree of far fewer than 64 DNode4 (a staged hot leaf advances through its slots,
    its box tested once).  one_leaf: the whole scene is one leaf (root4 < 0: no node, no table).  spheres: the SPH instantiation (a sphere hit
    in hand when a wall is popped).  zero_components: rays with zero direction components against the hot walls."""
    if case == "one_leaf":
        b = gpu.SceneBuilder()
        v, t = coincident_quad()
        b.add_mesh(v, t, b.MatteMaterial(scenes.WHITE, 60.0))
    elif case == "spheres":
        b = scenes.cornell_sphere("matte")
    else:
        b = scenes.cornell()
        if case == "leaf_of_four":
            v, t = coincident_quad()
            b.add_mesh(v, t, b.MatteMaterial(scenes.DRAGON_GREEN, 60.0))
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    first, count = leaf_table(scene)
    if case == "leaf_of_four":
        assert count.max() >= 4 and len(scene.bvh()[1]) < 64
    if case == "one_leaf":
        assert len(count) == 1 and count[0] == 4
    tc = tri_corners(b)
    check_queries(scene, aimed_rays(gpu, tc, N_RAYS // len(tc), seed=21), osc)
    check_queries(scene, aimed_rays(gpu, tc, N_RAYS // len(tc), seed=22, origin_box=4.0, tmax=5.0), osc)
    check_queries(scene, scenes.random_rays(N_RAYS, seed=23), osc)
    # (one_leaf: no origins in the plane of the quad's box.  A tree that is one leaf has no hot table and no cached node; there the 4-wide walk
    # enters the root leaf without the test of the root's box that the binary walk makes first, and the two differ for a ray whose origin lies
    # in a face of that box with a zero direction component across it (0 * inf in the box test): not a matter of where a leaf is read from.)
    check_queries(scene, axis_rays(gpu, tc, N_RAYS, seed=24, in_plane=case != "one_leaf"), osc)
    if case != "one_leaf":   # (a scene without lights renders black)
        check_render(gpu, scene, osc)
        hot, loaded = hot_share(gpu, scene)
        assert 0 < hot <= loaded


@pytest.mark.gpu
def test_edits_reach_the_hot_copy(gpu):
    """The hot copy is made from the live tables at every launch: after a wall has moved (gnxr_scene_update_vertices: refit) and after the mesh
    has been replaced (gnxr_scene_set_geometry: a new tree), queries and frames equal those of a freshly built scene."""
    b = cornell_with_mesh()
    scene = gpu.Scene(b)
    integ = gpu.PathIntegrator(DEPTH, 1.0, "spatial")
    integ.Render(scene, W, H, SPP)   # the scene has been traced before the edit
    v = tsu.vertices(b)
    idx = tsu.indices(b)
    movable = np.setdiff1d(np.unique(idx[:12]), tsu.emissive_vertices(b))
    far_x = movable[v[movable, 0] == v[movable, 0].max()]   # the wall at the largest x, pushed outwards
    assert len(far_x) >= 4
    v2 = v.copy()
    v2[far_x, 0] += np.float32(0.375)
    scene.update_vertices(v2)
    moved = tsu.Deformed(b, v2)   # (keeps v2 alive while the scene is created from it)
    fresh = gpu.Scene(moved.desc())
    tc = v2[idx]
    for rays in (aimed_rays(gpu, tc[:12], N_RAYS // 12, seed=31, origin_box=2.0), scenes.random_rays(N_RAYS, seed=32),
                 through_rays(gpu, tc[12:], tc[:12], N_RAYS, seed=33)):
        h, o = check_queries(scene, rays, tsu.oracle_on(b, v2, scene))
        hf, of = trq.dquery(fresh, rays)
        assert trq.same_records(h, hf) and (o == of).all()
    tsu.same_render(gpu, integ, scene, fresh, W, H, SPP)

    # another mesh: the box and every third model triangle left out, in another order
    g = tsg.start_geometry(b)
    scene.set_geometry(**g)
    fresh = gpu.Scene(tsg.ReGeom(b, g, "hlbvh").desc())
    tc = g["vertices"][g["indices"]]
    for rays in (aimed_rays(gpu, tc[:12], N_RAYS // 12, seed=34, origin_box=2.0), scenes.random_rays(N_RAYS, seed=35),
                 through_rays(gpu, tc[12:], tc[:12], N_RAYS, seed=36)):
        h, o = check_queries(scene, rays)
        hf, of = trq.dquery(fresh, rays)
        assert trq.same_records(h, hf) and (o == of).all()
    tsu.same_render(gpu, integ, scene, fresh, W, H, SPP)


# ---------------------------------------------------------------- budget
def test_register_budget_of_the_timed_kernels():
    """(No GPU: read from the built library.)  The two timed instantiations k_trace4<false, false, SPILL, 0> keep the parent's 96 VGPRs and
    five waves per SIMD (profiles/kernel_regs_hot_leaves_parent.txt), with no scratch and no spilled VGPRs."""
    import os
    import sys
    sys.path.insert(0, os.path.join(scenes.ROOT, "tools"))
    import kernel_regs
    timed = [k for k in kernel_regs.kernels() if any(f"k_trace4<false, false, {spill}, 0>" in k["name"] for spill in ("true", "false"))]
    assert len(timed) == 2, [k["name"] for k in timed]
    for k in timed:
        assert k["vgpr"] <= 96 and k["waves_per_simd"] == 5 and k["vgpr_spill"] == 0 and k["scratch"] == 0, k


@pytest.mark.gpu
def test_lds_budget_of_the_benchmark_scene(gpu):
    """trace_launch's own figures for the cfg 3 scene (gnxr_scene_trace_plan): the hot region is there, five blocks with the 1 KB each that the
    plan keeps back fit a CU's 160 KB, and the stack keeps the LDS levels the parent had -- 11, which is also what the same budget gives
    without the hot region's bytes."""
    scene = gpu.Scene(scenes.dragon_cornell(100000, "glass+metal"))
    p = scene.trace_plan(1920 * 1080 * 32)
    print(p)
    assert p["wide"] == 1 and p["n_top"] == 64 and p["hot_bytes"] == HOT_BYTES and p["blocks_per_cu"] == 5
    assert p["stack_entries"] >= 11 and p["lds_entries"] == 11
    assert 5 * (p["lds_bytes"] + 1024) <= 160 * 1024
    beside_the_stack = p["lds_bytes"] - p["lds_entries"] * 256 * 4
    assert ((160 * 1024) // 5 - 1024 - (beside_the_stack - p["hot_bytes"])) // (256 * 4) == p["lds_entries"]   # the parent's levels
    # a scene without a 4-wide node has nothing to cache and no hot table
    b = gpu.SceneBuilder()
    v, t = coincident_quad()
    b.add_mesh(v, t, b.MatteMaterial(scenes.WHITE, 60.0))
    q = gpu.Scene(b).trace_plan(4096)
    assert q["n_top"] == 0 and q["hot_bytes"] == 0
