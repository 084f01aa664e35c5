"""Lightmap baking (include/gnxr.h, "Lightmap baking"): the numpy restatement (tests/bake_reference.py) on hand-made cases, then on the GPU
bake_texels and surface_rays against it, BakeLightmap against the composition bake_texels + surface_rays + Li + the ordered sum + the
restated dilation, closed forms, live edits, the refusals and the streams.  Every comparison is on bits."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import bake_reference as br
import scenes
from conftest import GOLDEN, ROOT

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
f32 = np.float32
TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")
QUAD = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], f32)


# ---------------------------------------------------------------- CPU: the restatement on hand-made cases
def test_restated_quad_atlas_covers_every_texel_once_and_the_diagonal_goes_to_triangle_0():
    tri, bary = br.rasterise(QUAD, 8, 8)
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    assert (tri == np.where(x >= y, 0, 1)).all()
    assert (tri[np.arange(8), np.arange(8)] == 0).all()
    # on the diagonal of triangle 0 = (0,0), (1,0), (1,1): wb = E(p2, p0, P) = 0, so b1 = 0 and b2 = the centre's u
    cu = (np.arange(8, dtype=f32) + f32(0.5)) / f32(8)
    assert br.biteq(np.abs(bary[np.arange(8), np.arange(8), 0]), np.zeros(8, f32)) and br.biteq(bary[np.arange(8), np.arange(8), 1], cu)
    # the barycentrics give the centre back: u = b1 * 1 + b2 * 1, v = b2 * 1 for triangle 0
    lower = tri == 0
    assert np.allclose((bary[..., 0] + bary[..., 1])[lower], ((x + 0.5) / 8)[lower], atol=1e-6) and np.allclose(bary[..., 1][lower], ((y + 0.5) / 8)[lower], atol=1e-6)


def test_restated_reversed_winding_bakes_the_same_texels():
    tri, bary = br.rasterise(QUAD, 8, 8)
    rev = QUAD.reshape(2, 3, 2)[:, ::-1].reshape(2, 6)   # corners (p2, p1, p0): negative area
    tri_r, bary_r = br.rasterise(rev, 8, 8)
    assert (tri_r == tri).all()
    # (b1, b2) are the weights of the SECOND and THIRD corner as listed: reversed, b1 stays p1's and b2 becomes p0's
    b0 = 1 - bary[..., 0] - bary[..., 1]
    assert np.allclose(bary_r[..., 0], bary[..., 0], atol=1e-6) and np.allclose(bary_r[..., 1], b0, atol=1e-6)


def test_restated_degenerate_and_tiny_triangles_cover_nothing():
    zero_area = np.array([[0.1, 0.1, 0.5, 0.5, 0.9, 0.9], [0.3, 0.3, 0.3, 0.3, 0.3, 0.3]], f32)
    assert (br.rasterise(zero_area, 8, 8)[0] == -1).all()
    bad = np.array([[0, 0, np.nan, 0, 1, 1], [0, 0, np.inf, 0, 1, 1]], f32)
    assert (br.rasterise(bad, 8, 8)[0] == -1).all()
    # between the centres 0.0625 and 0.1875 of an 8-texel row: smaller than a texel, over no centre
    tiny = np.array([[0.07, 0.07, 0.18, 0.07, 0.18, 0.18]], f32)
    assert (br.rasterise(tiny, 8, 8)[0] == -1).all()
    # the same triangle moved over a centre covers exactly that texel
    over = tiny + f32(0.03)
    t = br.rasterise(over, 8, 8)[0]
    assert (t >= 0).sum() == 1 and t[1, 1] == 0
    # a chart outside [0, 1]^2 is clipped by the atlas, not wrapped
    outside = np.array([[0.5, 0.5, 1.5, 0.5, 1.5, 1.5], [2, 2, 3, 2, 3, 3]], f32)
    t = br.rasterise(outside, 8, 8)[0]
    assert (t[:, :4] == -1).all() and (t[:4] == -1).all() and (t == 1).sum() == 0 and (t == 0).sum() > 0


def test_restated_dilation_of_a_5x5_pattern_worked_out_by_hand():
    a, b = np.array([1, 0, 0], f32), np.array([0, 2, 0], f32)
    img = np.zeros((5, 5, 4), f32)
    img[1, 1] = (*a, 1)
    img[3, 3] = (*b, 1)
    m = (a + b) / f32(2)                       # texel (2, 2): (1, 1) comes first in (dy, dx) order, then (3, 3)
    one = br.dilate(img, 1)
    want = np.zeros((5, 5, 3), f32)
    want[0:3, 0:3] = a
    want[2:5, 2:5] = b
    want[2, 2] = m
    assert br.biteq(one[..., :3], want)
    assert br.biteq(one[..., 3], img[..., 3])   # alpha is never changed
    two = br.dilate(img, 2)
    mix = ((((a + a) + m) + b) + b) / f32(5)    # (x, y) = (3, 1): (2,0) a, (2,1) a, (2,2) m, (3,2) b, (4,2) b
    want2 = want.copy()
    want2[0, 3] = a                             # [y, x]: neighbours (2,0), (2,1)
    want2[1, 3] = mix
    want2[1, 4] = b                             # neighbours (3,2), (4,2)
    want2[3, 0] = a
    want2[3, 1] = mix                           # (0,2) a, (1,2) a, (2,2) m, (2,3) b, (2,4) b
    want2[4, 1] = b
    assert br.biteq(two[..., :3], want2)        # the corners (4, 0) and (0, 4) have no filled neighbour yet
    assert br.biteq(two[..., 3], img[..., 3])
    assert br.biteq(br.dilate(img, 0), img)


def test_bake_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    for name in ("gnxr_bake_texels_device", "gnxr_surface_rays_device", "gnxr_bake_dilate_device", "gnxr_bake_lightmap_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(gx.lib(), name) and name in gx._abi.PROTOTYPES, name
    # gnxr_bake_params carries struct_size, like every record since gnxr_geometry: the list of gnxr_abi_sizeof is the parent's
    assert re.search(r"struct gnxr_bake_params \{ int32_t struct_size; uint32_t flags; int32_t dilate, medium; \}", hdr)
    assert C.sizeof(gx._abi.BakeParams) == 16 and [f[0] for f in gx._abi.BakeParams._fields_] == ["struct_size", "flags", "dilate", "medium"]
    assert gx.lib().gnxr_abi_version() == 5 and gx.lib().gnxr_abi_sizeof(13) > 0 and gx.lib().gnxr_abi_sizeof(14) == -1
    assert gx._abi.BAKE_FLIP_NORMALS == 1 and re.search(r"#define GNXR_BAKE_FLIP_NORMALS 1u", hdr)
    for cls in (gx.PathIntegrator, gx.VolPathIntegrator, gx.WhittedIntegrator, gx.DirectLightingIntegrator):
        assert cls.BakeLightmap is gx.PathIntegrator.BakeLightmap
    for name in ("bake_texels", "surface_rays", "bake_dilate"):
        assert callable(getattr(gx, name))


def test_bake_calls_refuse_malformed_arguments_before_any_device(gx):
    lib = gx.lib()
    assert lib.gnxr_bake_texels_device(None, None, 8, 8, None, None, None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(8, 8, 1, None, None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(8, 8, -1, C.c_void_p(16), None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(0, 8, 1, C.c_void_p(16), None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(8, 8, 1, C.c_void_p(20), None) == ERR_INVALID and b"aligned" in lib.gnxr_last_error()
    assert lib.gnxr_surface_rays_device(None, 8, 8, None, None, None, None, None, 0, 0, -1, None, None, None, None) == ERR_INVALID
    assert lib.gnxr_bake_lightmap_device(None, None, None, None, None, None, None) == ERR_INVALID


# ---------------------------------------------------------------- GPU helpers
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def mesh_arrays(b):
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).copy()
    i = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).copy()
    return v, i


def soup_builder(n_tris, seed=7):
    """a scene of n_tris unrelated triangles: bake_texels reads only how many there are"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (3 * n_tris, 3)).astype(f32)
    b = gx_mod().SceneBuilder()
    b.add_mesh(v, np.arange(3 * n_tris, dtype=np.int32).reshape(-1, 3), b.MatteMaterial((0.5, 0.5, 0.5), 0.0))
    return b


def gx_mod():
    import gnxraytracer_amd
    return gnxraytracer_amd


def cells_for(n_tris):
    return max(1, math.ceil(math.sqrt((n_tris + 1) // 2)))


def make_atlas(cells):
    """cells^2 square charts of two triangles -- with cells = 8 the corners and the texel centres of a 64 x 64 atlas are exact, so centres lie
    exactly on diagonals and shared edges -- then zero-area triangles, sub-texel triangles, a chart that leaves [0, 1]^2, non-finite uvs
    and the first chart listed again (the lowest index must win)."""
    uv = br.grid_atlas(2 * cells * cells, cells)
    uv[5] = uv[5].reshape(3, 2)[::-1].reshape(6)     # one reversed winding
    extra = np.array([[0.2, 0.2, 0.4, 0.4, 0.8, 0.8], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5],            # zero area
                      [0.5001, 0.5001, 0.5003, 0.5001, 0.5003, 0.5003], [0.26, 0.26, 0.27, 0.26, 0.27, 0.27],   # sub-texel
                      [0.9, 0.9, 1.7, 0.9, 1.7, 1.7], [0.9, 0.9, 1.7, 1.7, 0.9, 1.7],            # a chart reaching outside
                      [-3, -3, -2, -3, -2, -2], [0, 0, np.nan, 0, 1, 1], [0, 0, 1, 0, np.inf, 1],
                      uv[0], uv[1]], f32)
    return np.concatenate([uv, extra])


def covered_records(tri, bary, spp):
    """the (texel, sample) records of a bake in sample-major order: tensors tri, bary, px, py, s and the number of covered texels"""
    H, W = tri.shape
    texel = torch.nonzero(tri.reshape(-1) >= 0).reshape(-1)
    n = texel.shape[0]
    t = tri.reshape(-1)[texel].repeat(spp).contiguous()
    bb = bary.reshape(-1, 2)[texel].repeat(spp, 1).contiguous()
    px = (texel % W).to(torch.int32).repeat(spp).contiguous()
    py = (texel // W).to(torch.int32).repeat(spp).contiguous()
    s = torch.arange(spp, device=tri.device, dtype=torch.int32).repeat_interleave(n).contiguous()
    return t, bb, px, py, s, n


def compose(gx, integ, scene, lm_uv, W, H, spp, dilate, flip=False, medium=-1):
    """the bake, spelled out: (image, L [spp, n_covered, 4], tri, rays [spp * n_covered, 8] on the device)"""
    tri, bary = gx.bake_texels(scene, lm_uv, W, H)
    t, bb, px, py, s, n = covered_records(tri, bary, spp)
    rays, samples, _ = gx.surface_rays(scene, t, bb, px, py, s, W, H, flip=flip, medium=medium)
    L, _ = integ.Li(scene, rays, samples, W, H, spp)
    L = L.cpu().numpy().reshape(spp, n, 4)
    tri = tri.cpu().numpy()
    return br.dilate(br.reduce_lightmap(tri, L, spp), dilate), L, tri, rays


def assert_escaped_into_the_constant_sky(scene, rays, L):
    """Every L is, bit for bit, Le of the environment (the scene's only light) along its ray -- the ray escaped at once, so it left on the
    side it should and did not hit the surface it started on -- and that Le is the map's constant 1 up to the roundings of the map's
    bilinear lookup (four weighted texels of 1: at most four roundings of 2^-24 below 1, never above)."""
    le = scene.light_le(0, rays).cpu().numpy()
    assert br.biteq(L[..., :3].reshape(-1, 3), le)
    assert (le <= 1).all() and (le >= f32(1 - 2.0 ** -22)).all() and (le == 1).mean() > 0.5


def sincos(gx):
    return lambda theta: (gx.eval_libm("sincos.sin", theta), gx.eval_libm("sincos.cos", theta))


def quad_builder(blocker=False):
    """a 2 x 2 floor quad at y = 0 wound so that Normalize(Cross(p0 - p2, p1 - p2)) = +y, under a constant environment of radiance 1;
    blocker: a 12 x 12 quad at y = 0.25 above it"""
    gx = gx_mod()
    b = gx.SceneBuilder()
    white = b.MatteMaterial(scenes.WHITE, 0.0)
    v = np.array([[-1, 0, 1], [1, 0, -1], [-1, 0, -1], [1, 0, -1], [-1, 0, 1], [1, 0, 1]], f32)
    b.add_mesh(v, np.arange(6, dtype=np.int32).reshape(2, 3), white)
    if blocker:
        b.add_mesh(v * f32(6) + np.array([0, 0.25, 0], f32), np.arange(6, dtype=np.int32).reshape(2, 3), white)
    b.AddInfLightData(np.ones((8, 16, 3), f32))
    return b


# ---------------------------------------------------------------- GPU 1: texels
@pytest.mark.gpu
@pytest.mark.parametrize("cells,W,H", [(8, 64, 64), (8, 50, 37), (10, 64, 64), (10, 50, 37)])
def test_bake_texels_equal_the_brute_force_restatement(gpu, cells, W, H):
    uv = make_atlas(cells)
    scene = gpu.Scene(soup_builder(len(uv)))
    tri, bary = gpu.bake_texels(scene, dev(uv), W, H)
    want_tri, want_bary = br.rasterise(uv, W, H)
    tri, bary = tri.cpu().numpy(), bary.cpu().numpy()
    assert tri.shape == (H, W) and tri.dtype == np.int32 and bary.shape == (H, W, 2)
    assert (tri == want_tri).all(), np.argwhere(tri != want_tri)[:4]
    assert br.biteq(bary, want_bary)
    n = 2 * cells * cells
    assert (tri != n + 9).all() and (tri != n + 10).all()    # chart 0 listed again never wins
    if (cells, W, H) == (8, 64, 64):                         # corners and centres are exact: the charts tile the atlas ...
        assert (tri >= 0).all() and (tri < n).all()
        d = np.arange(64)                                    # ... and centres exactly on a diagonal go to the lower triangle of the chart
        assert (tri[d, d] % 2 == 0).all() and (tri[d, d] // 2 == (d // 8) * 9).all()


@pytest.mark.gpu
def test_bake_texels_of_a_single_triangle_and_without_barycentrics(gpu):
    uv = np.array([[0.1, 0.15, 0.85, 0.2, 0.4, 0.9]], f32)
    scene = gpu.Scene(soup_builder(1))
    tri, bary = gpu.bake_texels(scene, dev(uv), 19, 23)
    want_tri, want_bary = br.rasterise(uv, 19, 23)
    assert (tri.cpu().numpy() == want_tri).all() and br.biteq(bary.cpu().numpy(), want_bary) and (want_tri == 0).sum() > 20
    only = torch.full((23, 19), 5, dtype=torch.int32, device=DEV)
    gx = gpu
    gx._check(gx.lib().gnxr_bake_texels_device(scene._h, C.c_void_p(dev(uv).data_ptr()), 19, 23, C.c_void_p(only.data_ptr()), None, None))
    assert (only.cpu().numpy() == want_tri).all()


# ---------------------------------------------------------------- GPU 2: surface rays
def surface_ray_case(gx, seed=3, n=1000, W=37, H=29, spp=16):
    b = scenes.cornell()
    b.add_mesh(np.array([[0.3, -1, 0.2], [0.3, -1, 0.2], [1.0, -1, 0.5]], f32), np.array([[0, 1, 2]], np.int32), b.MatteMaterial((0.5, 0.5, 0.5), 0.0))
    v, idx = mesh_arrays(b)
    nt = len(idx)
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, nt - 1, n).astype(np.int32)
    tri[::50] = nt - 1                                       # the degenerate triangle
    b1 = rng.uniform(0, 1, n).astype(f32)
    b2 = (rng.uniform(0, 1, n).astype(f32) * (f32(1) - b1)).astype(f32)
    bary = np.stack([b1, b2], axis=1)
    bary[1:30:3] = (0, 0)
    bary[2:30:3] = (1, 0)
    bary[3:30:3] = (0, 1)
    px, py = rng.integers(0, W, n).astype(np.int32), rng.integers(0, H, n).astype(np.int32)
    s = rng.integers(0, spp, n).astype(np.int32)
    return b, v, idx, tri, bary, px, py, s, W, H


def restated_surface_records(gx, v, idx, tri, bary, px, py, s, W, H, flip, medium):
    u = np.stack([gx.sample_halton(W, H, px, py, s, np.full(len(px), 3, np.int32)), gx.sample_halton(W, H, px, py, s, np.full(len(px), 4, np.int32))], axis=1)
    p0, p1, p2 = v[idx[tri, 0]], v[idx[tri, 1]], v[idx[tri, 2]]
    o, d, p, nrm, valid = br.surface_rays(p0, p1, p2, bary, u, sincos(gx), flip)
    n = len(tri)
    rays, pn, samples = np.zeros((n, 8), f32), np.zeros((n, 8), f32), np.zeros((n, 4), np.int32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = o, np.where(valid, f32(np.inf), f32(0)), d
    pn[:, 0:3], pn[:, 4:7] = p, nrm
    samples[valid] = np.stack([px, py, s, np.full(n, medium, np.int32)], axis=1)[valid]
    return rays, samples, pn, valid


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_surface_rays_equal_the_restatement(gpu, flip):
    gx = gpu
    b, v, idx, tri, bary, px, py, s, W, H = surface_ray_case(gx)
    scene = gx.Scene(b)
    rays, samples, pn = gx.surface_rays(scene, dev(tri), dev(bary), dev(px), dev(py), dev(s), W, H, flip=flip)
    want_rays, want_samples, want_pn, valid = restated_surface_records(gx, v, idx, tri, bary, px, py, s, W, H, flip, -1)
    rays, samples, pn = rays.cpu().numpy(), samples.cpu().numpy(), pn.cpu().numpy()
    assert (~valid).sum() == 20 and (valid == (tri != len(idx) - 1)).all()
    assert br.biteq(pn, want_pn), np.argwhere(pn.view(np.uint32) != want_pn.view(np.uint32))[:4]
    assert br.biteq(rays, want_rays), np.argwhere(rays.view(np.uint32) != want_rays.view(np.uint32))[:4]
    assert (samples == want_samples).all()
    # the rays leave on the normal's side, from an origin on that side of the surface point
    d, nrm = rays[valid, 4:7].astype(np.float64), pn[valid, 4:7].astype(np.float64)
    assert ((d * nrm).sum(1) >= -1e-6).all() and (((rays[valid, 0:3].astype(np.float64) - pn[valid, 0:3]) * nrm).sum(1) > 0).all()
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-5)


@pytest.mark.gpu
def test_surface_rays_zero_a_record_out_of_range_finish_the_others_and_raise(gpu):
    gx = gpu
    b, v, idx, tri, bary, px, py, s, W, H = surface_ray_case(gx, n=200)
    scene = gx.Scene(b)
    good = [t.cpu().numpy() for t in gx.surface_rays(scene, dev(tri), dev(bary), dev(px), dev(py), dev(s), W, H)]
    for what, k in (("tri", 17), ("tri_neg", 31), ("px", 64), ("py", 5), ("s", 130)):
        t2, px2, py2, s2 = tri.copy(), px.copy(), py.copy(), s.copy()
        if what == "tri":
            t2[k] = len(idx)
        elif what == "tri_neg":
            t2[k] = -1
        elif what == "px":
            px2[k] = W
        elif what == "py":
            py2[k] = -1
        else:
            s2[k] = -1
        out = (torch.full((200, 8), 7.0, device=DEV), torch.full((200, 4), 7, dtype=torch.int32, device=DEV), torch.full((200, 8), 7.0, device=DEV))
        with pytest.raises(gx.GnxrError, match=r"record %d\b" % k):
            gx.surface_rays(scene, dev(t2), dev(bary), dev(px2), dev(py2), dev(s2), W, H, out=out)
        for got, want in zip(out, good):
            got = got.cpu().numpy()
            keep = np.arange(200) != k
            assert (got[k] == 0).all() and (got[keep].view(np.uint32) == want[keep].view(np.uint32)).all(), what


# ---------------------------------------------------------------- GPU 3: the bake is the composition
def integrator_and_scene(gx, name):
    if name == "path":
        return gx.PathIntegrator(5, 1.0, "spatial"), scenes.cornell()
    if name == "whitted":
        return gx.WhittedIntegrator(5), scenes.cornell()
    return gx.VolPathIntegrator(5, 1.0, "spatial"), scenes.volume_cornell()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["path", "whitted", "volpath"])
def test_bake_equals_the_composition(gpu, name):
    gx = gpu
    integ, b = integrator_and_scene(gx, name)
    scene = gx.Scene(b)
    W = H = 32
    spp = 4
    uv = dev(br.grid_atlas(scene.n_triangles, cells_for(scene.n_triangles)))
    want0, L, tri, _ = compose(gx, integ, scene, uv, W, H, spp, 0)
    n_cov = int((tri >= 0).sum())
    assert 0 < n_cov < W * H and np.isfinite(L).all() and (L[..., :3] > 0).any()
    img0, st = integ.BakeLightmap(scene, uv, W, H, spp, dilate=0)
    assert img0.shape == (H, W, 4) and br.biteq(img0.cpu().numpy(), want0), np.argwhere(img0.cpu().numpy().view(np.uint32) != want0.view(np.uint32))[:4]
    assert st["camera_samples"] == n_cov * spp and st["rays_closest"] >= n_cov * spp
    img2, _ = integ.BakeLightmap(scene, uv, W, H, spp, dilate=2)
    want2 = br.dilate(want0, 2)
    assert br.biteq(img2.cpu().numpy(), want2)
    assert not br.biteq(want2, want0) and br.biteq(want2[..., 3], want0[..., 3])   # the gutters were filled; alpha still tells baked from dilated
    if name == "path":
        # sub-batches: the covered texels are no multiple of the batch, every layer of samples takes several, the last one partial
        spp_pass = 100
        assert n_cov % spp_pass != 0 and n_cov > 2 * spp_pass
        small, st_small = integ.BakeLightmap(scene, uv, W, H, spp, dilate=2, samples_per_pass=spp_pass)
        again, _ = integ.BakeLightmap(scene, uv, W, H, spp, dilate=2)
        assert br.biteq(small.cpu().numpy(), want2) and br.biteq(again.cpu().numpy(), want2)
        assert st_small["camera_samples"] == n_cov * spp
        # a layer fits a batch, two do not: whole layers per batch
        mid, _ = integ.BakeLightmap(scene, uv, W, H, spp, dilate=2, samples_per_pass=n_cov + 1)
        assert br.biteq(mid.cpu().numpy(), want2)


# ---------------------------------------------------------------- GPU 4: closed forms
@pytest.mark.gpu
def test_bake_without_lights_is_black_and_alpha_is_the_coverage(gpu):
    gx = gpu
    scene = gx.Scene(scenes.cornell_no_lights())
    uv = dev(br.grid_atlas(scene.n_triangles, cells_for(scene.n_triangles)))
    img, _ = gx.PathIntegrator(5, 1.0, "spatial").BakeLightmap(scene, uv, 32, 32, 4, dilate=0)
    tri, _ = gx.bake_texels(scene, uv, 32, 32)
    img = img.cpu().numpy()
    assert (img[..., :3] == 0).all() and (img[..., 3] == (tri.cpu().numpy() >= 0)).all() and 0 < img[..., 3].sum() < 32 * 32


@pytest.mark.gpu
def test_bake_of_a_quad_under_a_constant_sky_is_pi(gpu):
    """An upward-wound quad under an environment map of ones: every ray must escape upwards at once.  The map's bilinear lookup returns
    1 or a float just below it (0.9999999 = 1 - 2^-23: measured for a fraction of the directions), so Li is checked against the light's
    own Le along each ray, bit for bit; a texel whose four samples are exactly 1 is then exactly fl(4 / 4 * pi), the others lie within
    those roundings below it."""
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(quad_builder())
    uv = dev(QUAD * f32(0.75) + f32(0.125))
    want, L, tri, rays = compose(gx, integ, scene, uv, 32, 32, 4, 0)
    assert_escaped_into_the_constant_sky(scene, rays, L)
    assert (rays[:, 5] > 0).all()                                          # upwards: the quad's normal is +y
    img, _ = integ.BakeLightmap(scene, uv, 32, 32, 4, dilate=0)
    img = img.cpu().numpy()
    covered = tri >= 0
    assert covered.sum() == 24 * 24 and br.biteq(img, want) and (img[~covered] == 0).all()
    exact = (L[..., :3] == 1).all(axis=(0, 2))                             # per covered texel, in texel order
    pi_exact = (f32(4) / f32(4)) * br.PI
    assert exact.mean() > 0.25 and br.biteq(img[covered][exact][:, :3], np.full((exact.sum(), 3), pi_exact, f32))
    assert (img[covered][:, :3] <= pi_exact).all() and (img[covered][:, :3] >= pi_exact * f32(1 - 2.0 ** -21)).all() and (img[covered][:, 3] == 1).all()


@pytest.mark.gpu
def test_bake_flip_leaves_from_the_other_side(gpu):
    """The quad under a large blocker, in the constant environment: unflipped, every ray ends on the blocker's underside (a matte surface
    returns no sample of exactly the sky's radiance four times over); flipped, every ray leaves downwards and escapes.  (A sky that is
    black below the quad would make both bakes 0 under a blocker this size -- no light reaches the gap -- so the environment stays
    constant and the flipped side is the closed form.)"""
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(quad_builder(blocker=True))
    uv = np.zeros((4, 6), f32)
    uv[:2] = QUAD * f32(0.75) + f32(0.125)
    uv = dev(uv)
    want_down, L_down, tri, rays_down = compose(gx, integ, scene, uv, 32, 32, 4, 0, flip=True)
    assert_escaped_into_the_constant_sky(scene, rays_down, L_down)
    assert (rays_down[:, 5] < 0).all()
    up, _ = integ.BakeLightmap(scene, uv, 32, 32, 4, dilate=0)
    down, _ = integ.BakeLightmap(scene, uv, 32, 32, 4, dilate=0, flip=True)
    up, down = up.cpu().numpy(), down.cpu().numpy()
    covered = tri >= 0
    assert covered.sum() == 24 * 24 and br.biteq(down, want_down) and (down[..., 3] == up[..., 3]).all() and (up[..., 3] == covered).all()
    assert (up[covered][:, :3] != down[covered][:, :3]).all(axis=1).all() and np.isfinite(up).all()


# ---------------------------------------------------------------- GPU 5: live edits
@pytest.mark.gpu
def test_bake_after_update_vertices_sees_the_edit(gpu):
    """cornell() is five walls and the light: the edit lifts the floor (its first six vertices) by 1.5."""
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    b = scenes.cornell()
    scene = gx.Scene(b)
    uv = dev(br.grid_atlas(scene.n_triangles, cells_for(scene.n_triangles)))
    before, _ = integ.BakeLightmap(scene, uv, 32, 32, 4, dilate=1)
    before = before.cpu().numpy()
    v, idx = mesh_arrays(b)
    v2 = v.copy()
    v2[:6, 1] += f32(1.5)
    scene.update_vertices(v2[:6])
    want, _, tri, _ = compose(gx, integ, scene, uv, 32, 32, 4, 1)
    after, _ = integ.BakeLightmap(scene, uv, 32, 32, 4, dilate=1)
    after = after.cpu().numpy()
    assert br.biteq(after, want) and not br.biteq(after, before)
    floor = (tri == 0) | (tri == 1)
    assert (after[floor][:, :3] != before[floor][:, :3]).any(axis=1).mean() > 0.9
    # the surface points are those of the moved vertices
    n = 64
    t = np.arange(n, dtype=np.int32) % 2
    bary = np.full((n, 2), 0.25, f32)
    px = py = s = np.zeros(n, np.int32)
    _, _, pn = gx.surface_rays(scene, dev(t), dev(bary), dev(px), dev(py), dev(s), 32, 32)
    _, _, want_pn, _ = restated_surface_records(gx, v2, idx, t, bary, px, py, s, 32, 32, False, -1)
    assert br.biteq(pn.cpu().numpy(), want_pn)


# ---------------------------------------------------------------- GPU 6: errors
@pytest.mark.gpu
def test_bake_refusals_leave_the_output_untouched(gpu):
    gx = gpu
    lib = gx.lib()
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(scenes.cornell())
    uv = dev(br.grid_atlas(scene.n_triangles, 4))
    W = H = 16
    out = torch.full((H * W * 4 + 4,), 7.0, device=DEV)
    p = integ.params(W, H, 2)
    bp = lambda size=16, flags=0, dilate=1, medium=-1: gx._abi.BakeParams(size, flags, dilate, medium)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def bake(params=p, bake_params=None, uv_ptr=None, out_ptr=None, s=scene):
        return lib.gnxr_bake_lightmap_device(s._h, C.byref(params), C.byref(bake_params or bp()), uv_ptr or ptr(uv), out_ptr or ptr(out), None, None)

    host_img, host_uv = torch.zeros(H * W * 4), torch.zeros((scene.n_triangles, 6))
    assert bake(out_ptr=ptr(host_img)) == ERR_INVALID and b"device memory" in lib.gnxr_last_error()
    assert bake(uv_ptr=ptr(host_uv)) == ERR_INVALID
    assert bake(out_ptr=ptr(out, 4)) == ERR_INVALID and b"aligned" in lib.gnxr_last_error()
    assert bake(params=integ.params(0, H, 2)) == ERR_INVALID
    assert bake(params=integ.params(W, H, 0)) == ERR_INVALID
    assert bake(params=integ.params(W, H, 2, spp_begin=1, spp_end=2)) == ERR_INVALID
    assert bake(params=integ.params(W, H, 2, shard_index=1, shard_count=2)) == ERR_INVALID
    assert bake(bake_params=bp(dilate=-1)) == ERR_INVALID and b"dilate" in lib.gnxr_last_error()
    assert bake(bake_params=bp(size=12)) == ERR_INVALID and b"struct_size" in lib.gnxr_last_error()
    assert bake(bake_params=bp(flags=2)) == ERR_INVALID
    assert bake(bake_params=bp(medium=0)) == ERR_INVALID
    textured = gx.Scene(scenes.textured_cornell(TEX))
    uv_t = dev(br.grid_atlas(textured.n_triangles, cells_for(textured.n_triangles)))
    for cls in (gx.WhittedIntegrator(5), gx.DirectLightingIntegrator("all", 5), gx.VolPathIntegrator(5, 1.0, "spatial")):
        assert bake(params=cls.params(W, H, 2), uv_ptr=ptr(uv_t), s=textured) == ERR_UNSUPPORTED
    assert (out == 7).all()
    # the same through the bindings; PathIntegrator bakes the textured scene
    with pytest.raises(gx.GnxrError):
        gx.WhittedIntegrator(5).BakeLightmap(textured, uv_t, W, H, 2)
    img, _ = integ.BakeLightmap(textured, uv_t, W, H, 2)
    assert torch.isfinite(img).all() and (img[..., 3] == 1).any()
    for bad in (lambda: integ.BakeLightmap(scene, uv.cpu(), W, H, 2), lambda: integ.BakeLightmap(scene, uv[:-1], W, H, 2), lambda: integ.BakeLightmap(scene, uv, 0, H, 2),
                lambda: integ.BakeLightmap(scene, uv, W, H, 2, dilate=-1), lambda: gx.bake_texels(scene, uv.cpu(), W, H), lambda: gx.bake_dilate(torch.zeros((4, 4, 4)), 1),
                lambda: gx.bake_dilate(torch.zeros((4, 4, 4), device=DEV), -1)):
        with pytest.raises(ValueError):
            bad()
    # the layered calls: host memory and misaligned outputs
    tri_out = torch.full((H * W + 1,), 7, dtype=torch.int32, device=DEV)
    bary_out = torch.full((H * W * 2 + 1,), 7.0, device=DEV)
    assert lib.gnxr_bake_texels_device(scene._h, ptr(uv), W, H, ptr(tri_out), ptr(bary_out, 4), None) == ERR_INVALID
    assert lib.gnxr_bake_texels_device(scene._h, ptr(host_uv), W, H, ptr(tri_out), ptr(bary_out), None) == ERR_INVALID
    assert lib.gnxr_bake_texels_device(scene._h, ptr(uv), 0, H, ptr(tri_out), ptr(bary_out), None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(W, H, 1, ptr(host_img), None) == ERR_INVALID
    assert lib.gnxr_bake_dilate_device(W, H, 1, ptr(out, 4), None) == ERR_INVALID and b"aligned" in lib.gnxr_last_error()
    assert (tri_out == 7).all() and (bary_out == 7).all() and (out == 7).all()


# ---------------------------------------------------------------- GPU 7: streams
@pytest.mark.gpu
def test_bake_texels_and_dilate_on_a_side_stream_behind_the_kernels_that_fill_their_inputs(gpu):
    gx = gpu
    uv_np = make_atlas(8)
    scene = gx.Scene(soup_builder(len(uv_np)))
    W, H = 50, 37
    tri0, bary0 = gx.bake_texels(scene, dev(uv_np), W, H)
    rng = np.random.default_rng(5)
    img_np = rng.uniform(0, 1, (H, W, 4)).astype(f32)
    img_np[..., 3] = rng.uniform(0, 1, (H, W)) < 0.2
    dil0 = gx.bake_dilate(dev(img_np), 3)
    assert br.biteq(dil0.cpu().numpy(), br.dilate(img_np, 3))
    half_uv, half_img = dev(uv_np * f32(0.5)), dev(img_np * f32(0.5))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3                            # keeps the stream busy before the inputs exist
        uv_side = half_uv * 2 + big[0, 0] * 0                 # exact: every value doubles back
        img_side = half_img * 2 + big[0, 0] * 0
        img_side[..., 3] = dev(img_np[..., 3])
        tri1, bary1 = gx.bake_texels(scene, uv_side.contiguous(), W, H, stream=side)
        dil1 = gx.bake_dilate(img_side.contiguous(), 3, stream=side)
    side.synchronize()
    assert torch.isfinite(big[0, 0])
    assert (tri1 == tri0).all() and br.biteq(bary1.cpu().numpy(), bary0.cpu().numpy())
    assert br.biteq(dil1.cpu().numpy(), dil0.cpu().numpy())
