"""First-hit feature buffers: gnxr_render_aov_device / integrator.RenderAOV and gnxr_material_albedo / material_albedo.

Every expected value is composed from entry points that are pinned elsewhere: camera_rays_device gives the camera ray of every sample,
Scene.intersect the hit, and the per-sample values are added in fp32 in sample order from 0 and divided by np.float32(spp) -- what the
fused call does on the device.  Comparisons are bit for bit unless a test says otherwise."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import scenes
from conftest import GOLDEN, ROOT

MESH2K = os.path.join(GOLDEN, "mesh_2k.3d")
TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")
ERR_INVALID = -1
ALL = ("albedo", "normal", "shading_normal", "depth", "ids")
W, H = 72, 40   # a width that is no multiple of 64
CAMS = {"perspective": dict(eye=(1.2, 0.6, 4.4), look=(-0.2, -0.4, 0.0), fov=55.0),
        "thin_lens": dict(eye=(0.3, 0.2, 4.8), look=(0.0, -0.5, 0.0), fov=50.0, lens_radius=0.08, focal_distance=4.5),
        "orthographic": dict(eye=(0.0, 0.4, 5.0), look=(0.0, 0.0, 0.0), orthographic=True)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def biteq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def aov(gx, scene, w, h, spp, **kw):
    out, st = gx.PathIntegrator(5).RenderAOV(scene, w, h, spp, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, st


def samples(gx, scene, cam, w, h, s_range, medium=-1, chunk_rows=None):
    """camera_rays_device + Scene.intersect for every pixel and every sample of s_range: (rays [S, h, w, 8], prim [S, h, w] int32,
    t [S, h, w], n [S, h, w, 3]) as numpy arrays"""
    dev = torch.device("cuda", scene.device)
    py, px = torch.meshgrid(torch.arange(h, dtype=torch.int32, device=dev), torch.arange(w, dtype=torch.int32, device=dev), indexing="ij")
    px, py = px.reshape(-1).contiguous(), py.reshape(-1).contiguous()
    R, P, T, N = [], [], [], []
    for s in s_range:
        rays, _ = gx.camera_rays_device(gx.camera(**cam), w, h, px, py, torch.full_like(px, s), medium=medium)
        hits = scene.intersect(rays)
        torch.cuda.synchronize()
        R.append(rays.cpu().numpy().reshape(h, w, 8)); P.append(hits.prim.cpu().numpy().reshape(h, w).copy())
        T.append(hits.t.cpu().numpy().reshape(h, w).copy()); N.append(hits.n.cpu().numpy().reshape(h, w, 3).copy())
    return np.stack(R), np.stack(P), np.stack(T), np.stack(N)


def mean(values, spp):
    """sum over the leading (sample) axis in fp32, in order, from 0; then / float(spp)"""
    acc = np.zeros(values.shape[1:], np.float32)
    for v in values:
        acc = acc + v.astype(np.float32)
    return acc / np.float32(spp)


def prim_materials(b, prim):
    """authored material of every hit primitive (-1: a miss, no material, or a GNXR_MAT_NONE material)"""
    d = b.desc()
    tm = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,)).copy()
    sm = np.array([d.spheres[i].material for i in range(d.n_spheres)] + [-1], np.int32)
    types = np.array([d.materials[i].type for i in range(d.n_materials)] + [0], np.int32)
    m = np.where(prim < 0, -1, np.where(prim >= d.n_triangles, sm[np.clip(prim - d.n_triangles, 0, len(sm) - 1)], tm[np.clip(prim, 0, d.n_triangles - 1)]))
    return np.where((m >= 0) & (types[np.clip(m, 0, len(types) - 1)] != 0), m, -1).astype(np.int32)


def albedo_table(gx, b):
    d = b.desc()
    return np.stack([b.material_albedo(i) for i in range(d.n_materials)] + [np.zeros(3, np.float32)])   # [-1] = 0


def expected(gx, b, scene, cam, w, h, spp, s_range=None, medium=-1, albedo=True):
    s_range = range(spp) if s_range is None else s_range
    rays, prim, t, n = samples(gx, scene, cam, w, h, s_range, medium)
    e = {"depth": mean(t, spp), "normal": np.concatenate([mean(n, spp), np.zeros((h, w, 1), np.float32)], -1)}
    mat = prim_materials(b, prim)
    e["ids"] = np.stack([prim[0], mat[0]], -1).astype(np.int32)
    e["coverage"] = mean((prim >= 0).astype(np.float32), spp)
    if albedo:
        e["albedo"] = np.concatenate([mean(albedo_table(gx, b)[mat], spp), e["coverage"][..., None]], -1)
    return e, (rays, prim, t, n, mat)


def check(out, e, keys):
    for k in keys:
        if k == "coverage":
            assert biteq(out["albedo"][..., 3], e[k]), k
        else:
            assert biteq(out[k], e[k]), k


def builders():
    return {"cornell": scenes.cornell, "zoo": scenes.material_zoo, "mesh": lambda: scenes.dragon_cornell(2000, "glass+metal", mesh_path=MESH2K),
            "sphere": lambda: scenes.cornell_sphere("matte"), "sphere_medium": lambda: scenes.cornell_sphere("medium")}


# ---------------------------------------------------------------- CPU
def test_aov_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_render_aov_device", "gnxr_material_albedo"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in gx._abi.PROTOTYPES, name
    # gnxr_aov_buffers is five pointers; the list of gnxr_abi_sizeof is the parent's (tests/test_render_views.py pins its end)
    assert C.sizeof(gx._abi.AovBuffers) == 5 * C.sizeof(C.c_void_p)


def test_aov_rejects_null_arguments_before_any_device_work(gx):
    """a null scene, params or out: GNXR_ERR_INVALID before the handle (a dummy that must not be touched) or the device is looked at;
    so do the checks that need neither: no channel, misalignment, a shard index, null cameras for several views"""
    L = gx.lib()
    buf = (C.c_float * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    dummy = C.c_void_p(base)
    ok = gx.PathIntegrator(5).params(64, 48, 4)
    bufs = gx._abi.AovBuffers(base, None, None, None, None)
    st = gx.Stats()
    A = L.gnxr_render_aov_device
    assert A(None, C.byref(ok), None, None, 1, C.byref(bufs), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, None, None, None, 1, C.byref(bufs), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, 1, None, None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, 1, C.byref(gx._abi.AovBuffers()), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, 1, C.byref(gx._abi.AovBuffers(base + 4, None, None, None, None)), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, 1, C.byref(gx._abi.AovBuffers(None, None, None, base + 2, None)), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, 2, C.byref(bufs), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(ok), None, None, -1, C.byref(bufs), None, C.byref(st)) == ERR_INVALID
    assert A(dummy, C.byref(gx.PathIntegrator(5).params(64, 48, 4, shard_index=1, shard_count=2)), None, None, 1, C.byref(bufs), None, C.byref(st)) == ERR_INVALID
    assert not any(buf)


def test_material_albedo_matches_the_documented_table(gx):
    """gnxr_material_albedo against a numpy fp32 restatement of the table in include/gnxr.h, one material of every type"""
    A = gx._abi
    f = np.float32

    def clamp0(v):
        return np.array([f(0) if x < 0 else f(x) for x in np.asarray(v, f)], f)

    def metal(eta, k):
        eta, k = np.asarray(eta, f), np.asarray(k, f)
        a, b, k2 = eta - f(1), eta + f(1), k * k
        num, den = a * a + k2, b * b + k2
        return (num / den).astype(f)

    kd, kr = (0.3, -0.25, 1.7), (0.9, 0.05, -1.0)
    eta, k = (0.2, 0.924, 1.102), (3.912, 2.452, 2.142)
    cases = [(dict(type=A.MAT_MATTE, kd=kd, sigma=20.0), clamp0(kd)), (dict(type=A.MAT_PLASTIC, kd=kd, ks=(0.4, 0.4, 0.4), urough=0.1), clamp0(kd)),
             (dict(type=A.MAT_DISNEY, kd=kd, eta=(1.5, 0, 0), disney_roughness=0.4), clamp0(kd)), (dict(type=A.MAT_MIRROR, kr=kr), clamp0(kr)),
             (dict(type=A.MAT_GLASS, kr=(0.5, 0.5, 0.5), kt=(0.2, 0.2, 0.2), eta=(1.5, 0, 0)), np.ones(3, f)),
             (dict(type=A.MAT_METAL, eta=eta, k=k, urough=0.01, vrough=0.01), metal(eta, k)), (dict(type=A.MAT_NONE, kd=kd), np.zeros(3, f))]
    for fields, want in cases:
        got = gx.material_albedo(**fields)
        assert got.dtype == np.float32 and biteq(got, want), (fields, got, want)
    # a kd texture does not change the host value; the builder's form reads the material it stored
    assert biteq(gx.material_albedo(type=A.MAT_MATTE, kd=kd, kd_texture=1), clamp0(kd))
    b = gx.SceneBuilder()
    m = b.add_material(type=A.MAT_METAL, eta=eta, k=k, urough=0.01, vrough=0.01)
    assert biteq(b.material_albedo(m), metal(eta, k))
    with pytest.raises(gx.GnxrError):
        gx.material_albedo(type=99)
    assert gx.lib().gnxr_material_albedo(None, (C.c_float * 3)()) == ERR_INVALID


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 16])
@pytest.mark.parametrize("name", ["cornell", "zoo", "mesh", "sphere"])
def test_depth_normal_coverage_ids(gpu, name, spp):
    gx = gpu
    b = builders()[name]()
    scene = gx.Scene(b)
    for cname, cam in CAMS.items():
        out, st = aov(gx, scene, W, H, spp, cameras=[gx.camera(**cam)])
        e, _ = expected(gx, b, scene, cam, W, H, spp, albedo=False)
        check({k: v[0] for k, v in out.items()}, e, ("depth", "normal", "coverage", "ids"))
        assert out["depth"].any() and out["normal"].any() and (out["normal"][..., 3] == 0).all() and (out["shading_normal"][..., 3] == 0).all(), cname
        assert st["camera_samples"] == st["rays_closest"] == W * H * spp and st["passes"] >= 1


@pytest.mark.gpu
def test_constant_albedo_of_every_material_type_and_a_null_material_boundary(gpu):
    gx = gpu
    for name, spp in (("zoo", 16), ("sphere_medium", 4), ("mesh", 4)):
        b = builders()[name]()
        scene = gx.Scene(b)
        cam = CAMS["perspective"]
        out, _ = aov(gx, scene, W, H, spp, cameras=[gx.camera(**cam)], channels=("albedo", "ids"))
        e, (_, prim, _, _, mat) = expected(gx, b, scene, cam, W, H, spp)
        check({k: v[0] for k, v in out.items()}, e, ("albedo", "ids"))
        d = b.desc()
        if name == "zoo":   # every material type is in view
            seen = {d.materials[int(m)].type for m in np.unique(mat) if m >= 0}
            assert seen == {gx._abi.MAT_MATTE, gx._abi.MAT_MIRROR, gx._abi.MAT_GLASS, gx._abi.MAT_METAL, gx._abi.MAT_PLASTIC, gx._abi.MAT_DISNEY}, seen
        if name == "sphere_medium":   # the null-material sphere: a hit with material -1 and albedo 0
            ball = (prim == d.n_triangles).all(0)
            assert ball.any()
            assert (out["ids"][0][ball] == np.array([d.n_triangles, -1])).all()
            assert (out["albedo"][0][ball][:, :3] == 0).all() and (out["albedo"][0][ball][:, 3] == 1).all()


def lambert_poster():
    """Cornell box + a poster with per-vertex uvs that shows the whole image once, on a Lambertian Matte (sigma = 0) whose Kd is the image"""
    import gnxraytracer_amd as gx
    b = scenes.cornell()
    tex = b.add_image_texture(TEX)
    m = b.MatteMaterial((0.5, 0.5, 0.5), 0.0)
    b.set_material_texture(m, "kd", tex)
    poster = np.array([[-2.0, -1.6, -1.2], [1.6, -1.6, -1.6], [1.6, 1.4, -1.6], [-2.0, 1.4, -1.2]], np.float32)
    first = b.add_mesh(poster, np.array([[0, 1, 2], [0, 2, 3]], np.int32), m, uv=[[0, 0], [1, 0], [1, 1], [0, 1]])
    return b, first, m


@pytest.mark.gpu
def test_textured_albedo_is_what_the_lambertian_bsdf_reflects(gpu):
    """LambertianReflection::f is R * InvPi with R the unfiltered Kd lookup at the hit (hasDifferentials == false), so per sample
    albedo * fp32(1 / pi) must be scene.bsdf(...).f bit for bit, for a wi on wo's side of the geometric normal.  spp 1: the mean is the sample."""
    gx = gpu
    b, first, m = lambert_poster()
    scene = gx.Scene(b)
    cam = CAMS["perspective"]
    out, _ = aov(gx, scene, W, H, 1, cameras=[gx.camera(**cam)], channels=("albedo", "ids"))
    rays, prim, t, n = samples(gx, scene, cam, W, H, [0])
    on = (prim[0] == first) | (prim[0] == first + 1)
    assert on.sum() > 200 and (out["ids"][0][on][:, 1] == m).all()
    d = rays[0][..., 4:7]
    side = np.where((-(d * n[0]).sum(-1) > 0)[..., None], n[0], -n[0]).astype(np.float32)
    dev = torch.device("cuda", scene.device)
    r = scene.bsdf(torch.from_numpy(rays[0].reshape(-1, 8)).to(dev), torch.from_numpy(side.reshape(-1, 3)).to(dev).contiguous(),
                   torch.full((W * H, 2), 0.5, device=dev))
    torch.cuda.synchronize()
    f = r.cpu().numpy()[:, 0:3].reshape(H, W, 3)
    alb = out["albedo"][0][..., :3]
    assert biteq((alb * np.float32(1 / np.pi))[on], f[on])
    assert len(np.unique(bits(alb[on]))) > 50   # the image, not one colour
    # everything else in view is constant-Kd: the table
    e, _ = expected(gx, b, scene, cam, W, H, 1)
    assert biteq(out["albedo"][0][~on], e["albedo"][~on])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_shading_normal_without_vertex_normals_is_the_geometric_one(gpu, name):
    """No per-vertex normals: ns comes out of normalize / cross / faceforward of unit-scale vectors, a few dozen fp32 operations on
    well-conditioned values: ~30 x 2^-24 = 2e-6, bound 1e-5 (fivefold margin).  Every pixel of the frame is checked."""
    gx = gpu
    b = builders()[name]()
    scene = gx.Scene(b)
    out, _ = aov(gx, scene, W, H, 1, cameras=[gx.camera(**CAMS["perspective"])])
    ns, n, cov = out["shading_normal"][0][..., :3].astype(np.float64), out["normal"][0][..., :3].astype(np.float64), out["albedo"][0][..., 3]
    hit = cov == 1
    assert hit.sum() > W * H // 2
    print(f"{name}: max | |ns| - 1 | = {np.abs(np.linalg.norm(ns[hit], axis=-1) - 1).max():.3e}, max |ns - n| = {np.abs(ns - n).max():.3e}")
    assert (np.abs(np.linalg.norm(ns[hit], axis=-1) - 1) <= 1e-5).all()
    assert ((ns[hit] * n[hit]).sum(-1) > 0).all()
    assert (np.abs(ns - n) <= 1e-5).all()
    assert (ns[~hit] == 0).all()


@pytest.mark.gpu
def test_shading_normal_with_vertex_normals(gpu):
    """The smooth-shaded balls of render_smooth's scene (no tangents, no uvs on the two balls checked): ns = normalize(b0 n0 + b1 n1 + b2 n2)
    in float64, oriented as Triangle.cpp:228-297 + Material::Bump leave it: SetShadingGeometry flips the GEOMETRIC normal onto ns's side, and
    Bump's faceforward onto that flipped normal then keeps ns.  Within 1e-5 per component (fp32 interpolation, one normalisation and the
    frame's two cross products of unit vectors; same budget as above).  spp 1."""
    gx = gpu
    b = scenes.smooth_cornell(TEX)
    scene = gx.Scene(b)
    cam = CAMS["perspective"]
    out, _ = aov(gx, scene, W, H, 1, cameras=[gx.camera(**cam)], channels=("shading_normal", "normal", "ids"))
    rays, prim, t, n = samples(gx, scene, cam, W, H, [0])
    d = b.desc()
    tri_n = np.ctypeslib.as_array(d.tri_n, shape=(d.n_triangles, 3, 3)).astype(np.float64)
    tri_s = np.ctypeslib.as_array(d.tri_s, shape=(d.n_triangles, 3, 3))
    dev = torch.device("cuda", scene.device)
    hits = scene.intersect(torch.from_numpy(rays[0].reshape(-1, 8)).to(dev))
    torch.cuda.synchronize()
    bary = hits.bary.cpu().numpy().reshape(H, W, 3).astype(np.float64)
    p = prim[0]
    smooth = (p >= 0) & (p < d.n_triangles)
    smooth &= np.where(smooth, np.abs(tri_n[np.clip(p, 0, d.n_triangles - 1)]).sum((-1, -2)) > 0, False)
    smooth &= np.where(smooth, np.abs(tri_s[np.clip(p, 0, d.n_triangles - 1)]).sum((-1, -2)) == 0, False)   # tangents set the frame differently: not this test
    assert smooth.sum() > 150
    want = (bary[..., None] * tri_n[np.clip(p, 0, d.n_triangles - 1)]).sum(-2)
    with np.errstate(invalid="ignore"):   # (pixels outside `smooth` have no normals to interpolate)
        want /= np.linalg.norm(want, axis=-1, keepdims=True)
    ns = out["shading_normal"][0][..., :3].astype(np.float64)
    err = np.abs(ns - want)[smooth]
    print(f"smooth: {smooth.sum()} pixels, max |ns - normalize(sum b_i n_i)| = {err.max():.3e}")
    assert (err <= 1e-5).all()
    # the geometric normal of those hits lies on the shading side, and the two differ (a coarse sphere)
    assert ((ns * out["normal"][0][..., :3]).sum(-1)[smooth] > 0).all() and np.abs(ns - out["normal"][0][..., :3])[smooth].max() > 1e-2


@pytest.mark.gpu
def test_views_equal_single_view_calls_and_the_scene_camera(gpu):
    gx = gpu
    b = scenes.cornell_in_fog()
    scene = gx.Scene(b)
    cams = [CAMS["perspective"], CAMS["thin_lens"], CAMS["orthographic"]]
    media = [-1, 0, -1]
    out, st = aov(gx, scene, W, H, 4, cameras=[gx.camera(**c) for c in cams], media=media)
    assert out["albedo"].shape == (3, H, W, 4) and out["depth"].shape == (3, H, W) and out["ids"].shape == (3, H, W, 2) and st["camera_samples"] == 3 * W * H * 4
    for v, c in enumerate(cams):
        scene.set_camera(**c, medium=media[v])
        one, _ = aov(gx, scene, W, H, 4)
        assert one["albedo"].shape == (H, W, 4) and one["depth"].shape == (H, W)
        single, _ = aov(gx, scene, W, H, 4, cameras=[gx.camera(**c)], media=[media[v]])
        for k in ALL:
            assert biteq(out[k][v], one[k]) and biteq(out[k][v], single[k][0]), (v, k)
        assert one["depth"].any()


@pytest.mark.gpu
def test_results_do_not_depend_on_the_plan_and_ranges_add_up(gpu):
    gx = gpu
    b = scenes.material_zoo()
    scene = gx.Scene(b)
    cam = CAMS["thin_lens"]
    cams = [gx.camera(**cam)]
    spp = 16
    auto, st = aov(gx, scene, W, H, spp, cameras=cams)
    for k in (1, 3, spp):
        o, s = aov(gx, scene, W, H, spp, cameras=cams, samples_per_pass=k)
        assert s["passes"] == -(-spp // k)
        for c in ALL:
            assert biteq(o[c], auto[c]), (k, c)
    lo, _ = aov(gx, scene, W, H, spp, cameras=cams, spp_begin=0, spp_end=8)
    hi, _ = aov(gx, scene, W, H, spp, cameras=cams, spp_begin=8, spp_end=16, samples_per_pass=3)
    e_lo, _ = expected(gx, b, scene, cam, W, H, spp, range(0, 8))
    e_hi, _ = expected(gx, b, scene, cam, W, H, spp, range(8, 16))
    check({k: v[0] for k, v in lo.items()}, e_lo, ("depth", "normal", "albedo", "ids"))
    check({k: v[0] for k, v in hi.items()}, e_hi, ("depth", "normal", "albedo", "ids"))   # ids: sample 8
    for c in ("depth", "normal", "albedo"):
        assert biteq(lo[c][0] + hi[c][0], e_lo[c] + e_hi[c]), c
    assert not biteq(lo["ids"], hi["ids"])   # an anti-aliased edge somewhere: samples 0 and 8 see different primitives


@pytest.mark.gpu
def test_channel_mask(gpu):
    """depth alone carries the bits of the full request; tensors of channels that were not requested, and memory beside the ones that
    were, keep their sentinel"""
    gx = gpu
    scene = gx.Scene(scenes.material_zoo())
    cams = [gx.camera(**CAMS["perspective"])]
    full, _ = aov(gx, scene, W, H, 4, cameras=cams)
    dev = torch.device("cuda", scene.device)
    n = W * H
    # one allocation: [guard | depth | guard], all sentinel-filled
    pool = torch.full((n * 5,), -7.25, dtype=torch.float32, device=dev)
    depth = pool[n:2 * n].view(1, H, W)
    others = {c: torch.full((1, H, W, 4), -7.25, dtype=torch.float32, device=dev) for c in ("albedo", "normal", "shading_normal")}
    out, _ = gx.PathIntegrator(5).RenderAOV(scene, W, H, 4, cameras=cams, channels=("depth",), out={"depth": depth})
    torch.cuda.synchronize()
    assert out["depth"] is depth and set(out) == {"depth"}
    assert biteq(depth.cpu().numpy(), full["depth"])
    host = pool.cpu().numpy()
    assert (host[:n] == -7.25).all() and (host[2 * n:] == -7.25).all()
    assert all((t == -7.25).all().item() for t in others.values())
    for sel in (("ids",), ("normal", "ids"), ("albedo",), ("shading_normal", "depth")):
        o, _ = aov(gx, scene, W, H, 4, cameras=cams, channels=sel)
        for c in sel:
            assert biteq(o[c], full[c]), (sel, c)


@pytest.mark.gpu
def test_refusals_leave_the_buffers_untouched(gpu):
    gx = gpu
    L = gx.lib()
    scene = gx.Scene(scenes.cornell_in_fog())
    dev = torch.device("cuda", scene.device)
    n = W * H
    buf = torch.full((n * 4 + 8,), 3.5, dtype=torch.float32, device=dev)
    host = np.full(n * 4 + 8, 3.5, np.float32)
    base = buf.data_ptr()
    ok = gx.PathIntegrator(5).params(W, H, 4)
    cam2 = (gx.Camera * 2)(gx.camera(), gx.camera(eye=(1, 0, 5)))
    st = gx.Stats()
    A = L.gnxr_render_aov_device
    B = gx._abi.AovBuffers
    calls = [(ok, None, None, 1, B(host.ctypes.data, None, None, None, None)),                  # host memory
             (ok, None, None, 1, B(base, None, None, host.ctypes.data, None)),                  # one of two on the host
             (ok, None, None, 1, B(base + 4, None, None, None, None)),                          # misaligned
             (ok, None, None, 1, B(None, None, None, base + 2, None)),
             (ok, None, None, 1, B(None, None, None, None, None)),                              # no channel
             (gx.PathIntegrator(5).params(W, H, 4, shard_index=1, shard_count=2), None, None, 1, B(base, None, None, None, None)),
             (ok, None, None, 2, B(base, None, None, None, None)),                              # null cameras, two views
             (ok, cam2, (C.c_int32 * 2)(-1, 1), 2, B(None, None, None, base, None)),            # medium out of range (the scene has one)
             (ok, cam2, (C.c_int32 * 2)(-2, 0), 2, B(None, None, None, base, None)),
             (gx.PathIntegrator(5).params(W, H, 4, spp_begin=4), None, None, 1, B(base, None, None, None, None))]   # an empty sample range
    for i, (p, cams, med, v, bufs) in enumerate(calls):
        assert A(scene._h, C.byref(p), cams, med, v, C.byref(bufs), None, C.byref(st)) == ERR_INVALID, i
    torch.cuda.synchronize()
    assert (buf == 3.5).all().item() and (host == 3.5).all()
    # n_views == 0 is a no-op
    assert A(scene._h, C.byref(ok), cam2, None, 0, C.byref(B(base, None, None, None, None)), None, C.byref(st)) == 0 and (buf == 3.5).all().item()
    with pytest.raises(ValueError):
        gx.PathIntegrator(5).RenderAOV(scene, W, H, 4, channels=("depth", "colour"))
    with pytest.raises(ValueError):
        gx.PathIntegrator(5).RenderAOV(scene, W, H, 4, channels=("depth",), out={"depth": torch.zeros((H, W), device="cpu")})


@pytest.mark.gpu
def test_a_render_after_an_aov_call_is_the_render_of_a_fresh_scene(gpu):
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    b = scenes.material_zoo()
    fresh, _ = integ.Render(gx.Scene(b), 64, 48, 8)
    scene = gx.Scene(b)
    integ.Reserve(scene, 64, 48, 8)
    aov(gx, scene, W, H, 16, samples_per_pass=5)
    img, _ = integ.Render(scene, 64, 48, 8)
    assert biteq(img, fresh) and img[..., :3].any()
    aov(gx, scene, 64, 48, 8)
    img2, _ = integ.Render(scene, 64, 48, 8)
    assert biteq(img2, fresh)


@pytest.mark.gpu
def test_full_size_depth_and_ids(gpu):
    """1920 x 1080, spp 4 on the cfg 3 scene: depth and ids against the composition, and the state the call reports -- 32 bytes per camera
    sample of the largest sub-pass plus the running sums -- below 64 bytes per such sample plus the sums"""
    gx = gpu
    b = scenes.dragon_cornell(100000, "glass+metal")
    scene = gx.Scene(b)
    w, h, spp = 1920, 1080, 4
    cam = dict(eye=(0, 0, 5), look=(0, 0, 0), fov=90.0)
    out, st = aov(gx, scene, w, h, spp, cameras=[gx.camera(**cam)])
    e, _ = expected(gx, b, scene, cam, w, h, spp, albedo=False)
    check({k: v[0] for k, v in out.items()}, e, ("depth", "ids", "normal", "coverage"))
    assert out["depth"].any() and (out["ids"][..., 0] >= 0).any()
    per_pass = -(-spp // st["passes"])
    sums = 3 * w * h * 16
    print(f"1920x1080x{spp}: {st['passes']} sub-pass(es), state {st['state_bytes'] / 1e6:.1f} MB, {st['camera_samples'] / st['seconds_render'] / 1e6:.1f} M samples/s")
    assert st["camera_samples"] == w * h * spp
    assert st["state_bytes"] < 64 * w * h * per_pass + sums
