"""Deforming smooth meshes in place: gnxr_skin_vertices_device, gnxr_scene_update_attributes / gnxr_scene_triangle_attributes,
gnxr_scene_recompute_normals and gx.SkinnedMesh.

The header defines all three operation by operation in rounded fp32, so tests/deform_reference.py restates them in numpy float32 and
every comparison here is on bits (biteq; no tolerance anywhere).  Edited scenes are also compared, as tests/test_scene_update.py does,
with the CPU oracle built from the description carrying the edited arrays and walking the device's tree."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import deform_reference as ref
import oracle_lib as ol
import scenes
from conftest import GOLDEN
from test_scene_update import biteq, indices, same_render, vertices

TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
W, H, SPP = 48, 40, 4
f32 = np.float32


# ---------------------------------------------------------------- helpers
class Edited:
    """The builder's description with other vertices and / or per-corner tables (kept alive here)."""

    FIELDS = ("vertices", "tri_uv", "tri_n", "tri_s")

    def __init__(self, builder, **arrays):
        self.builder = builder
        self.arrays = {k: np.ascontiguousarray(v, f32) for k, v in arrays.items() if v is not None}
        assert set(self.arrays) <= set(self.FIELDS)

    def desc(self):
        d = self.builder.desc()
        for k, a in self.arrays.items():
            setattr(d, k, a.ctypes.data_as(C.POINTER(C.c_float)))
        return d


def scene_of(gx, e):
    s = gx.Scene(e.desc())
    s._keep = e
    return s


def table(b, field, cols):
    d = b.desc()
    p = getattr(d, field)
    return np.ctypeslib.as_array(p, shape=(d.n_triangles, cols)).copy() if p else None


def tables(b):
    return table(b, "tri_uv", 6), table(b, "tri_n", 9), table(b, "tri_s", 9)


def tri_ints(b, field):
    d = b.desc()
    return np.ctypeslib.as_array(getattr(d, field), shape=(d.n_triangles,)).copy()


def integrators(gx):
    return {"path": gx.PathIntegrator(5, 1.0, "spatial"), "volpath": gx.VolPathIntegrator(5, 1.0, "spatial"), "whitted": gx.WhittedIntegrator(5),
            "direct": gx.DirectLightingIntegrator("all", 5)}


def oracle_of(b, scene, **arrays):
    o = ol.OracleScene(Edited(b, **arrays))
    o.set_bvh(*scene.bvh())
    return o


def aimed_probes(gx, v, idx, tris, seed):
    """BSDF probes at the given triangles: rays from a point inside the box at seeded points of them, unit wi, samples u"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris)
    bary = rng.dirichlet((1.0, 1.0, 1.0), size=len(tris)).astype(f32)
    p = (v[idx[tris]] * bary[:, :, None]).sum(1)
    o = np.tile(np.array([0.1, 0.2, 2.2], f32), (len(tris), 1))
    rays = gx.make_rays(o, (p - o).astype(f32))
    wi = rng.normal(size=(len(tris), 3))
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(f32)
    return rays, wi, rng.random((len(tris), 2), dtype=f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def device_bsdf(scene, rays, wi, u):
    out = scene.bsdf(dev(rays), dev(wi), dev(u))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_attributes(scene, want):
    got = scene.triangle_attributes()
    for g, w, name in zip(got, want, ("uv", "normals", "tangents")):
        assert (g is None) == (w is None), name
        assert g is None or biteq(g, w), name


def check_edited_scene(gx, scene, b, want, probe_tris, verts=None, which=("path", "volpath", "whitted", "direct")):
    """the device's tables are `want`, and renders and BSDF probes equal those of the oracle built with them on the device's tree"""
    same_attributes(scene, want)
    v = vertices(b) if verts is None else verts
    o = oracle_of(b, scene, vertices=verts, tri_uv=want[0], tri_n=want[1], tri_s=want[2])
    its = integrators(gx)
    for name in which:
        same_render(gx, its[name], scene, o, W, H, SPP)
    rays, wi, u = aimed_probes(gx, v, indices(b), probe_tris, seed=5)
    rows, orows = device_bsdf(scene, rays, wi, u), o.bsdf_probe(rays, wi, u)
    assert (orows[:, 13] == 1).mean() >= 0.25
    assert biteq(rows, orows)


def shading_normals(gx, scene):
    out, _ = gx.PathIntegrator(5, 1.0, "spatial").RenderAOV(scene, W, H, 1, channels=("shading_normal",))
    torch.cuda.synchronize()
    return out["shading_normal"].cpu().numpy()


def smooth_case(gx):
    """smooth_cornell, the triangles of its mirror ball and of its textured ball, and an edit of both: normals of a sub-range of the
    mirror ball tilted and renormalised, the uvs of the textured ball shrunk towards the image's centre"""
    b = scenes.smooth_cornell(TEX)
    d = b.desc()
    mat = tri_ints(b, "tri_material")
    types = [d.materials[i].type for i in range(d.n_materials)]
    ball = np.flatnonzero(mat == types.index(gx._abi.MAT_MIRROR))
    uv0, n0, s0 = tables(b)
    textured = np.flatnonzero((mat == max(i for i, t in enumerate(types) if t == gx._abi.MAT_PLASTIC)) & ref.smooth_rows(n0))
    assert len(ball) > 40 and len(textured) > 40 and (np.diff(ball) == 1).all() and (np.diff(textured) == 1).all()
    sub = ball[len(ball) // 4: 3 * len(ball) // 4]
    n_new = n0[sub].reshape(-1, 3) + np.array([0.35, 0.1, -0.2], f32)
    n_new = (n_new / np.linalg.norm(n_new, axis=1, keepdims=True)).astype(f32).reshape(-1, 9)
    uv_new = (uv0[textured] * f32(0.5) + f32(0.25)).astype(f32)
    want = (uv0.copy(), n0.copy(), s0.copy())
    want[0][textured] = uv_new
    want[1][sub] = n_new
    return b, sub, n_new, textured, uv_new, want


# ---------------------------------------------------------------- CPU
def test_entry_points_exported_and_reject_null(gx):
    """Checked before the device is touched: GNXR_ERR_INVALID without a GPU."""
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_scene_update_attributes", "gnxr_scene_recompute_normals", "gnxr_skin_vertices_device", "gnxr_scene_triangle_attributes"):
        assert hasattr(lib, name), name
    L = gx.lib()
    rows = np.zeros((2, 9), f32)
    n = C.c_int64(0)
    assert L.gnxr_scene_update_attributes(None, 0, 2, None, C.c_void_p(rows.ctypes.data), None, None) == ERR_INVALID
    assert L.gnxr_scene_triangle_attributes(None, 1, None, 0, C.byref(n)) == ERR_INVALID
    assert L.gnxr_scene_recompute_normals(None, 0, None) == ERR_INVALID
    assert L.gnxr_skin_vertices_device(None, None, None, None, None, None, None, None, None) == ERR_INVALID
    p = gx._abi.SkinParams(C.sizeof(gx._abi.SkinParams) + 4, 1, 1, 0)   # a record of another size
    assert L.gnxr_skin_vertices_device(C.byref(p), None, None, None, None, None, None, None, None) == ERR_INVALID


def test_abi_mirror(gx):
    A = gx._abi
    assert A.NORMALS_FLIP == 1
    assert [f[0] for f in A.SkinParams._fields_] == ["struct_size", "n_vertices", "n_bones", "n_morphs"] and C.sizeof(A.SkinParams) == 16
    assert gx.lib().gnxr_abi_version() == 5 and gx.lib().gnxr_abi_sizeof(14) == -1
    for name in ("gnxr_scene_update_attributes", "gnxr_scene_recompute_normals", "gnxr_skin_vertices_device", "gnxr_scene_triangle_attributes"):
        assert name in A.PROTOTYPES


def test_wrappers_reject_other_inputs_before_the_library(gx):
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_vertices, s.n_triangles = None, 0, 8, 4
    for kw in ({}, dict(normals=np.zeros((2, 9), np.float64)), dict(normals=np.zeros((2, 6), f32)), dict(uv=np.zeros((2, 6), f32), normals=np.zeros((3, 9), f32)),
               dict(uv="uv")):
        with pytest.raises(ValueError):
            s.update_attributes(**kw)
    with pytest.raises((ValueError, TypeError)):
        s.recompute_normals(stream=-3)


def test_reference_skin_identity():
    rng = np.random.default_rng(1)
    rest = rng.normal(size=(100, 3)).astype(f32)
    rest[0] = (0.0, 1e-40, -1e-40)   # a zero and subnormals (a -0 would come back as +0: P starts from +0)
    ident = np.tile(np.eye(3, 4, dtype=f32), (3, 1, 1))
    bi = rng.integers(0, 3, size=(100, 4)).astype(np.int32)
    bw = np.zeros((100, 4), f32)
    bw[np.arange(100), rng.integers(0, 4, size=100)] = 1
    out = ref.skin(rest, bi, bw, ident)
    assert biteq(out, rest)   # 0 + 1 * (((1 x + 0 y) + 0 z) + 0): every step is exact
    with pytest.raises(ValueError):
        ref.skin(rest, bi + 3, bw, ident)


def test_reference_normals_on_an_ellipsoid():
    """A wrong but self-consistent definition must not pass: on the 320-triangle icosphere scaled to an ellipsoid the reference normals lie
    within 15 degrees of the analytic ones, with no corner keeping its old normal; FLIP negates every written component."""
    v, idx = ref.icosphere(2)
    assert len(idx) == 320 and len(v) == 162
    scale = np.array([1.6, 0.7, 1.1], f32)
    # (a seeded wobble of 0.2 % breaks the mirror symmetries, under which a component of a sum can cancel to a zero whose sign FLIP keeps)
    v2 = (v * scale + np.random.default_rng(2).normal(size=v.shape).astype(f32) * f32(0.002)).astype(f32)
    old = np.tile(np.array([0, 0, 1], f32), (320, 3))
    got, kept = ref.recompute_normals(v2, idx, old)
    assert kept == 0
    analytic = (v2.astype(np.float64) / scale.astype(np.float64) ** 2)[idx].reshape(-1, 3)
    analytic /= np.linalg.norm(analytic, axis=1, keepdims=True)
    cos = (got.reshape(-1, 3).astype(np.float64) * analytic).sum(1)
    print(f"largest angle to the analytic normal: {np.degrees(np.arccos(cos.min())):.2f} degrees")
    assert cos.min() > np.cos(np.radians(15.0))
    assert np.allclose(np.linalg.norm(got.reshape(-1, 3).astype(np.float64), axis=1), 1.0, atol=1e-6)
    flipped, kept_f = ref.recompute_normals(v2, idx, old, flip=True)
    assert kept_f == 0 and biteq(flipped, -got)


def test_reference_normals_flat_triangles_and_creases():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]], f32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    old = np.tile(np.array([0, 0, 1], f32), (2, 3))
    both, _ = ref.recompute_normals(v, idx, old)
    assert biteq(both[0, 0:3], both[1, 0:3]) and biteq(both[0, 6:9], both[1, 3:6])   # the shared vertices carry one normal
    flat = old.copy()
    flat[1] = 0
    one, _ = ref.recompute_normals(v, idx, flat)
    assert not one[1].any() and not biteq(one[0], both[0])   # the flat triangle is not written and takes no part


# ---------------------------------------------------------------- GPU: skinning
def skin_case(V, B, M, seed):
    rng = np.random.default_rng(seed)
    rest = rng.normal(size=(V, 3)).astype(f32)
    bones = rng.normal(size=(B, 3, 4)).astype(f32)
    bi = rng.integers(0, B, size=(V, 4)).astype(np.int32)
    bw = rng.random((V, 4), dtype=f32)
    bw /= bw.sum(1, keepdims=True)
    kind = np.arange(V) % 5
    bw[kind == 0] = (1, 0, 0, 0)                                   # one bone
    bi[kind == 1] = bi[kind == 1][:, :1]                            # four slots on one bone
    bw[kind == 2, 1] = 0; bw[kind == 2, 3] = 0                      # zero-weight slots whose index must be ignored
    bi[kind == 2, 1] = -7; bi[kind == 2, 3] = -7
    bi[kind == 0, 1:] = -7
    bw[kind == 3] *= f32(1.7)                                       # unnormalised weights (kind 4: a plain four-bone blend)
    md = rng.normal(size=(M, V, 3)).astype(f32) * f32(0.1) if M else None
    mw = rng.random(M, dtype=f32) if M else None
    return rest, bi, bw, bones, md, mw


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, 3])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 5000])
def test_skin_matches_reference(gpu, V, B, M):
    rest, bi, bw, bones, md, mw = skin_case(V, B, M, seed=V + 10 * B + M)
    want = ref.skin(rest, bi, bw, bones, md, mw)
    got = gpu.skin_vertices(dev(rest), dev(bi), dev(bw), dev(bones), dev(md) if M else None, dev(mw) if M else None)
    torch.cuda.synchronize()
    assert biteq(got.cpu().numpy(), want)
    out = torch.full((V, 3), -7.25, dtype=torch.float32, device="cuda:0")   # `out` and the (B, 12) form of the matrices
    assert gpu.skin_vertices(dev(rest), dev(bi), dev(bw), dev(bones.reshape(B, 12)), dev(md) if M else None, dev(mw) if M else None, out=out) is out
    torch.cuda.synchronize()
    assert biteq(out.cpu().numpy(), want)


@pytest.mark.gpu
def test_skin_out_of_range_index(gpu):
    """An index outside [0, B) in a used slot is never dereferenced: GNXR_ERR_INVALID; the next valid call on the same buffers is right."""
    rest, bi, bw, bones, _, _ = skin_case(300, 5, 0, seed=3)
    d_rest, d_bw, d_bones = dev(rest), dev(bw), dev(bones)
    out = torch.zeros((300, 3), dtype=torch.float32, device="cuda:0")
    for bad in (5, -1, 2 ** 30):
        bi_bad = bi.copy()
        bi_bad[4::5, 2] = bad     # kind 4: every slot is used
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
            gpu.skin_vertices(d_rest, dev(bi_bad), d_bw, d_bones, out=out)
    gpu.skin_vertices(d_rest, dev(bi), d_bw, d_bones, out=out)
    torch.cuda.synchronize()
    assert biteq(out.cpu().numpy(), ref.skin(rest, bi, bw, bones))
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):   # the output must not overlap an input
        gpu.skin_vertices(d_rest, dev(bi), d_bw, d_bones, out=d_rest)
    with pytest.raises(ValueError):
        gpu.skin_vertices(d_rest, dev(bi), d_bw.double(), d_bones)


# ---------------------------------------------------------------- GPU: attributes
@pytest.mark.gpu
@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("rebuilt", [False, True])
def test_update_attributes_matches_oracle(gpu, source, rebuilt):
    """Normals of a sub-range of one ball and the uvs of the textured ball replaced, from host or device memory, on the tree the scene was
    created with and on a rebuilt one (the leaf order then exists only on the device)."""
    b, sub, n_new, textured, uv_new, want = smooth_case(gpu)
    scene = gpu.Scene(b)
    before = gpu.PathIntegrator(5, 1.0, "spatial").Render(scene, W, H, SPP)[0]
    if rebuilt:
        scene.rebuild_bvh()
    conv = dev if source == "torch" else (lambda a: a)
    scene.update_attributes(normals=conv(n_new), first_triangle=int(sub[0]))
    scene.update_attributes(uv=conv(uv_new), first_triangle=int(textured[0]))
    check_edited_scene(gpu, scene, b, want, np.concatenate([sub, textured]))
    assert not biteq(gpu.PathIntegrator(5, 1.0, "spatial").Render(scene, W, H, SPP)[0], before)
    if not rebuilt:   # the first-hit shading normals are those of a scene created with the arrays (the same build: the same tree)
        fresh = scene_of(gpu, Edited(b, tri_uv=want[0], tri_n=want[1]))
        sn = shading_normals(gpu, scene)
        assert biteq(sn, shading_normals(gpu, fresh)) and not biteq(sn, shading_normals(gpu, gpu.Scene(b)))


@pytest.mark.gpu
def test_update_attributes_identity_and_sub_range(gpu):
    """Re-sending the rows a scene holds changes nothing; a sub-range edit equals the full-range edit with the other rows re-sent."""
    b, sub, n_new, textured, uv_new, want = smooth_case(gpu)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    scene = gpu.Scene(b)
    before, st0 = integ.Render(scene, W, H, SPP)
    uv0, n0, s0 = tables(b)
    scene.update_attributes(uv=uv0, normals=n0, tangents=s0)
    same_attributes(scene, (uv0, n0, s0))
    after, st1 = integ.Render(scene, W, H, SPP)
    assert biteq(after, before) and (st0["rays_closest"], st0["rays_any"]) == (st1["rays_closest"], st1["rays_any"])
    s_sub, s_full = gpu.Scene(b), gpu.Scene(b)
    s_sub.update_attributes(normals=n_new, first_triangle=int(sub[0]))
    s_sub.update_attributes(uv=uv_new, first_triangle=int(textured[0]))
    s_full.update_attributes(uv=want[0], normals=want[1], tangents=want[2])
    same_attributes(s_sub, want)
    same_attributes(s_full, want)
    same_render(gpu, integ, s_sub, s_full, W, H, SPP)


@pytest.mark.gpu
def test_update_attributes_refusals(gpu):
    """Every refusal leaves triangle_attributes() and a render as they were."""
    b, sub, n_new, textured, uv_new, want = smooth_case(gpu)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    scene = gpu.Scene(b)
    before = integ.Render(scene, W, H, SPP)[0]
    t0 = tables(b)
    nt = scene.n_triangles
    light = np.flatnonzero(tri_ints(b, "tri_light") >= 0)
    flat = np.flatnonzero(~ref.own_attributes(*t0, nt))
    assert len(light) and len(flat)
    L, h = gpu.lib(), scene._h
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.gnxr_scene_update_attributes(h, 0, 2, None, None, None, None) == ERR_INVALID            # nothing given
    assert L.gnxr_scene_update_attributes(h, 0, 0, None, None, None, None) == 0                      # ... but n == 0 is a no-op
    for first, cnt in ((-1, 2), (nt - 1, 2), (nt, 1)):
        assert L.gnxr_scene_update_attributes(h, first, cnt, None, p(n_new), None, None) == ERR_INVALID
    d_uv = dev(uv_new)
    assert L.gnxr_scene_update_attributes(h, int(textured[0]), len(uv_new), C.c_void_p(d_uv.data_ptr()), p(want[1][textured]), None, None) == ERR_INVALID   # mixed sides
    unsupported = [
        dict(normals=np.tile(np.array([0, 1, 0], f32), (1, 3)), first_triangle=int(flat[0])),        # a flat triangle would become smooth
        dict(normals=np.zeros((1, 9), f32), first_triangle=int(sub[0])),                             # a smooth triangle would become flat
        dict(uv=np.tile(ref.UV_DEFAULT * f32(0.5), (1, 1)), first_triangle=int(flat[0])),            # default uvs would become custom
        dict(normals=np.tile(np.array([0, -1, 0], f32), (1, 3)), first_triangle=int(light[0])),      # normals on an emissive triangle
        dict(tangents=np.tile(np.array([1, 0, 0], f32), (1, 3)), first_triangle=int(light[0])),      # tangents on an emissive triangle
    ]
    for kw in unsupported:
        with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
            scene.update_attributes(**kw)
    same_attributes(scene, t0)
    assert biteq(integ.Render(scene, W, H, SPP)[0], before)
    # a table the scene was created without
    plain = gpu.Scene(scenes.cornell())
    assert plain.triangle_attributes() == (None, None, None)
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_UNSUPPORTED}"):
        plain.update_attributes(normals=np.tile(np.array([0, 1, 0], f32), (1, 3)))
    # -0 in a normal row is a set bit, as at creation: the triangle stays smooth
    z = np.zeros((1, 9), f32); z[0, 4] = -0.0
    scene.update_attributes(normals=z, first_triangle=int(sub[0]))
    assert biteq(scene.triangle_attributes()[1][sub[0]], z[0])


@pytest.mark.gpu
def test_update_attributes_on_replicas(gpu):
    """Device 0 listed twice (rows are dealt over the replicas): the edits reach both copies."""
    b, sub, n_new, textured, uv_new, want = smooth_case(gpu)
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    single = gpu.Scene(b)
    single.update_attributes(uv=want[0], normals=want[1])
    single.recompute_normals()
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(b)
        integ.Render(multi, 16, 12, 1)
        multi.update_attributes(normals=dev(n_new), first_triangle=int(sub[0]))
        multi.update_attributes(uv=uv_new, first_triangle=int(textured[0]))
        multi.recompute_normals()
        same_render(gpu, integ, multi, single, W, H, SPP)
        same_attributes(multi, single.triangle_attributes())
    finally:
        gpu.init(0)


# ---------------------------------------------------------------- GPU: normals
WHITE = (0.8, 0.8, 0.8)
UP = np.array([0, 0, 1], f32)


def mesh_scene(gx, v, idx, smooth=None, normals=True):
    """a one-mesh scene whose smooth triangles (all, or the mask) start with the placeholder normal (0, 0, 1); -> builder, scene, its tri_n"""
    b = gx.SceneBuilder()
    b.add_mesh(v, idx, b.MatteMaterial(WHITE, 60.0), normals=np.tile(UP, (len(v), 1)) if normals else None)
    if not normals:
        return b, gx.Scene(b), None
    tri_n = table(b, "tri_n", 9)
    if smooth is not None:
        tri_n[~smooth] = 0
    return b, scene_of(gx, Edited(b, tri_n=tri_n)), tri_n


def check_normals(gx, v, idx, v2, smooth=None, flip=False, min_kept=0, max_kept=None):
    b, scene, tri_n = mesh_scene(gx, v, idx, smooth)
    scene.update_vertices(v2)
    scene.recompute_normals(flip=flip)
    want, kept = ref.recompute_normals(v2, idx, tri_n, flip)
    assert kept >= min_kept and (max_kept is None or kept <= max_kept), kept
    got = scene.triangle_attributes()[1]
    assert biteq(got, want), f"first differing triangle: {int(np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0])}"
    return b, scene, want


def grid_mesh(nx, ny, seed):
    """a bumpy (nx x ny)-cell grid with shared vertices: 2 nx ny triangles"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx + 1, dtype=f32), np.arange(ny + 1, dtype=f32), indexing="ij")
    v = np.stack([x.ravel() * f32(0.1), y.ravel() * f32(0.1), rng.normal(size=x.size).astype(f32) * f32(0.03)], 1).astype(f32)
    idx = []
    for i in range(nx):
        for j in range(ny):
            a, c = i * (ny + 1) + j, (i + 1) * (ny + 1) + j
            idx += [[a, c, c + 1], [a, c + 1, a + 1]]
    return v, np.asarray(idx, np.int32)


def wobble(v, seed, amount=0.02):
    return (v + np.random.default_rng(seed).normal(size=v.shape).astype(f32) * f32(amount)).astype(f32)


@pytest.mark.gpu
def test_normals_one_triangle(gpu):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    v2 = np.array([[0.1, 0, 0.3], [1, 0.2, 0], [0, 1, -0.4]], f32)
    _, scene, want = check_normals(gpu, v, np.array([[0, 1, 2]], np.int32), v2, max_kept=0)
    assert biteq(want[0, 0:3], want[0, 3:6]) and not biteq(want[0, 0:3], UP)


@pytest.mark.gpu
def test_normals_shared_edge_against_crease(gpu):
    """Two triangles sharing an edge through shared indices are smooth across it; the same two with duplicated vertices are a crease."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], f32)
    v2 = np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0.6], [0, 1, 0]], f32)
    _, _, shared = check_normals(gpu, v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), v2, max_kept=0)
    dup = np.array([0, 1, 2, 0, 2, 3])
    _, _, crease = check_normals(gpu, v[dup], np.arange(6, dtype=np.int32).reshape(2, 3), v2[dup], max_kept=0)
    assert biteq(shared[0, 0:3], shared[1, 0:3]) and not biteq(crease[0, 0:3], crease[1, 0:3]) and not biteq(shared, crease)


@pytest.mark.gpu
def test_normals_icosphere_renders_match_oracle(gpu):
    """The 320-triangle icosphere in the Cornell box under a seeded deformation: normals against the reference (no corner keeps its old
    one), then the four integrators against the oracle built with the moved vertices and the reference normals."""
    b = scenes.cornell()
    sv, sidx = ref.icosphere(2, 0.9)
    first_v = b.desc().n_vertices
    first_t = b.add_mesh(sv + np.array([0.2, -1.2, 0.3], f32), sidx, b.MirrorMaterial((0.9, 0.9, 0.9)), normals=sv)
    scene = gpu.Scene(b)
    v, idx, n0 = vertices(b), indices(b), table(b, "tri_n", 9)
    assert first_t + 320 == len(idx) and ref.smooth_rows(n0).sum() == 320
    v2 = v.copy()
    c = v[first_v:].mean(0)
    v2[first_v:] = wobble((v[first_v:] - c) * np.array([1.3, 0.8, 1.0], f32) + c, seed=7, amount=0.03)
    scene.update_vertices(v2[first_v:], first_vertex=first_v)
    scene.recompute_normals()
    want, kept = ref.recompute_normals(v2, idx, n0)
    assert kept == 0 and not biteq(want, n0)
    check_edited_scene(gpu, scene, b, (None, want, None), np.arange(first_t, first_t + 320), verts=v2)


@pytest.mark.gpu
def test_normals_fan_of_valence_300(gpu):
    """One vertex named by 300 triangles: its list is longer than a wave and than a block."""
    rng = np.random.default_rng(4)
    ang = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    rim = np.stack([np.cos(ang), np.sin(ang), rng.normal(size=300) * 0.05], 1)
    v = np.concatenate([[[0, 0, 0.4]], rim]).astype(f32)
    idx = np.array([[0, 1 + i, 1 + (i + 1) % 300] for i in range(300)], np.int32)
    check_normals(gpu, v, idx, wobble(v, seed=5), max_kept=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_smooth", [255, 256, 257])
def test_normals_smooth_among_flat(gpu, n_smooth):
    """Flat triangles that share vertices with smooth ones take no part in the sums and their rows stay zero."""
    v, idx = grid_mesh(14, 14, seed=6)
    smooth = np.zeros(len(idx), bool)
    smooth[np.random.default_rng(n_smooth).permutation(len(idx))[:n_smooth]] = True
    _, _, want = check_normals(gpu, v, idx, wobble(v, seed=8), smooth=smooth, max_kept=0)
    assert not want[~smooth].any() and ref.smooth_rows(want).sum() == n_smooth
    all_smooth, _ = ref.recompute_normals(wobble(v, seed=8), idx, np.tile(UP, (len(idx), 3)))
    assert not biteq(all_smooth[smooth], want[smooth])   # (with the flat ones taking part the sums would differ)


@pytest.mark.gpu
def test_normals_degenerate_sums(gpu):
    """A zero-area triangle at a smooth vertex adds nothing; two exactly opposite faces sum to zero and their corners keep their normals."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.2], [2, 0, 0], [3, 0.5, 0]], f32)
    v2 = v.copy(); v2[2] = (0.1, 1, 0.5); v2[4] = v2[3]                     # triangle (1, 3, 4) collapses: vertex 3 == vertex 4
    idx = np.array([[0, 1, 2], [1, 3, 4]], np.int32)
    _, _, want = check_normals(gpu, v, idx, v2, min_kept=2)                  # corners 3 and 4 have a zero sum: kept
    assert biteq(want[1, 3:9], np.tile(UP, 2)) and biteq(want[1, 0:3], want[0, 3:6])
    back = np.array([[0, 1, 2], [0, 2, 1]], np.int32)                         # the same face, both ways round
    _, _, want = check_normals(gpu, v[:3], back, v2[:3], min_kept=6)
    assert biteq(want, np.tile(UP, (2, 3)))


@pytest.mark.gpu
def test_normals_flip_repeat_and_rebuild(gpu):
    """FLIP negates; a second call gives the same bits; after rebuild_bvh() the result is the same (the table stores authoring ids)."""
    v, idx = grid_mesh(9, 7, seed=9)
    v2 = wobble(v, seed=10)
    _, scene, want = check_normals(gpu, v, idx, v2, max_kept=0)
    _, flipped_scene, flipped = check_normals(gpu, v, idx, v2, flip=True, max_kept=0)
    assert biteq(flipped, -want)
    scene.recompute_normals()
    assert biteq(scene.triangle_attributes()[1], want)
    scene.rebuild_bvh()
    assert biteq(scene.triangle_attributes()[1], want)
    scene.recompute_normals()
    assert biteq(scene.triangle_attributes()[1], want)
    v3 = wobble(v, seed=11)
    scene.update_vertices(v3)
    scene.recompute_normals(flip=True)
    assert biteq(scene.triangle_attributes()[1], ref.recompute_normals(v3, idx, want, flip=True)[0])
    with pytest.raises(gpu.GnxrError, match=f"error {ERR_INVALID}"):
        gpu._check(gpu.lib().gnxr_scene_recompute_normals(scene._h, 2, None))


@pytest.mark.gpu
def test_normals_follow_set_geometry(gpu):
    """After set_geometry() with another index array the adjacency is the new mesh's."""
    v, idx = grid_mesh(8, 8, seed=12)
    v2 = wobble(v, seed=13)
    _, scene, _ = check_normals(gpu, v, idx, v2, max_kept=0)
    idx2 = np.ascontiguousarray(idx[::-1][:, [1, 2, 0]][: len(idx) - 5])   # another order, rotated corners, fewer triangles
    n2 = np.tile(UP, (len(idx2), 3))
    scene.set_geometry(v2, idx2, 0, normals=n2)
    scene.recompute_normals()
    want, kept = ref.recompute_normals(v2, idx2, n2)
    assert kept == 0 and biteq(scene.triangle_attributes()[1], want)


@pytest.mark.gpu
def test_normals_without_table_is_a_no_op(gpu):
    v, idx = grid_mesh(3, 3, seed=14)
    _, scene, _ = mesh_scene(gpu, v, idx, normals=False)
    scene.update_vertices(wobble(v, seed=15))
    scene.recompute_normals()
    assert scene.triangle_attributes() == (None, None, None)


# ---------------------------------------------------------------- GPU: the chain
@pytest.mark.gpu
def test_skinned_mesh_equals_the_chain(gpu):
    """SkinnedMesh.pose for three poses of the mirror ball of smooth_cornell (two bones, weights blending along the ball's height) against
    the explicit chain skin_vertices -> update_vertices -> recompute_normals on a second scene: vertices, attributes, a Path render; and
    the returned previous tensor gives the motion vectors of a hand-kept previous array."""
    b, _, _, _, _, _ = smooth_case(gpu)
    mat = tri_ints(b, "tri_material")
    d = b.desc()
    mirror = [d.materials[i].type for i in range(d.n_materials)].index(gpu._abi.MAT_MIRROR)
    v, idx = vertices(b), indices(b)
    used = np.unique(idx[mat == mirror])
    lo, n = int(used[0]), len(used)
    assert (used == np.arange(lo, lo + n)).all()
    rest = v[lo:lo + n]
    h = (rest[:, 1] - rest[:, 1].min()) / (rest[:, 1].max() - rest[:, 1].min())
    bw = np.stack([h, 1 - h, np.zeros(n), np.zeros(n)], 1).astype(f32)
    bi = np.tile(np.array([0, 1, -7, -7], np.int32), (n, 1))
    c = rest.mean(0)

    def bones(angle, lift):
        ca, sa = np.cos(angle), np.sin(angle)
        r = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
        top = np.concatenate([r, (c - r @ c + np.array([0, lift, 0]))[:, None]], 1)
        return np.stack([top, np.eye(3, 4)]).astype(f32)

    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    s1, s2 = gpu.Scene(b), gpu.Scene(b)
    d_rest, d_bi, d_bw = dev(rest), dev(bi), dev(bw)
    sk = gpu.SkinnedMesh(s1, v, d_rest, d_bi, d_bw, first_vertex=lo)
    hand_prev, hand_cur = v.copy(), v.copy()
    n0 = table(b, "tri_n", 9)
    for k, (angle, lift) in enumerate(((0.4, 0.1), (0.9, 0.25), (-0.3, 0.0))):
        d_bones = dev(bones(angle, lift))
        prev = sk.pose(d_bones)
        moved = gpu.skin_vertices(d_rest, d_bi, d_bw, d_bones)
        s2.update_vertices(moved, first_vertex=lo)
        s2.recompute_normals()
        torch.cuda.synchronize()
        hand_prev, hand_cur = hand_cur, hand_cur.copy()
        hand_cur[lo:lo + n] = ref.skin(rest, bi, bw, bones(angle, lift))
        assert biteq(sk.vertices.cpu().numpy(), hand_cur) and biteq(prev.cpu().numpy(), hand_prev) and biteq(moved.cpu().numpy(), hand_cur[lo:lo + n])
        same_attributes(s1, s2.triangle_attributes())
        n0, kept = ref.recompute_normals(hand_cur, idx, n0)
        assert biteq(s1.triangle_attributes()[1], n0)
        same_render(gpu, integ, s1, s2, W, H, SPP)
        m1 = s1.motion(W, H, s1.camera, prev_vertices=prev)
        m2 = s2.motion(W, H, s2.camera, prev_vertices=dev(hand_prev))
        torch.cuda.synchronize()
        for ch in m1:
            assert biteq(m1[ch].cpu().numpy().view(np.float32), m2[ch].cpu().numpy().view(np.float32)), (k, ch)
    assert not biteq(hand_cur, v)
