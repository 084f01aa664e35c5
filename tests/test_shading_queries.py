"""Shading queries on device memory: gnxr_bsdf_device / gnxr_light_sample_device / gnxr_light_le_device and Scene.bsdf / sample_light /
light_le.

The device's BSDF and light code (device_bsdf.h, device_lights.h) against the goldens recorded from the compiled reference and against
the CPU oracle's probes, function by function instead of through images.  Every comparison is bit for bit (NaN equal to NaN) on whole
records; the columns of the device results are in the order of the oracle probes' output."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import GOLDEN, golden

TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")
ERR_INVALID, ERR_NO_DEVICE = -1, -2
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR = 1, 2, 4, 8, 16
REFLECTION_ONLY = BSDF_REFLECTION | BSDF_DIFFUSE | BSDF_GLOSSY | BSDF_SPECULAR
SPECULAR_ONLY = BSDF_SPECULAR | BSDF_REFLECTION | BSDF_TRANSMISSION


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def mismatch(a, b):
    """rows that differ (for the assertion message)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    rows = np.nonzero(bad.reshape(len(a), -1).any(1))[0]
    return f"{len(rows)} of {len(a)} rows differ, first {rows[:5].tolist()}, columns {sorted(set(np.nonzero(bad.reshape(len(a), -1))[1].tolist()))}"


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def probes(n, seed, tmax=np.inf):
    """n seeded BSDF probes: rays from inside the box (scenes.random_rays), unit directions wi, samples u in [0, 1)"""
    rng = np.random.default_rng(1000 + seed)
    rays = scenes.random_rays(n, seed=seed, tmax=tmax)
    wi = rng.normal(size=(n, 3))
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    u = rng.random((n, 2), dtype=np.float32)
    return rays, wi, u


def synthetic_differentials(rays, eps_milli):
    """the offset rays gnxo_bsdf_probe builds for `flags | (eps_milli << 8)`: rx / ryOrigin = o, rxDirection = d + (eps, 0, 0),
    ryDirection = d + (0, eps, 0), eps = eps_milli / 1000 in float32"""
    eps = np.float32(eps_milli) / np.float32(1000.0)
    o, d = rays[:, 0:3], rays[:, 4:7]
    rxd, ryd = d.copy(), d.copy()
    rxd[:, 0] = d[:, 0] + eps
    ryd[:, 1] = d[:, 1] + eps
    return np.ascontiguousarray(np.concatenate([o, rxd, o, ryd], 1), np.float32)


def light_probes(n, seed):
    """n seeded light probes inside the Cornell box: reference points, unit normals, samples, unit query directions"""
    rng = np.random.default_rng(2000 + seed)
    p = rng.uniform(-2.4, 2.4, (n, 3)).astype(np.float32)
    nn, wq = rng.normal(size=(2, n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)
    wq = (wq / np.linalg.norm(wq, axis=1, keepdims=True)).astype(np.float32)
    return p, nn, rng.random((n, 2), dtype=np.float32), wq


def dbsdf(scene, rays, wi, u, flags=31, diffs=None, **kw):
    out = scene.bsdf(dev(rays), dev(wi), dev(u), flags, differentials=None if diffs is None else dev(diffs), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def dlight(scene, li, p, n, u, wq, strategy):
    out = scene.sample_light(li, dev(p), dev(n), dev(u), dev(wq), strategy=strategy)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def env_scene():
    b = scenes.cornell(sky=True)
    b.AddInfLight(os.path.join(GOLDEN, "env_100x50.hdr"))
    return b


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_bsdf_device", "gnxr_light_sample_device", "gnxr_light_le_device"):
        assert hasattr(lib, name), name
    assert gx.lib().gnxr_abi_sizeof(12) == C.sizeof(gx._abi.BsdfResult) == 64
    assert gx.lib().gnxr_abi_sizeof(13) == C.sizeof(gx._abi.LightResult) == 48
    assert gx.lib().gnxr_abi_sizeof(11) == C.sizeof(gx._abi.LiSample)
    for i, st in gx._abi.ABI_STRUCTS_SHADING.items():
        assert i >= len(gx._abi.ABI_STRUCTS) and gx.lib().gnxr_abi_sizeof(i) == C.sizeof(st), st.__name__
    assert gx.lib().gnxr_abi_sizeof(14) == -1
    assert gx.lib().gnxr_abi_version() == 5


def test_rejects_bad_arguments_before_any_device_work(gx):
    """A null scene, a null array with n > 0, n < 0, a flags / strategy value out of range and a misaligned pointer are refused with
    GNXR_ERR_INVALID before the library looks at the handle or the device (the handle below is a dummy that a call must not touch);
    n == 0 is a no-op.  What is decided only with the runtime -- are these device pointers -- reports GNXR_ERR_NO_DEVICE on a box
    without a GPU: there is no CPU fallback."""
    L = gx.lib()
    buf = (C.c_float * 256)()
    base = (C.addressof(buf) + 15) & ~15
    p, dummy, odd = C.c_void_p(base), C.c_void_p(base), C.c_void_p(base + 4)
    B, S, E = L.gnxr_bsdf_device, L.gnxr_light_sample_device, L.gnxr_light_le_device
    assert B(None, p, p, p, None, 1, 31, p, None) == ERR_INVALID
    assert B(dummy, None, p, p, None, 4, 31, p, None) == ERR_INVALID
    assert B(dummy, p, None, p, None, 4, 31, p, None) == ERR_INVALID
    assert B(dummy, p, p, None, None, 4, 31, p, None) == ERR_INVALID
    assert B(dummy, p, p, p, None, 4, 31, None, None) == ERR_INVALID
    assert B(dummy, p, p, p, None, -1, 31, p, None) == ERR_INVALID
    assert B(dummy, p, p, p, None, 4, 32, p, None) == ERR_INVALID
    assert B(dummy, p, p, p, None, 4, -1, p, None) == ERR_INVALID
    assert B(dummy, odd, p, p, None, 2, 31, p, None) == ERR_INVALID
    assert B(dummy, p, p, p, None, 2, 31, odd, None) == ERR_INVALID
    assert "aligned" in L.gnxr_last_error().decode()
    assert B(dummy, None, None, None, None, 0, 31, None, None) == 0
    assert S(None, p, 1, 0, p, None) == ERR_INVALID
    assert S(dummy, None, 4, 0, p, None) == ERR_INVALID
    assert S(dummy, p, 4, 0, None, None) == ERR_INVALID
    assert S(dummy, p, -1, 0, p, None) == ERR_INVALID
    assert S(dummy, p, 4, 3, p, None) == ERR_INVALID
    assert S(dummy, odd, 2, 0, p, None) == ERR_INVALID
    assert S(dummy, None, 0, 0, None, None) == 0
    assert E(None, 0, p, 1, p, None) == ERR_INVALID
    assert E(dummy, 0, None, 4, p, None) == ERR_INVALID
    assert E(dummy, 0, p, 4, None, None) == ERR_INVALID
    assert E(dummy, 0, p, -1, p, None) == ERR_INVALID
    if not torch.cuda.is_available():
        # host memory that passes every argument check: the next question needs the runtime
        assert B(dummy, p, p, p, None, 2, 31, p, None) == ERR_NO_DEVICE
        assert S(dummy, p, 2, 0, p, None) == ERR_NO_DEVICE
        assert "no HIP device" in L.gnxr_last_error().decode()


def test_python_layer_refuses_other_tensors_naming_the_argument(gx):
    """Only contiguous float32 tensors of the documented shapes on the scene's device are accepted; anything else raises ValueError that
    names the argument, before a library call (the handle here is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    f = torch.zeros
    good = {"rays": f((4, 8)), "wi": f((4, 3)), "u": f((4, 2))}
    bad = {"rays": [np.zeros((4, 8), np.float32), f((4, 8), dtype=torch.float64), f((4, 7)), f((8, 4)).t(), f((4, 16))[:, ::2], f(32)],
           "wi": [f((4, 3), dtype=torch.float16), f((4, 4)), f((3, 4)).t(), f(12)],
           "u": [f((4, 2), dtype=torch.int32), f((4, 3)), f((4, 4))[:, ::2]]}
    for name, cases in bad.items():
        for b in cases:
            with pytest.raises(ValueError, match=f"bsdf: {name}"):
                s.bsdf(**{**good, name: b})
    with pytest.raises(ValueError, match="bsdf: differentials"):
        s.bsdf(**good, differentials=f((4, 6)))
    with pytest.raises(ValueError, match="bsdf: rays"):      # a CPU tensor of the right layout is on the wrong device
        s.bsdf(**good)
    with pytest.raises(ValueError, match="flags"):
        s.bsdf(**good, flags=64)
    lg = {"p": f((4, 3)), "n": f((4, 3)), "u": f((4, 2)), "wi_query": f((4, 3))}
    for name in lg:
        for b in (f((4, 5)), f((4, lg[name].shape[1]), dtype=torch.float64), np.zeros((4, 3), np.float32)):
            with pytest.raises(ValueError, match=f"sample_light: {name}"):
                s.sample_light(0, **{**lg, name: b})
    with pytest.raises(ValueError, match="sample_light: p"):
        s.sample_light(0, **lg)
    for bad_strategy in ("importance", 3, -1, True):
        with pytest.raises(ValueError, match="sample_light: strategy"):
            s.sample_light(0, **lg, strategy=bad_strategy)
    with pytest.raises(ValueError, match="light_le: rays"):
        s.light_le(0, f((4, 7)))
    with pytest.raises(ValueError, match="light_le: rays"):
        s.light_le(0, f((4, 8)))
    if torch.cuda.is_available():
        c = {k: v.cuda() for k, v in good.items()}
        with pytest.raises(ValueError, match="bsdf: wi has 3 rows"):
            s.bsdf(c["rays"], c["wi"][:3].contiguous(), c["u"])
        with pytest.raises(ValueError, match="bsdf: out"):
            s.bsdf(**c, out=torch.zeros((4, 12), device="cuda"))
        with pytest.raises(ValueError, match="sample_light: light"):
            s.sample_light(torch.zeros(4, dtype=torch.int64, device="cuda"), **{k: v.cuda() for k, v in lg.items()})


def test_chosen_seeds_give_enough_valid_probes():
    """The oracle alone, on the CPU: every probe set the GPU tests below use has at least a quarter of valid hits (so that an all-zero
    device result cannot pass), and the env / sky fixtures compare P1 on a known share of their records."""
    for name, b, seed in oracle_cases():
        rays, wi, u = probes(4096, seed)
        o = ol.OracleScene(b).bsdf_probe(rays, wi, u, 31)
        frac = float((o[:, 13] == 1).mean())
        print(f"{name}: valid fraction {frac:.3f}")
        assert frac >= 0.25, (name, frac)
    g = golden("light_env.npz")
    for nm in ("sky", "env"):
        frac = float((g[nm][:, 3] > 0).mean())
        print(f"light_env.npz {nm}: pdf > 0 on {frac:.4f} of {len(g[nm])} records")
        assert frac > 0


def oracle_cases():
    return [("glass_sphere", scenes.cornell_sphere("glass"), 31), ("textured", scenes.textured_cornell(TEX, uv_quads=True), 32),
            ("smooth", scenes.smooth_cornell(TEX), 33)]


# ---------------------------------------------------------------- GPU: the reference's goldens, directly
@pytest.mark.gpu
def test_bsdf_reference_goldens(gpu):
    g = golden("bsdf_zoo.npz")
    scene = gpu.Scene(scenes.material_zoo())
    assert len(g["rays"]) == 8192
    for flags in (31, 15):
        o = dbsdf(scene, g["rays"], g["wi"], g["u"], flags)
        assert o.shape == (8192, 16)
        assert biteq(o, g[f"out_{flags}"]), (flags, mismatch(o, g[f"out_{flags}"]))
    assert (g["out_31"][:, 13] == 1).sum() > 4000


@pytest.mark.gpu
def test_area_light_reference_goldens(gpu):
    g = golden("light_area.npz")
    scene = gpu.Scene(scenes.cornell())
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]   # column 8 of the fixture was recorded under another selection strategy
    for li in (0, 1):
        o = dlight(scene, li, g["refP"], g["refN"], g["u"], g["wiQ"], gpu._abi.LIGHTS_UNIFORM)
        r = g[f"light{li}"]
        assert biteq(o[:, keep], r[:, keep]), (li, mismatch(o[:, keep], r[:, keep]))
        assert (r[:, 3] > 0).mean() > 0.25
    pts = g["pts"]
    for li in (0, 1):
        o = dlight(scene, li, pts, pts * 0, pts[:, :2] * 0 + 0.5, pts, gpu._abi.LIGHTS_SPATIAL)
        assert biteq(o[:, 8], g["spatial_pdf"][:, li]), (li, mismatch(o[:, 8:9], g["spatial_pdf"][:, li:li + 1]))


@pytest.mark.gpu
def test_env_and_skybox_reference_goldens(gpu):
    g = golden("light_env.npz")
    scene = gpu.Scene(env_scene())
    for li, nm in ((2, "sky"), (3, "env")):
        o = dlight(scene, li, g["refP"], g["refN"], g["u"], g["wiQ"], gpu._abi.LIGHTS_UNIFORM)
        r = g[nm]
        assert biteq(o[:, :8], r[:, :8]), (nm, mismatch(o[:, :8], r[:, :8]))
        pdf_pos = r[:, 3] > 0                      # the reference leaves P1 unset otherwise
        fixture_fraction = float(pdf_pos.mean())   # the share of the fixture that carries a P1: all of it is compared
        print(f"{nm}: P1 compared on {fixture_fraction:.4f} of {len(r)} records")
        got_p1, want_p1 = o[pdf_pos, 9:], r[pdf_pos, 9:]                   # what is handed to the comparison
        assert got_p1.shape == want_p1.shape and len(got_p1) / len(r) >= fixture_fraction > 0
        assert biteq(got_p1, want_p1), (nm, mismatch(got_p1, want_p1))
        rays = g[nm + "_rays"]
        assert len(rays) == 4096
        le = scene.light_le(li, dev(rays))
        torch.cuda.synchronize()
        assert biteq(le.cpu().numpy(), g[nm + "_le"]), (nm, mismatch(le.cpu().numpy(), g[nm + "_le"]))
    # lights without Le
    le = scene.light_le(0, dev(g["sky_rays"]))
    torch.cuda.synchronize()
    assert (le.cpu().numpy() == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", scenes.MATERIAL_GRID_FLAGS)
def test_bsdf_material_grid_goldens(gpu, flags):
    """The materials' parameter space (scenes.MATERIAL_GRID: every branch of compile_material) under aimed probes -- grazing incidence, wi
    on the mirror and the refraction axis, the edges of u --, whole records against the compiled reference.  The reference's NaN records
    (rough transmission at eta == 1) must come back as NaN.  tests/test_material_grid.py states what the fixture must show."""
    g = scenes.material_grid_golden()
    want = g[f"out_{flags}"]
    got = dbsdf(gpu.Scene(scenes.material_grid()), g["rays"], g["wi"], g["u"], flags)
    assert got.shape == want.shape == (len(scenes.MATERIAL_GRID) * scenes.MATERIAL_GRID_PROBES, 16) and (want[:, 13] == 1).all()
    bad = {}
    for i, name in enumerate(scenes.MATERIAL_GRID_NAMES):
        s = g["material"] == i
        if not biteq(got[s], want[s]):
            bad[name] = mismatch(got[s], want[s])
    assert not bad, (flags, bad)


@pytest.mark.gpu
def test_delta_light_grid_goldens(gpu):
    """Point, spot and distant lights across cone shapes and transforms (scenes.DELTA_GRID), reference points on the cone edges and on the
    light itself, under the uniform strategy.  Column 8 (the selection pdf) is not produced by the reference; P1 (columns 9 to 11) is
    compared where the reference's pdf is > 0, as for the environment lights."""
    g = golden("light_delta.npz")
    b, first = scenes.delta_grid()
    scene = gpu.Scene(b)
    assert int(g["first_light"]) == first and len(g["out"]) == len(scenes.DELTA_GRID)
    bad = {}
    for k, l in enumerate(scenes.DELTA_GRID):
        r = g["out"][k]
        o = dlight(scene, first + k, g["refP"][k], g["refN"], g["u"], g["wiQ"], gpu._abi.LIGHTS_UNIFORM)
        pdf_pos = r[:, 3] > 0
        assert o.shape == r.shape and pdf_pos.mean() > 0.9
        if not biteq(o[:, :8], r[:, :8]):
            bad[l["name"]] = mismatch(o[:, :8], r[:, :8])
        elif not biteq(o[pdf_pos, 9:], r[pdf_pos, 9:]):
            bad[l["name"]] = "P1: " + mismatch(o[pdf_pos, 9:], r[pdf_pos, 9:])
    assert not bad, bad


# ---------------------------------------------------------------- GPU: against the oracle, where no golden exists
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["glass_sphere", "textured", "smooth"])
@pytest.mark.parametrize("flags", [31, 15, REFLECTION_ONLY, SPECULAR_ONLY])
def test_bsdf_against_oracle(gpu, case, flags):
    name, b, seed = next(c for c in oracle_cases() if c[0] == case)
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    rays, wi, u = probes(4096, seed)
    want = osc.bsdf_probe(rays, wi, u, flags)
    got = dbsdf(scene, rays, wi, u, flags)
    assert (want[:, 13] == 1).mean() >= 0.25
    assert biteq(got, want), mismatch(got, want)
    if case == "glass_sphere":
        h = scene.Intersect(rays)
        assert (h["prim"] == scene.n_triangles).sum() > 100   # the sphere is probed


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["textured", "smooth", "glass_sphere"])
@pytest.mark.parametrize("eps_milli", [2, 40])
def test_bsdf_with_differentials_against_oracle(gpu, case, eps_milli):
    """the probe's synthetic offset rays: image textures are filtered with them (trilinear and EWA) and dudx / dvdy come back"""
    name, b, seed = next(c for c in oracle_cases() if c[0] == case)
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    rays, wi, u = probes(4096, seed + 100)
    for flags in (31, REFLECTION_ONLY):
        want = osc.bsdf_probe(rays, wi, u, flags | (eps_milli << 8))
        got = dbsdf(scene, rays, wi, u, flags, diffs=synthetic_differentials(rays, eps_milli))
        assert (want[:, 13] == 1).mean() >= 0.25
        assert (want[:, 14] != 0).mean() >= 0.25 and (want[:, 15] != 0).mean() >= 0.25   # the differentials are live
        assert biteq(got, want), (flags, mismatch(got, want))
    if case == "textured":   # and they change what the textures return
        plain = osc.bsdf_probe(rays, wi, u, 31)
        assert (plain[:, 0:3] != want[:, 0:3]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 1, 2])
def test_delta_lights_against_oracle(gpu, strategy):
    """point, spot and distant lights (and the area lights beside them) under the three selection strategies, all 12 columns"""
    b = scenes.delta_cornell()
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    d = b.desc()
    types = [d.lights[i].type for i in range(d.n_lights)]
    assert {gpu._abi.LIGHT_POINT, gpu._abi.LIGHT_SPOT, gpu._abi.LIGHT_DISTANT, gpu._abi.LIGHT_AREA_TRI} <= set(types)
    p, n, u, wq = light_probes(4096, 40 + strategy)
    per_light = {}
    for li in range(d.n_lights):
        want = osc.light_probe(li, p, n, u, wq, strategy=strategy)
        got = dlight(scene, li, p, n, u, wq, strategy)
        assert (want[:, 3] > 0).mean() >= 0.25 and (want[:, 8] > 0).mean() >= 0.25, li
        assert biteq(got, want), (li, types[li], mismatch(got, want))
        per_light[li] = want
    # one light per query
    lights = (np.arange(4096) % d.n_lights).astype(np.int32)
    got = scene.sample_light(dev(lights, np.int32), dev(p), dev(n), dev(u), dev(wq), strategy=strategy)
    torch.cuda.synchronize()
    want = np.stack([per_light[int(l)][i] for i, l in enumerate(lights)])
    assert biteq(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_light_index_out_of_range(gpu):
    scene = gpu.Scene(scenes.cornell())
    p, n, u, wq = light_probes(1000, 7)
    lights = np.zeros(1000, np.int32)
    lights[[417, 800]] = [2, -1]
    out = torch.full((1000, 12), 7.0, device="cuda")
    with pytest.raises(gpu.GnxrError, match="query 417"):
        scene.sample_light(dev(lights, np.int32), dev(p), dev(n), dev(u), dev(wq), strategy="uniform", out=out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[[417, 800]] == 0).all()
    lights[[417, 800]] = 0
    assert biteq(np.delete(o, [417, 800], 0), np.delete(dlight(scene, 0, p, n, u, wq, 1), [417, 800], 0))
    with pytest.raises(gpu.GnxrError):
        scene.light_le(2, dev(scenes.random_rays(8, seed=1)))


# ---------------------------------------------------------------- GPU: consistency with what already ships
@pytest.mark.gpu
def test_valid_agrees_with_intersect(gpu):
    g = golden("bsdf_zoo.npz")
    seen_null = seen_miss = False
    for b, rays, wi, u in ((scenes.material_zoo(), g["rays"], g["wi"], g["u"]), (scenes.delta_cornell(),) + probes(8192, 51, tmax=1.5),
                           (scenes.cornell_in_fog(),) + probes(8192, 52)):
        scene = gpu.Scene(b)
        o = dbsdf(scene, rays, wi, u)
        hits = scene.intersect(dev(rays))
        torch.cuda.synchronize()
        prim = hits.prim.cpu().numpy()
        d = b.desc()
        mats = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
        null = np.zeros(len(prim), bool)
        tri = (prim >= 0) & (prim < d.n_triangles)
        null[tri] = mats[prim[tri]] < 0
        assert ((o[:, 13] == 0) == ((prim == -1) | null)).all()
        assert (o[o[:, 13] == 0] == 0).all()
        seen_null, seen_miss = seen_null or null.any(), seen_miss or (prim == -1).any()
    assert seen_null and seen_miss   # null-material triangles (the medium ball, the fog box) and rays cut short by tmax both occur


@pytest.mark.gpu
def test_independent_of_batch_size_and_position(gpu):
    g = golden("bsdf_zoo.npz")
    scene = gpu.Scene(scenes.material_zoo())
    rays, wi, u = g["rays"], g["wi"], g["u"]
    whole = dbsdf(scene, rays, wi, u)
    perm = np.random.default_rng(5).permutation(len(rays))
    drays, dwi, du = dev(rays[perm]), dev(wi[perm]), dev(u[perm])
    for bs in (1, 63, 64, 65, 8192):
        out = torch.empty((len(rays), 16), device="cuda")
        for s in range(0, len(rays), bs):
            e = min(s + bs, len(rays))
            scene.bsdf(drays[s:e], dwi[s:e], du[s:e], out=out[s:e])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert biteq(o, whole[perm]), (bs, mismatch(o, whole[perm]))


@pytest.mark.gpu
def test_two_streams_alongside_a_render(gpu):
    """Two BSDF calls on two streams, queued while a gnxr_render_device of the same handle is in flight.  gnxr_render_device returns
    only when its image is written, so the render runs on a second thread (ctypes releases the GIL around the call) and is large enough
    to outlast the two submissions; that it was still inside the call when both queries had been queued is asserted."""
    import threading
    import time
    b = scenes.delta_cornell()
    scene = gpu.Scene(b)
    integ, (W, H, spp) = gpu.PathIntegrator(5, 1.0, "spatial"), (1280, 720, 128)
    alone, _ = integ.Render(scene, W, H, spp)
    ra, rb = probes(1 << 18, 61), probes(1 << 17, 62)
    quiet_a, quiet_b = dbsdf(scene, *ra), dbsdf(scene, *rb, flags=15)
    da, db = [dev(x) for x in ra], [dev(x) for x in rb]
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rs, sa, sb = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for s in (rs, sa, sb):
        s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    entered, failure = threading.Event(), []

    def render():
        try:
            entered.set()
            integ.RenderDevice(scene, img.data_ptr(), W, H, spp, stream=rs.cuda_stream)
        except Exception as e:   # noqa: BLE001  (reported by the main thread)
            failure.append(e)

    t = threading.Thread(target=render)
    t.start()
    assert entered.wait(10)
    time.sleep(0.01)             # the render thread is inside gnxr_render_device and has queued its first launches
    oa = scene.bsdf(*da, stream=sa)
    ob = scene.bsdf(*db, flags=15, stream=sb)
    in_flight_when_queued = t.is_alive()
    sa.synchronize(); sb.synchronize()
    in_flight_when_done = t.is_alive()
    t.join(120)
    assert not t.is_alive() and not failure, failure
    torch.cuda.synchronize()
    print(f"render in flight when the queries were queued: {in_flight_when_queued}, when they had finished: {in_flight_when_done}")
    assert in_flight_when_queued, "the render returned before both queries were queued: nothing overlapped"
    assert biteq(img.cpu().numpy()[..., :3], alone[..., :3]) and alone[..., :3].any()
    assert biteq(oa.cpu().numpy(), quiet_a) and biteq(ob.cpu().numpy(), quiet_b)
    assert (quiet_a[:, 13] == 1).mean() >= 0.25


@pytest.mark.gpu
def test_binary_fallback_and_pointer_checks(gpu):
    """a scene on the reference's binary walk gives the same records; host memory is refused before anything is queued"""
    b = scenes.material_zoo()
    g = golden("bsdf_zoo.npz")
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(b)
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    assert biteq(dbsdf(scene, g["rays"], g["wi"], g["u"]), g["out_31"])
    L = gpu.lib()
    rays, wi, u = dev(g["rays"]), dev(g["wi"]), dev(g["u"])
    out = torch.zeros((8192, 16), device="cuda")
    host = np.ascontiguousarray(g["wi"])
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert L.gnxr_bsdf_device(scene._h, vp(rays), C.c_void_p(host.ctypes.data), vp(u), None, 8192, 31, vp(out), None) == ERR_INVALID
    assert "d_wi" in L.gnxr_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 0).all()
