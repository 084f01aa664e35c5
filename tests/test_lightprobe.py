"""Light probes (include/gnxr.h, "Light probes"): the numpy restatement (tests/lightprobe_reference.py) on cases worked out by hand, then
on the GPU lightprobe_rays, sh_project and sh_irradiance against it, BakeLightProbes against the composition lightprobe_rays + Li +
sh_project + the scaling, a constant sky, the orientation of the basis, live edits, the refusals and the streams.  Comparisons are on
bits unless a test says why not."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import lightprobe_reference as lr
import scenes
from conftest import GOLDEN, ROOT

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
f32 = np.float32
TEX = os.path.join(GOLDEN, "tex_smile_96x80.hdr")
NAMES = ("gnxr_lightprobe_rays_device", "gnxr_sh_project_device", "gnxr_bake_lightprobes_device", "gnxr_sh_irradiance_device")


# ---------------------------------------------------------------- CPU: the restatement on cases worked out by hand
def test_restated_butterfly_differs_from_a_sequential_sum_as_worked_out_by_hand():
    """2^24, 1, 1, ...: added one after another every 1 is lost (2^24 + 1 rounds back to 2^24).  In the butterfly only lane 0's first
    step loses one: lane 0 goes 2^24 + 1 -> 2^24, then + 2, + 4, + 8, + 16, + 32, all exact (the spacing up there is 2)."""
    v = np.ones(64, f32)
    v[0] = f32(2.0 ** 24)
    seq = f32(0)
    for t in v:
        seq = f32(seq + t)
    assert seq == f32(2.0 ** 24)
    assert lr.butterfly(v) == f32(2.0 ** 24 + 62) and lr.butterfly(v) != seq
    # the large term in another lane: lane 37 pairs with lane 5 at m = 32, the same loss, the same sum -- every lane ends with the same bits
    w = np.ones(64, f32)
    w[37] = f32(2.0 ** 24)
    assert lr.butterfly(w) == f32(2.0 ** 24 + 62)
    # through project(): direction +z, slot 2 is 0.488603f * 1, channel r carries the terms
    d = np.tile(np.array([0, 0, 1], f32), (64, 1))
    L = np.zeros((64, 4), f32)
    L[:, 0] = v
    y2 = f32(0.488603)
    got = lr.project(d, L, 1)
    assert got.shape == (1, 9, 4) and got[0, 2, 0] == lr.butterfly((v * y2).astype(f32)) and (got[0, :, 3] == 0).all() and (got[0, 2, 1:] == 0).all()


def test_restated_partial_blocks_of_1_and_63_samples_and_the_order_of_blocks():
    t = f32(0.282095)                                   # the term of L = 1 in slot 0
    d = np.tile(np.array([1, 0, 0], f32), (130, 1))
    L = np.ones((130, 4), f32)
    assert lr.project(d[:1], L[:1], 1)[0, 0, 0] == t    # t + 0 six times over
    # 63 terms and a +0 in lane 63: the lanes that pair with it fall one term short, step by step
    t2 = t + t; t3 = t2 + t; t4 = t2 + t2; t7 = t4 + t3; t8 = t4 + t4; t15 = t8 + t7; t16 = t8 + t8; t31 = t16 + t15; t32 = t16 + t16
    want63 = t32 + t31                                  # lane 0 at m = 1: its own 32 t plus lane 1's 31 t
    assert lr.project(d[:63], L[:63], 1)[0, 0, 0] == want63
    t64 = t32 + t32
    # 130 samples: two whole blocks and one of two terms (lanes 0 and 1 meet at m = 1), added to 0 in block order
    want130 = ((f32(0) + t64) + t64) + t2
    assert lr.project(d, L, 1)[0, 0, 0] == want130
    # continuing from the sums of the first 64 gives the same bits; probes do not mix
    first = lr.project(d[:64], L[:64], 1)
    assert lr.biteq(lr.project(d[64:], L[64:], 1, start=first), lr.project(d, L, 1))
    two = lr.project(np.concatenate([d[:63], d[:63]]), np.concatenate([L[:63], L[:63] * f32(2)]), 2)
    assert two[0, 0, 0] == want63 and two[1, 0, 0] == f32(2) * want63
    assert lr.bake_scale(two, 63)[0, 0, 0] == (want63 * f32(12.566370614359172)) / f32(63)


def test_restated_irradiance_of_a_probe_that_holds_only_c0():
    sh = np.zeros((2, 9, 4), f32)
    sh[1, 0, :3] = (0.5, 2.0, 3.0)
    n = np.array([[0, 1, 0], [0.6, 0, -0.8], [0, 0, 1]], f32)
    E, valid = lr.irradiance(sh, np.array([1, 1, 5]), n)
    want = f32(3.14159265) * (np.array([0.5, 2.0, 3.0], f32) * f32(0.282095))
    assert valid.tolist() == [True, True, False]
    assert lr.biteq(E[0], [*want, 1]) and lr.biteq(E[1], [*want, 1]) and (E[2] == 0).all()
    # band 1 alone: E = A1 * (c * 0.488603 * n.y) on top of a zero band 0
    sh[0, 1, :3] = 1
    E, _ = lr.irradiance(sh, np.array([0, 0]), np.array([[0, 1, 0], [0, -1, 0]], f32))
    a = f32(2.09439510) * (f32(1) * (f32(0.488603) * f32(1)))
    assert E[0, 0] == a and E[1, 0] == -a


def test_lightprobe_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(gx.lib(), name) and name in gx._abi.PROTOTYPES, name
    assert re.search(r"struct gnxr_lightprobe_params \{ int32_t struct_size; uint32_t flags; int32_t medium; \}", hdr)
    assert C.sizeof(gx._abi.LightprobeParams) == 12 and [f[0] for f in gx._abi.LightprobeParams._fields_] == ["struct_size", "flags", "medium"]
    assert gx.lib().gnxr_abi_version() == 5 and gx.lib().gnxr_abi_sizeof(14) == -1
    assert gx._abi.SH_CONTINUE == 1 and re.search(r"#define GNXR_SH_CONTINUE 1u", hdr)
    for cls in (gx.PathIntegrator, gx.VolPathIntegrator, gx.WhittedIntegrator, gx.DirectLightingIntegrator):
        assert cls.BakeLightProbes is gx.PathIntegrator.BakeLightProbes
    for name in ("lightprobe_rays", "sh_project", "sh_irradiance"):
        assert callable(getattr(gx, name))


def test_lightprobe_calls_refuse_malformed_arguments_before_any_device(gx):
    lib = gx.lib()
    vp = C.c_void_p
    err = lambda: lib.gnxr_last_error()
    # probe rays
    assert lib.gnxr_lightprobe_rays_device(None, 8, 8, None, None, None, None, 0, -1, None, None, None) == ERR_INVALID and b"null" in err()
    assert lib.gnxr_lightprobe_rays_device(None, 8, 8, vp(16), vp(16), vp(16), vp(16), -1, -1, vp(16), vp(16), None) == ERR_INVALID and b"n = -1" in err()
    assert lib.gnxr_lightprobe_rays_device(None, 0, 8, vp(16), vp(16), vp(16), vp(16), 1, -1, vp(16), vp(16), None) == ERR_INVALID and b"0 x 8" in err()
    assert lib.gnxr_lightprobe_rays_device(None, 8, 8, vp(16), vp(16), vp(16), vp(16), 1, -2, vp(16), vp(16), None) == ERR_INVALID and b"medium" in err()
    assert lib.gnxr_lightprobe_rays_device(None, 8, 8, vp(16), vp(16), vp(16), vp(16), 1, -1, vp(24), vp(16), None) == ERR_INVALID and b"aligned" in err()
    assert lib.gnxr_lightprobe_rays_device(None, 8, 8, vp(18), vp(16), vp(16), vp(16), 1, -1, vp(16), vp(16), None) == ERR_INVALID and b"aligned" in err()
    # projection
    assert lib.gnxr_sh_project_device(None, None, 1, 1, None, 0, None) == ERR_INVALID and b"null" in err()
    assert lib.gnxr_sh_project_device(vp(16), vp(16), -1, 1, vp(16), 0, None) == ERR_INVALID
    assert lib.gnxr_sh_project_device(vp(16), vp(16), 1, -1, vp(16), 0, None) == ERR_INVALID
    assert lib.gnxr_sh_project_device(vp(16), vp(16), 1, 1, vp(16), 2, None) == ERR_INVALID and b"flag" in err()
    assert lib.gnxr_sh_project_device(vp(16), vp(24), 1, 1, vp(16), 0, None) == ERR_INVALID and b"aligned" in err()
    assert lib.gnxr_sh_project_device(vp(16), vp(16), 1, 1, vp(20), 1, None) == ERR_INVALID and b"aligned" in err()
    # evaluation
    assert lib.gnxr_sh_irradiance_device(None, 1, None, None, 1, None, None) == ERR_INVALID and b"null" in err()
    assert lib.gnxr_sh_irradiance_device(vp(16), -1, vp(16), vp(16), 1, vp(16), None) == ERR_INVALID
    assert lib.gnxr_sh_irradiance_device(vp(16), 1, vp(16), vp(16), -1, vp(16), None) == ERR_INVALID
    assert lib.gnxr_sh_irradiance_device(vp(24), 1, vp(16), vp(16), 1, vp(16), None) == ERR_INVALID and b"aligned" in err()
    assert lib.gnxr_sh_irradiance_device(vp(16), 1, vp(18), vp(16), 1, vp(16), None) == ERR_INVALID and b"aligned" in err()
    # the bake
    p = gx.PathIntegrator(5, 1.0, "spatial").params(3, 2, 4)
    pp = lambda size=12, flags=0, medium=-1: gx._abi.LightprobeParams(size, flags, medium)

    def bake(params=p, probe=None, pos=16, n=5, out=16):
        return lib.gnxr_bake_lightprobes_device(None, C.byref(params), C.byref(probe or pp()), vp(pos), n, vp(out), None, None)

    assert lib.gnxr_bake_lightprobes_device(None, None, None, None, 0, None, None, None) == ERR_INVALID and b"null" in err()
    assert bake(probe=pp(size=16)) == ERR_INVALID and b"struct_size" in err()
    assert bake(probe=pp(flags=1)) == ERR_INVALID and b"flag" in err()
    assert bake(probe=pp(medium=-2)) == ERR_INVALID and b"medium" in err()
    assert bake(n=-1) == ERR_INVALID and b"n_probes" in err()
    assert bake(n=7) == ERR_INVALID and b"does not hold 7 probes" in err()
    assert bake(out=24) == ERR_INVALID and b"aligned" in err()
    assert bake(pos=18) == ERR_INVALID and b"aligned" in err()
    assert bake(params=gx.PathIntegrator(5, 1.0, "spatial").params(3, 2, 4, spp_begin=1, spp_end=2)) == ERR_INVALID and b"spp_begin" in err()
    assert bake(params=gx.PathIntegrator(5, 1.0, "spatial").params(3, 2, 4, shard_index=1, shard_count=2)) == ERR_INVALID and b"shard" in err()
    assert bake() == ERR_INVALID and b"null" in err()      # everything well-formed but the scene


# ---------------------------------------------------------------- GPU helpers
DEV = "cuda:0"
W3, H2 = 3, 2


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def gx_mod():
    import gnxraytracer_amd
    return gnxraytracer_amd


def sincos(gx):
    return lambda theta: (gx.eval_libm("sincos.sin", theta), gx.eval_libm("sincos.cos", theta))


def halton_pair(gx, W, H, px, py, s):
    n = len(px)
    return np.stack([gx.sample_halton(W, H, px, py, s, np.full(n, 3, np.int32)), gx.sample_halton(W, H, px, py, s, np.full(n, 4, np.int32))], axis=1)


def sky_builder():
    """a constant environment of radiance 1 (the bake tests' map of ones) around a millimetre-sized quad 100 units below the origin: a probe
    near the origin is in the open"""
    gx = gx_mod()
    b = gx.SceneBuilder()
    white = b.MatteMaterial(scenes.WHITE, 0.0)
    v = np.array([[-1, 0, 1], [1, 0, -1], [-1, 0, -1], [1, 0, -1], [-1, 0, 1], [1, 0, 1]], f32) * f32(1e-3) + np.array([0, -100, 0], f32)
    b.add_mesh(v, np.arange(6, dtype=np.int32).reshape(2, 3), white)
    b.AddInfLightData(np.ones((8, 16, 3), f32))
    return b


# the winding of AddAreaLight's quad: Normalize(Cross(p0 - p2, p1 - p2)) = -y, the side a one-sided area light emits to
LIGHT_QUAD = np.array([[-1, 1, 1], [-1, 1, -1], [1, 1, 1], [1, 1, 1], [-1, 1, -1], [1, 1, -1]], f32)
LIGHT_QUAD_BELOW = LIGHT_QUAD * np.array([-1, -1, 1], f32)     # half a turn about z: at y = -1, facing up


def light_quad_builder(v):
    """one emissive 2 x 2 quad of radiance 3 and nothing else: from the origin it fills a face of the cube, a sixth of the sphere"""
    gx = gx_mod()
    b = gx.SceneBuilder()
    b.add_emissive_mesh(v, np.arange(6, dtype=np.int32).reshape(2, 3), b.MatteMaterial(scenes.WHITE, 0.0), (3.0, 3.0, 3.0), 1)
    return b


def luminance(rgb):
    return 0.212671 * rgb[..., 0] + 0.715160 * rgb[..., 1] + 0.072169 * rgb[..., 2]


def compose(gx, integ, scene, pos, spp, W, H, medium=-1):
    """the bake, spelled out through the layered calls: (coefficients [n, 9, 4] as the bake defines them, rays, L), probe-major"""
    n = len(pos)
    k = np.repeat(np.arange(n, dtype=np.int32), spp)
    s = np.tile(np.arange(spp, dtype=np.int32), n)
    rays, samples = gx.lightprobe_rays(scene, dev(np.repeat(pos, spp, axis=0)), dev(k % W), dev(k // W), dev(s), W, H, medium=medium)
    L, _ = integ.Li(scene, rays, samples, W, H, spp)
    sums = gx.sh_project(rays, L, n)
    sh = (sums * torch.tensor(lr.FOUR_PI, device=DEV)) / torch.tensor(f32(spp), device=DEV)
    return sh.cpu().numpy(), rays, L


# ---------------------------------------------------------------- GPU 1: probe rays
def pole_candidates(W, H):
    """Sample numbers that can reach the pole z = 1, which takes u0 <= 2^-26.  Dimension 3 is the scrambled radical inverse in base 7: it is
    that small when the ten lowest base-7 digits of the Halton index are all the digit `a` the permutation sends to 0 (the digits above
    weigh less than 7^-10), so index = a * (7^10 - 1) / 6 + m * 7^10.  Such indices lie far beyond the first few thousand -- among
    samples 0 .. 8191 of these pixels the smallest u0 is 4e-6.  A pixel's indices are offset + s * stride with offset < stride; 7^10 = 1
    modulo the stride (a power of 2 times a power of 3, here 12), so some m < stride fits every pixel.  Neither `a` nor the offsets are
    known here: all of them are tried, and the caller keeps what reaches the pole."""
    stride = 1
    while stride < min(W, 128):
        stride *= 2
    sy = 1
    while sy < min(H, 128):
        sy *= 3
    stride *= sy
    assert (7 ** 10) % stride == 1
    cand = []
    for a in range(7):
        for m in range(stride):
            X = a * ((7 ** 10 - 1) // 6) + m * 7 ** 10
            for o in range(stride):
                if (X - o) % stride == 0 and X - o >= 0 and X < 2 ** 32:
                    cand.append((X - o) // stride)
    return np.unique(np.array(cand, np.int64)).astype(np.int32)


def ray_records(gx, n=300, seed=11):
    """n records over the 3 x 2 grid, among them samples whose u0 (Halton dimension 3) is so small that z = 1 - 2 u0 is 1 and
    1 - z*z is 0: r = 0 and the direction is the pole itself; and the smallest and largest u0 among the first 8192 samples of every pixel"""
    rng = np.random.default_rng(seed)
    px, py = rng.integers(0, W3, n).astype(np.int32), rng.integers(0, H2, n).astype(np.int32)
    s = rng.integers(0, 4096, n).astype(np.int32)
    cand_s = np.concatenate([np.arange(8192, dtype=np.int32), pole_candidates(W3, H2)])
    poles = []
    for x in range(W3):
        for y in range(H2):
            m = len(cand_s)
            u0 = gx.sample_halton(W3, H2, np.full(m, x, np.int32), np.full(m, y, np.int32), cand_s, np.full(m, 3, np.int32))
            z = f32(1) - f32(2) * u0
            for k in np.nonzero((f32(1) - z * z) <= 0)[0][:4]:
                poles.append((x, y, int(cand_s[k])))
            order = np.argsort(u0[:8192])
            for k in (*order[:2], *order[-2:]):
                poles.append((x, y, int(k)))
    assert len(poles) <= n
    for i, (x, y, k) in enumerate(poles):
        px[i], py[i], s[i] = x, y, k
    pos = rng.uniform(-2, 2, (n, 3)).astype(f32)
    return pos, px, py, s, len(poles)


@pytest.mark.gpu
def test_lightprobe_rays_equal_the_restatement(gpu):
    gx = gpu
    scene = gx.Scene(scenes.cornell())
    pos, px, py, s, n_poles = ray_records(gx)
    u = halton_pair(gx, W3, H2, px, py, s)
    want_rays, want_samples, valid = lr.probe_rays(pos, px, py, s, u, W3, H2, -1, sincos(gx))
    rays, samples = gx.lightprobe_rays(scene, dev(pos), dev(px), dev(py), dev(s), W3, H2)
    rays, samples = rays.cpu().numpy(), samples.cpu().numpy()
    assert valid.all() and rays.shape == (300, 8) and samples.shape == (300, 4)
    assert lr.biteq(rays, want_rays), np.argwhere(rays.view(np.uint32) != want_rays.view(np.uint32))[:4]
    assert (samples == want_samples).all()
    z = f32(1) - f32(2) * u[:, 0]
    at_pole = (f32(1) - z * z) <= 0
    print("records at the pole:", int(at_pole.sum()), "of", n_poles, "planted; smallest u0", u[:, 0].min())
    assert at_pole.sum() >= W3 * H2                      # every pixel has one
    assert (rays[at_pole, 4:6] == 0).all() and (np.abs(rays[at_pole, 6]) == 1).all()
    d = rays[:, 4:7].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6) and (rays[:, 3] == np.inf).all() and (rays[:, 7] == 0).all()


@pytest.mark.gpu
def test_lightprobe_rays_zero_a_bad_record_finish_the_others_and_raise(gpu):
    gx = gpu
    scene = gx.Scene(scenes.cornell())
    pos, px, py, s, _ = ray_records(gx, n=200)
    good = [t.cpu().numpy() for t in gx.lightprobe_rays(scene, dev(pos), dev(px), dev(py), dev(s), W3, H2)]
    for what, k in (("nan", 17), ("inf", 31), ("px", 64), ("py", 5), ("s", 130)):
        pos2, px2, py2, s2 = pos.copy(), px.copy(), py.copy(), s.copy()
        if what == "nan":
            pos2[k, 1] = np.nan
        elif what == "inf":
            pos2[k, 2] = -np.inf
        elif what == "px":
            px2[k] = W3
        elif what == "py":
            py2[k] = -1
        else:
            s2[k] = -1
        out = (torch.full((200, 8), 7.0, device=DEV), torch.full((200, 4), 7, dtype=torch.int32, device=DEV))
        with pytest.raises(gx.GnxrError, match=r"record %d\b" % k):
            gx.lightprobe_rays(scene, dev(pos2), dev(px2), dev(py2), dev(s2), W3, H2, out=out)
        for got, want in zip(out, good):
            got = got.cpu().numpy()
            keep = np.arange(200) != k
            assert (got[k] == 0).all() and (got[keep].view(np.uint32) == want[keep].view(np.uint32)).all(), what


# ---------------------------------------------------------------- GPU 2: projection
def projection_case(n_probes, n_samples, seed=5):
    """unit directions and radiance over thirty binary orders of magnitude with mixed signs: the order of the additions decides the bits"""
    rng = np.random.default_rng(seed + n_samples)
    n = n_probes * n_samples
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    L = (rng.normal(size=(n, 4)) * np.exp2(rng.integers(-15, 16, (n, 1)))).astype(f32)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:4] = rng.normal(size=(n, 4))               # origins and tmax are not read
    rays[:, 4:7] = d
    rays[:, 7] = 3
    return rays, L, d


@pytest.mark.gpu
@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 130])
def test_sh_project_equals_the_restatement(gpu, n_samples):
    gx = gpu
    rays, L, d = projection_case(5, n_samples)
    want = lr.project(d, L, 5)
    got = gx.sh_project(dev(rays), dev(L), 5).cpu().numpy()
    assert got.shape == (5, 9, 4) and lr.biteq(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    if n_samples >= 63:                                   # the order matters for this input: a plain sum gives other bits
        plain = (L[:, None, :3].astype(f32) * lr.basis(d)[:, :, None]).reshape(5, n_samples, 9, 3).sum(axis=1, dtype=f32)
        assert not lr.biteq(plain, want[..., :3])


@pytest.mark.gpu
def test_sh_project_accumulates_whole_blocks_to_the_bits_of_one_call(gpu):
    gx = gpu
    rays, L, d = projection_case(5, 128)
    r5, L5 = rays.reshape(5, 128, 8), L.reshape(5, 128, 4)
    one = gx.sh_project(dev(rays), dev(L), 5)
    acc = gx.sh_project(dev(r5[:, :64].reshape(-1, 8)), dev(L5[:, :64].reshape(-1, 4)), 5)
    half = acc.cpu().numpy()
    again = gx.sh_project(dev(r5[:, 64:].reshape(-1, 8)), dev(L5[:, 64:].reshape(-1, 4)), 5, out=acc, accumulate=True)
    assert again is acc and lr.biteq(acc.cpu().numpy(), one.cpu().numpy()) and lr.biteq(one.cpu().numpy(), lr.project(d, L, 5))
    assert lr.biteq(half, lr.project(d.reshape(5, 128, 3)[:, :64].reshape(-1, 3), L5[:, :64].reshape(-1, 4), 5)) and not lr.biteq(half, one.cpu().numpy())
    # no samples: the sums stay (accumulate) or are zero
    empty_r, empty_L = torch.zeros((0, 8), device=DEV), torch.zeros((0, 4), device=DEV)
    assert lr.biteq(gx.sh_project(empty_r, empty_L, 5, out=acc, accumulate=True).cpu().numpy(), one.cpu().numpy())
    assert (gx.sh_project(empty_r, empty_L, 5, out=acc).cpu().numpy() == 0).all()


# ---------------------------------------------------------------- GPU 3: the bake is the composition
def integrator_and_scene(gx, name):
    if name == "path":
        return gx.PathIntegrator(5, 1.0, "spatial"), scenes.cornell()
    if name == "whitted":
        return gx.WhittedIntegrator(5), scenes.cornell()
    return gx.VolPathIntegrator(5, 1.0, "spatial"), scenes.volume_cornell()


PROBES = np.array([[0, 0, 0], [-1.5, -2.0, 0.5], [1.2, 1.0, -1.0], [-0.7, 0.5, -0.4], [2.0, -0.5, 1.9]], f32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["path", "whitted", "volpath"])
def test_bake_lightprobes_equals_the_composition(gpu, name):
    gx = gpu
    integ, b = integrator_and_scene(gx, name)
    scene = gx.Scene(b)
    spp = 130
    want, _, L = compose(gx, integ, scene, PROBES, spp, W3, H2)
    assert torch.isfinite(L).all() and (L[:, :3] > 0).any()
    sh, st = integ.BakeLightProbes(scene, dev(PROBES), spp, width=W3, height=H2)
    got = sh.cpu().numpy()
    assert got.shape == (5, 9, 4) and lr.biteq(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    assert st["camera_samples"] == 5 * spp and st["rays_closest"] >= 5 * spp and (got[..., 3] == 0).all() and (got[:, 0, :3] > 0).all()
    # 100 paths per sub-batch: every probe on its own, its samples as blocks of 64, 64 and 2; 300: two probes at a time, the last one alone
    small, st_small = integ.BakeLightProbes(scene, dev(PROBES), spp, width=W3, height=H2, samples_per_pass=100)
    mid, _ = integ.BakeLightProbes(scene, dev(PROBES), spp, width=W3, height=H2, samples_per_pass=300)
    assert lr.biteq(small.cpu().numpy(), got) and lr.biteq(mid.cpu().numpy(), got) and st_small["camera_samples"] == 5 * spp


# ---------------------------------------------------------------- GPU 4: closed forms
@pytest.mark.gpu
def test_bake_lightprobes_in_the_open_under_a_constant_sky(gpu):
    """An environment map of ones: the map's bilinear lookup returns 1 or 1 - 2^-23 (test_bake.py), so Li is checked against the light's own
    Le along each ray, bit for bit, and c0 against the restatement's sums for radiance 1 and for radiance 1 - 2^-23 over the same
    directions (fp32 addition is monotonic in either argument, so every sum of radiances in between lies between the two)."""
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(sky_builder())
    pos = np.array([[0.25, 0.5, -0.125]], f32)
    spp = 130
    want, rays, L = compose(gx, integ, scene, pos, spp, W3, H2)
    le = scene.light_le(0, rays).cpu().numpy()
    L = L.cpu().numpy()
    assert lr.biteq(L[:, :3], le)                                           # every ray escaped at once
    assert (le <= 1).all() and (le >= f32(1 - 2.0 ** -22)).all() and (le == 1).mean() > 0.5
    sh, _ = integ.BakeLightProbes(scene, dev(pos), spp, width=W3, height=H2)
    got = sh.cpu().numpy()
    assert lr.biteq(got, want)
    d = rays.cpu().numpy()[:, 4:7]
    ones = np.ones((spp, 3), f32)
    hi = lr.bake_scale(lr.project(d, ones, 1), spp)[0, 0, :3]
    lo = lr.bake_scale(lr.project(d, ones * f32(1 - 2.0 ** -23), 1), spp)[0, 0, :3]
    print("c0", got[0, 0, :3], "between", lo, "and", hi)
    assert (lo <= got[0, 0, :3]).all() and (got[0, 0, :3] <= hi).all() and (lo < hi).all()
    assert abs(float(hi[0]) - 0.282095 * 4 * np.pi) < 1e-5                  # the mean of Y_0 over the sphere times 4 pi
    # a probe that holds only that c0 lights every normal alike
    only = np.zeros((1, 9, 4), f32)
    only[0, 0] = got[0, 0]
    normals = np.array([[0, 1, 0], [0, -1, 0], [0.6, 0.0, -0.8], [-0.48, 0.64, 0.6]], f32)
    probe = np.zeros(4, np.int32)
    E = gx.sh_irradiance(dev(only), dev(probe), dev(normals)).cpu().numpy()
    want_E, _ = lr.irradiance(only, probe, normals)
    assert lr.biteq(E, want_E) and np.allclose(E[:, :3], np.pi, rtol=1e-5) and (E[:, 3] == 1).all()


@pytest.mark.gpu
def test_sh_irradiance_equals_the_restatement_and_flags_a_probe_out_of_range(gpu):
    gx = gpu
    rng = np.random.default_rng(9)
    sh = np.zeros((7, 9, 4), f32)
    sh[..., :3] = rng.normal(size=(7, 9, 3)) * np.exp2(rng.integers(-6, 7, (7, 9, 1)))
    n = 333
    normals = rng.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)
    probe = rng.integers(0, 7, n).astype(np.int32)
    want, _ = lr.irradiance(sh, probe, normals)
    got = gx.sh_irradiance(dev(sh), dev(probe), dev(normals)).cpu().numpy()
    assert lr.biteq(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    for k, bad in ((40, 7), (222, -1)):
        p2 = probe.copy()
        p2[k] = bad
        out = torch.full((n, 4), 7.0, device=DEV)
        with pytest.raises(gx.GnxrError, match=r"record %d\b" % k):
            gx.sh_irradiance(dev(sh), dev(p2), dev(normals), out=out)
        out = out.cpu().numpy()
        keep = np.arange(n) != k
        assert (out[k] == 0).all() and lr.biteq(out[keep], want[keep])


# ---------------------------------------------------------------- GPU 5: orientation and live edits
ORIENT_SPP = 256


def test_orientation_spp_clears_the_margin_on_the_cpu():
    """How noisy the band-1 direction is at ORIENT_SPP, on the CPU: uniform directions (pseudo-random here, which is no better than the
    Halton points the bake uses), Li in closed form -- the light's radiance where the ray meets the quad's plane inside the quad, else 0;
    the scene holds nothing else -- and the restatement.  The worst of 200 seeds keeps the dot product with +y above 0.97."""
    worst = 1.0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        u = rng.uniform(0, 1, (ORIENT_SPP, 2)).astype(f32)
        d = lr.probe_directions(u, lambda t: (np.sin(t.astype(np.float64)).astype(f32), np.cos(t.astype(np.float64)).astype(f32)))
        with np.errstate(all="ignore"):
            hit = (d[:, 1] > 0) & (np.abs(d[:, 0] / d[:, 1]) <= 1) & (np.abs(d[:, 2] / d[:, 1]) <= 1)
        L = np.where(hit[:, None], f32(3), f32(0)) * np.ones((1, 3), f32)
        sh = lr.bake_scale(lr.project(d, L, 1), ORIENT_SPP)[0]
        v = np.array([luminance(sh[3, :3]), luminance(sh[1, :3]), luminance(sh[2, :3])], np.float64)
        worst = min(worst, v[1] / np.linalg.norm(v))
    assert worst > 0.97, worst


def band1_direction(sh):
    v = np.array([luminance(sh[3, :3]), luminance(sh[1, :3]), luminance(sh[2, :3])], np.float64)   # (c3, c1, c2) go with (x, y, z)
    return v / np.linalg.norm(v)


@pytest.mark.gpu
def test_bake_lightprobes_points_band_1_at_the_light_and_follows_a_live_edit(gpu):
    """A down-facing emissive quad centred above a probe at the origin and no other light: by symmetry (c3, c1, c2) points along +y exactly;
    0.9 leaves room for the sampling noise at 256 samples (the CPU test above measures it).  Bit-equality with our own restatement cannot
    pin which slot goes with which axis; this does.  Then the quad moves below the probe, facing up."""
    gx = gpu
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(light_quad_builder(LIGHT_QUAD))
    pos = dev(np.zeros((1, 3), f32))
    sh, _ = integ.BakeLightProbes(scene, pos, ORIENT_SPP)
    up = band1_direction(sh.cpu().numpy()[0])
    print("band 1 points along", up)
    assert up[1] > 0.9
    normals = dev(np.array([[0, 1, 0], [0, -1, 0]], f32))
    E = gx.sh_irradiance(sh, dev(np.zeros(2, np.int32)), normals).cpu().numpy()
    assert luminance(E[0, :3]) > luminance(E[1, :3]) and luminance(E[0, :3]) > 0
    # c0 = 4 pi * mean(L * Y_0): the quad fills a sixth of the sphere with radiance 3
    assert abs(sh.cpu().numpy()[0, 0, 0] / (0.282095 * 4 * np.pi * 3 / 6) - 1) < 0.25
    scene.update_vertices(LIGHT_QUAD_BELOW, move_lights=True)
    moved, _ = integ.BakeLightProbes(scene, pos, ORIENT_SPP)
    fresh, _ = integ.BakeLightProbes(gx.Scene(light_quad_builder(LIGHT_QUAD_BELOW)), pos, ORIENT_SPP)
    assert lr.biteq(moved.cpu().numpy(), fresh.cpu().numpy()) and not lr.biteq(moved.cpu().numpy(), sh.cpu().numpy())
    assert band1_direction(moved.cpu().numpy()[0])[1] < -0.9
    E = gx.sh_irradiance(moved, dev(np.zeros(2, np.int32)), normals).cpu().numpy()
    assert luminance(E[1, :3]) > luminance(E[0, :3])


# ---------------------------------------------------------------- GPU 6: errors
@pytest.mark.gpu
def test_lightprobe_refusals_leave_the_output_untouched(gpu):
    gx = gpu
    lib = gx.lib()
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    scene = gx.Scene(scenes.cornell())
    pos = dev(PROBES)
    out = torch.full((5 * 9 * 4 + 4,), 7.0, device=DEV)
    p = integ.params(W3, H2, 4)
    pp = lambda size=12, flags=0, medium=-1: gx._abi.LightprobeParams(size, flags, medium)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def bake(params=p, probe=None, pos_ptr=None, n=5, out_ptr=None, s=scene):
        return lib.gnxr_bake_lightprobes_device(s._h, C.byref(params), C.byref(probe or pp()), pos_ptr or ptr(pos), n, out_ptr or ptr(out), None, None)

    host_out, host_pos = torch.zeros(5 * 9 * 4), torch.zeros((5, 3))
    assert bake(out_ptr=ptr(host_out)) == ERR_INVALID and b"device memory" in lib.gnxr_last_error()
    assert bake(pos_ptr=ptr(host_pos)) == ERR_INVALID and b"device memory" in lib.gnxr_last_error()
    assert bake(out_ptr=ptr(out, 4)) == ERR_INVALID and b"aligned" in lib.gnxr_last_error()
    assert bake(params=integ.params(2, 2, 4)) == ERR_INVALID and b"does not hold" in lib.gnxr_last_error()
    assert bake(params=integ.params(W3, H2, 0)) == ERR_INVALID
    assert bake(params=integ.params(W3, H2, 4, spp_begin=1, spp_end=2)) == ERR_INVALID
    assert bake(probe=pp(size=16)) == ERR_INVALID and b"struct_size" in lib.gnxr_last_error()
    assert bake(probe=pp(flags=2)) == ERR_INVALID
    assert bake(probe=pp(medium=0)) == ERR_INVALID and b"medium" in lib.gnxr_last_error()
    textured = gx.Scene(scenes.textured_cornell(TEX))
    for cls in (gx.WhittedIntegrator(5), gx.DirectLightingIntegrator("all", 5), gx.VolPathIntegrator(5, 1.0, "spatial")):
        assert bake(params=cls.params(W3, H2, 4), s=textured) == ERR_UNSUPPORTED
    assert bake(n=0) == 0                                   # no probes: nothing happens
    if torch.cuda.device_count() > 1:                       # memory of a device that holds no copy of the scene
        other = torch.full((5 * 9 * 4,), 7.0, device="cuda:1")
        assert bake(out_ptr=ptr(other)) == ERR_INVALID and (other == 7).all()
    assert (out == 7).all()
    # the same through the bindings; PathIntegrator bakes the textured scene
    with pytest.raises(gx.GnxrError):
        gx.WhittedIntegrator(5).BakeLightProbes(textured, pos, 4)
    sh, _ = integ.BakeLightProbes(textured, pos, 4)
    assert torch.isfinite(sh).all() and (sh[:, 0, :3] > 0).any()
    rays, L = torch.zeros((10, 8), device=DEV), torch.zeros((10, 4), device=DEV)
    for bad in (lambda: integ.BakeLightProbes(scene, pos.cpu(), 4), lambda: integ.BakeLightProbes(scene, pos, 4, width=2, height=2),
                lambda: integ.BakeLightProbes(scene, pos[:, :2], 4), lambda: integ.BakeLightProbes(scene, pos, 4, dilate=1),
                lambda: gx.lightprobe_rays(scene, pos.cpu(), pos, pos, pos, 3, 2), lambda: gx.lightprobe_rays(scene, pos, dev(np.zeros(4, np.int32)), dev(np.zeros(5, np.int32)), dev(np.zeros(5, np.int32)), 3, 2),
                lambda: gx.sh_project(rays.cpu(), L, 5), lambda: gx.sh_project(rays, L, 3), lambda: gx.sh_project(rays, L[:5], 5), lambda: gx.sh_project(rays, L, 5, accumulate=True),
                lambda: gx.sh_irradiance(torch.zeros((2, 9, 4)), dev(np.zeros(2, np.int32)), dev(np.zeros((2, 3), f32))),
                lambda: gx.sh_irradiance(torch.zeros((2, 9, 4), device=DEV), dev(np.zeros(2, np.int32)), dev(np.zeros((3, 3), f32)))):
        with pytest.raises(ValueError):
            bad()
    # the layered calls: host memory leaves the outputs alone
    sums = torch.full((5, 9, 4), 7.0, device=DEV)
    host_rays, host_sh, two_probes, two_normals = torch.zeros((10, 8)), torch.zeros((5, 9, 4)), dev(np.zeros(2, np.int32)), dev(np.zeros((2, 3), f32))
    assert lib.gnxr_sh_project_device(ptr(host_rays), ptr(L), 5, 2, ptr(sums), 0, None) == ERR_INVALID and b"device memory" in lib.gnxr_last_error()
    E = torch.full((2, 4), 7.0, device=DEV)
    assert lib.gnxr_sh_irradiance_device(ptr(host_sh), 5, ptr(two_probes), ptr(two_normals), 2, ptr(E), None) == ERR_INVALID
    assert (sums == 7).all() and (E == 7).all()


# ---------------------------------------------------------------- GPU 7: streams
@pytest.mark.gpu
def test_sh_project_and_irradiance_on_a_side_stream_behind_the_kernels_that_fill_their_inputs(gpu):
    gx = gpu
    rays_np, L_np, d = projection_case(5, 130)
    sums0 = gx.sh_project(dev(rays_np), dev(L_np), 5)
    rng = np.random.default_rng(2)
    normals = rng.normal(size=(64, 3))
    normals = dev((normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32))
    probe = dev(rng.integers(0, 5, 64).astype(np.int32))
    E0 = gx.sh_irradiance(sums0, probe, normals)
    assert lr.biteq(sums0.cpu().numpy(), lr.project(d, L_np, 5))
    half_rays, half_L = dev(rays_np * f32(0.5)), dev(L_np * f32(0.5))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3                            # keeps the stream busy before the inputs exist
        rays_side = half_rays * 2 + big[0, 0] * 0             # exact: every value doubles back
        L_side = half_L * 2 + big[0, 0] * 0
        sums1 = gx.sh_project(rays_side.contiguous(), L_side.contiguous(), 5, stream=side)
        E1 = gx.sh_irradiance(sums1, probe, normals, stream=side)
    side.synchronize()
    assert torch.isfinite(big[0, 0])
    assert lr.biteq(sums1.cpu().numpy(), sums0.cpu().numpy()) and lr.biteq(E1.cpu().numpy(), E0.cpu().numpy())
