"""Image-texture filtering (csrc/device_texture.h: tex_evaluate, tex_lookup_width, tex_triangle, tex_ewa, tex_texel,
compute_differentials) against the compiled reference and the CPU oracle, branch by branch.

The sweep (scenes.TEXTURE_FILTER_QUADS): one flat quad per texture record -- EWA and trilinear under Repeat, Black and Clamp wrap,
max_aniso 1 / 8 / 16, a scaled and shifted mapping that makes st negative, gamma and scale -- over images of 16x16, 64x4, 5x3, 33x17 and
1x1 texels, uv running over [0, 1] or [-1.5, 2.5], probed by rays aimed at chosen uv targets (half of them within one texel of an image
border) under incidence cosines 1, 0.5, 0.1 and 0.02.  tests/golden/texture_filter.npz holds what the compiled reference returned for
these probes under its driver's synthetic offset rays at eps = 1e-5 ... 0.7 (oracle/make_goldens.py texture_filter_goldens); offset
rays that driver cannot express are compared with the oracle, which tests/test_oracle_golden.py pins to the same fixture.

Every comparison is bit for bit (NaN equal to NaN) on whole 16-column records and takes every probe of its set.  The CPU test below
counts, from the oracle's branch report, how many valid probes take each path of the lookup: the sets are built so that none is left
to chance."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes
from conftest import golden
from test_shading_queries import biteq, dbsdf, mismatch

QUADS = scenes.TEXTURE_FILTER_QUADS
KINDS = ("displaced", "x_longer", "y_longer", "x_is_main", "y_is_main", "x_parallel", "y_parallel")
ORACLE_ONLY_PER_QUAD = 126   # 18 of each kind
MIN_PROBES = 32


def quad_filter(q):
    return "trilinear" if QUADS[q]["kd"].get("trilinear") else "ewa"


def axis_aligned(q):
    return q % 5 < 3   # scenes._TF_FRAMES: the first three frames have their normal along z, x, y


@functools.lru_cache(maxsize=None)
def oracle_only_probes():
    """Probes with offset rays the reference driver cannot express, on every quad of the sweep: (rays, wi, u, diffs, kind, quad).
    displaced: offset origins away from the main origin, general offset directions; x_longer / y_longer: one offset ten to a hundred
    times the other (MIPMap::Lookup swaps the axes when dst0 is the shorter); x_is_main / y_is_main: one offset ray equal to the main
    ray, so that its uv differentials are exactly 0 and minorLength == 0 while hasDifferentials is true; x_parallel / y_parallel: one
    offset direction along an edge of an axis-aligned quad, so that Dot(n, direction) is exactly 0, tx (ty) infinite and all
    differentials zeroed (on the tilted quads, where that dot product need not vanish, these two kinds fall back to `displaced`)."""
    out = []
    for q in range(len(QUADS)):
        rays, wi, u = scenes.texture_filter_probes(q, ORACLE_ONLY_PER_QUAD, 2)
        rng = np.random.default_rng([5, q])
        n = len(rays)
        c, e1, e2, half, _ = scenes.texture_filter_quad(q)
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
        kind = np.arange(n) % len(KINDS)
        if not axis_aligned(q):
            kind[kind >= 5] = 0
        v1, v2 = rng.normal(size=(2, n, 3))
        v1 /= np.linalg.norm(v1, axis=1, keepdims=True)
        v2 /= np.linalg.norm(v2, axis=1, keepdims=True)
        size = 10.0 ** rng.uniform(-4.0, -0.5, (n, 1))
        ratio = 10.0 ** rng.uniform(1.0, 2.0, (n, 1))
        ax = np.where((kind == 2)[:, None], size / ratio, size)
        ay = np.where((kind == 1)[:, None], size / ratio, size * rng.uniform(0.5, 2.0, (n, 1)))
        rxo, ryo = o.copy(), o.copy()
        moved = kind == 0
        rxo[moved] += 0.05 * v2[moved]
        ryo[moved] -= 0.03 * v1[moved]
        rxd, ryd = d + ax * v1, d + ay * v2
        rxd[kind == 3] = d[kind == 3]
        ryd[kind == 4] = d[kind == 4]
        rxd[kind == 5] = e1
        ryd[kind == 6] = e2
        diffs = np.ascontiguousarray(np.concatenate([rxo, rxd, ryo, ryd], 1), np.float32)
        diffs[kind == 3, 0:6] = rays[kind == 3][:, [0, 1, 2, 4, 5, 6]]     # the main ray's float32 values, untouched
        diffs[kind == 4, 6:12] = rays[kind == 4][:, [0, 1, 2, 4, 5, 6]]
        out.append((rays, wi, u, diffs, kind, np.full(n, q)))
    return tuple(np.ascontiguousarray(np.concatenate([p[k] for p in out])) for k in range(6))


def sweep_oracle():
    return ol.OracleScene(scenes.texture_filter_scene("sweep"))


# ---------------------------------------------------------------- CPU: the sweep reaches what it claims
def test_sweep_reaches_every_branch():
    """The oracle alone.  Over the fixture's probes (every eps value), the oracle-only probes and the unfiltered probes of the GPU tests
    below, every path of the lookup that the oracle's branch report names is taken by at least 32 valid probes; per wrap mode the wrap
    code changes a texel index for at least 32 probes under EWA and 32 under trilinear; every image has at least 32 valid probes per
    filter; at least a quarter of every probe set is valid.  These are conditions on the inputs: the counts are printed, not tuned to."""
    g = golden("texture_filter.npz")
    osc = sweep_oracle()
    rays, wi, u, quad = g["rays"], g["wi"], g["u"], g["quad"]
    sets = []   # (name, out, mask, quad)
    for e in g["eps"]:
        out, mask = osc.bsdf_probe_diff(rays, wi, u, scenes.synthetic_differentials(rays, e), 31, branch=True)
        sets.append((f"fixture eps {float(e):g}", out, mask, quad))
    out, mask = osc.bsdf_probe_diff(rays, wi, u, None, 31, branch=True)
    sets.append(("unfiltered", out, mask, quad))
    orays, owi, ou, odiffs, okind, oquad = oracle_only_probes()
    out, mask = osc.bsdf_probe_diff(orays, owi, ou, odiffs, 31, branch=True)
    sets.append(("oracle-only", out, mask, oquad))
    for name, out, mask, _ in sets:
        frac = float((out[:, 13] == 1).mean())
        print(f"{name}: {len(out)} probes, valid fraction {frac:.3f}")
        assert frac >= 0.25, (name, frac)
        assert (mask[out[:, 13] == 0] == 0).all()
    valid = np.concatenate([s[1][:, 13] == 1 for s in sets])
    mask = np.concatenate([s[2] for s in sets])
    quad = np.concatenate([s[3] for s in sets])
    filt = np.array([quad_filter(q) for q in range(len(QUADS))])[quad]
    wrap = np.array([QUADS[q]["kd"]["wrap"] for q in range(len(QUADS))])[quad]
    image = np.array([QUADS[q]["kd"]["image"] for q in range(len(QUADS))])[quad]
    for name, bit in list(ol.TEXB.items()) + list(ol.DIFFB.items()):
        count = int((valid & ((mask & bit) != 0)).sum())
        print(f"branch {name}: {count} valid probes")
        assert count >= MIN_PROBES, (name, count)
    # the complements of the two EWA decisions: not swapped, not clamped
    ewa_lerp = valid & ((mask & ol.TEXB["ewa_lerp"]) != 0)
    for name in ("ewa_swap", "ewa_clamped", "ewa_lod0", "ewa_past"):
        count = int((ewa_lerp & ((mask & ol.TEXB[name]) == 0)).sum())
        print(f"branch not {name}: {count} valid probes")
        assert count >= MIN_PROBES, (name, count)
    for w in ("repeat", "black", "clamp"):
        for f in ("ewa", "trilinear"):
            count = int((valid & (wrap == w) & (filt == f) & ((mask & ol.TEXB["wrap"]) != 0)).sum())
            print(f"wrap {w} engaged under {f}: {count} valid probes")
            assert count >= MIN_PROBES, (w, f, count)
    for im in scenes.TEXTURE_FILTER_IMAGES:
        for f in ("ewa", "trilinear"):
            count = int((valid & (image == im) & (filt == f)).sum())
            print(f"image {im} under {f}: {count} valid probes")
            assert count >= MIN_PROBES, (im, f, count)
    # the oracle-only kinds do what their names say
    ok = sets[-1][1][:, 13] == 1
    om = sets[-1][2]
    assert ((om[ok & (okind == 5)] & ol.DIFFB["tx_fail"]) != 0).all() and ((om[ok & (okind == 6)] & ol.DIFFB["ty_fail"]) != 0).all()
    # an offset ray equal to the main ray: p comes from the barycentrics and px from the plane equation, so px - p is rounding error,
    # exactly zero for some probes only; the rest have a minor axis of ~1e-7 that max_aniso rescales.  minorLength == 0 with
    # hasDifferentials true is also what the `tiny` quad (both 2x2 systems refused) and the parallel offsets (all zeroed) give.
    is_main = ok & ((okind == 3) | (okind == 4)) & (filt[-len(ok):] == "ewa") & ((om & ol.DIFFB["solve_x_fail"]) == 0)
    minor0, clamped = (om[is_main] & ol.TEXB["ewa_minor0"]) != 0, (om[is_main] & ol.TEXB["ewa_clamped"]) != 0
    print(f"offset ray equal to the main ray under EWA: {int(is_main.sum())} probes, minorLength == 0 for {int(minor0.sum())}, rescaled for {int(clamped.sum())}")
    assert is_main.sum() >= MIN_PROBES and clamped.sum() >= MIN_PROBES
    live_minor0 = valid & ((mask & ol.TEXB["ewa_minor0"]) != 0) & ((mask & ol.DIFFB["none"]) == 0)
    print(f"minorLength == 0 with hasDifferentials true: {int(live_minor0.sum())} valid probes")
    assert live_minor0.sum() >= MIN_PROBES


def test_eps_milli_probe_agrees_with_the_caller_differentials_probe():
    """gnxo_bsdf_probe's `flags | eps_milli << 8` form and gnxo_bsdf_probe_diff given the same offset rays return the same records."""
    from test_shading_queries import TEX, probes, synthetic_differentials
    osc = ol.OracleScene(scenes.textured_cornell(TEX, uv_quads=True))
    rays, wi, u = probes(2048, 132)
    for eps_milli in (2, 40):
        a = osc.bsdf_probe(rays, wi, u, 31 | (eps_milli << 8))
        b = osc.bsdf_probe_diff(rays, wi, u, synthetic_differentials(rays, eps_milli), 31)
        assert (a[:, 14] != 0).mean() >= 0.25
        assert biteq(a, b), mismatch(a, b)
    assert biteq(osc.bsdf_probe(rays, wi, u, 15), osc.bsdf_probe_diff(rays, wi, u, None, 15))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def sweep(gpu):
    return gpu.Scene(scenes.texture_filter_scene("sweep"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(5))
def test_device_against_the_reference_fixture(sweep, k):
    """Scene.bsdf under the reference driver's synthetic offset rays of size eps[k]: all 16 columns of every probe of the fixture"""
    g = golden("texture_filter.npz")
    rays, want = g["rays"], g["out"][:, k]
    assert len(g["eps"]) == 5 and want.shape == (len(rays), 16)
    got = dbsdf(sweep, rays, g["wi"], g["u"], 31, diffs=scenes.synthetic_differentials(rays, g["eps"][k]))
    assert (want[:, 13] == 1).mean() >= 0.25
    assert biteq(got, want), (float(g["eps"][k]), mismatch(got, want))


@pytest.mark.gpu
def test_device_against_the_oracle_under_caller_offset_rays(sweep):
    """offset origins away from the main origin, one offset far longer than the other (both ways), an offset ray equal to the main ray,
    an offset direction parallel to the surface, on quads facing x, y, z and two tilted directions: oracle_only_probes()"""
    rays, wi, u, diffs, kind, quad = oracle_only_probes()
    want = sweep_oracle().bsdf_probe_diff(rays, wi, u, diffs, 31)
    got = dbsdf(sweep, rays, wi, u, 31, diffs=diffs)
    assert (want[:, 13] == 1).mean() >= 0.25
    zeroed = (want[:, 13] == 1) & (kind >= 5)
    assert zeroed.sum() >= MIN_PROBES and (want[zeroed][:, 14:16] == 0).all()
    assert biteq(got, want), mismatch(got, want)


@pytest.mark.gpu
def test_unfiltered_lookups_against_the_oracle(sweep):
    """no differentials: MIPMap::triangle(0) alone, the only lookup PathIntegrator ever does, under all three wrap modes at the borders"""
    g = golden("texture_filter.npz")
    osc = sweep_oracle()
    for flags in (31, 15):
        want = osc.bsdf_probe(g["rays"], g["wi"], g["u"], flags)
        got = dbsdf(sweep, g["rays"], g["wi"], g["u"], flags)
        assert (want[:, 13] == 1).mean() >= 0.25 and (want[:, 14:16] == 0).all()
        assert biteq(got, want), (flags, mismatch(got, want))
    assert biteq(want, osc.bsdf_probe_diff(g["rays"], g["wi"], g["u"], None, 15))


def texture_image(builder, index):
    """decoded texels (h, w, 3) of texture `index` of a builder's description"""
    d = builder.desc()
    t = d.textures[index]
    n = t.width * t.height * 3
    return np.ctypeslib.as_array(d.texels, shape=(t.texel_offset + n,))[t.texel_offset:].copy().reshape(t.height, t.width, 3)


@pytest.mark.gpu
def test_filtered_lookups_after_a_device_side_pyramid_build(gpu):
    """Scene.update_textures replaces the 16x16 Repeat texture of one quad by the 33x17 image under Clamp (the pyramid is resampled and
    built on the device); the quad's probes, under the fixture's offset rays and the oracle-only ones, then equal the oracle on a scene
    authored with that texture -- and the other quads' results are what they were."""
    q = scenes.TEXTURE_FILTER_UPDATED_QUAD
    scene = gpu.Scene(scenes.texture_filter_scene("sweep"))
    bu = scenes.texture_filter_scene("updated")
    ti = scenes.texture_filter_texture_index(q)
    img = texture_image(bu, ti)
    assert img.shape == (17, 33, 3)
    scene.update_textures(img, first_texture=ti, params=dict(wrap=scenes.TEXTURE_FILTER_UPDATED["wrap"]))
    osc, before = ol.OracleScene(bu), sweep_oracle()
    g = golden("texture_filter.npz")
    rays, wi, u = g["rays"], g["wi"], g["u"]
    on = g["quad"] == q
    for e in g["eps"]:
        diffs = scenes.synthetic_differentials(rays, e)
        want = osc.bsdf_probe_diff(rays, wi, u, diffs, 31)
        got = dbsdf(scene, rays, wi, u, 31, diffs=diffs)
        assert biteq(got, want), (float(e), mismatch(got, want))
        old = before.bsdf_probe_diff(rays, wi, u, diffs, 31)
        assert (want[on][:, 0:3] != old[on][:, 0:3]).any(1).sum() >= MIN_PROBES and biteq(want[~on], old[~on])
    orays, owi, ou, odiffs, okind, oquad = oracle_only_probes()
    want = osc.bsdf_probe_diff(orays, owi, ou, odiffs, 31)
    got = dbsdf(scene, orays, owi, ou, 31, diffs=odiffs)
    assert biteq(got, want), mismatch(got, want)


@pytest.mark.gpu
def test_aov_albedo_of_the_black_wrap_quad(gpu, sweep):
    """RenderAOV's albedo on the Black-wrap quad whose uv runs from -1.5 to 2.5: per pixel (spp 1) albedo * fp32(1 / pi) is the oracle's
    Lambert f of the unfiltered Kd; outside the image's one tile Kd is black, the albedo exactly zero and the material without a lobe."""
    from test_aov import aov, samples
    gx = gpu
    q = next(i for i, r in enumerate(QUADS) if r["name"] == "ewa_black")
    c, e1, e2, half, _ = scenes.texture_filter_quad(q)
    nrm = np.cross(e1, e2)
    cam = dict(eye=tuple(c + 2.5 * nrm + 0.2 * e1), look=tuple(c), up=tuple(e2), fov=60.0)
    W, H = 40, 32
    out, _ = aov(gx, sweep, W, H, 1, cameras=[gx.camera(**cam)], channels=("albedo", "ids"))
    rays, prim, t, n = samples(gx, sweep, cam, W, H, [0])
    rays = rays[0].reshape(-1, 8)
    wi = np.broadcast_to(nrm.astype(np.float32), (len(rays), 3))
    u = np.full((len(rays), 2), 0.5, np.float32)
    want = sweep_oracle().bsdf_probe(rays, wi, u, 31)
    alb = out["albedo"][0][..., :3].reshape(-1, 3)
    on = want[:, 13] == 1
    assert (on == (prim[0].reshape(-1) >= 0)).all() and on.sum() >= 200
    assert biteq(alb * np.float32(1 / np.pi), want[:, 0:3]), mismatch(alb * np.float32(1 / np.pi), want[:, 0:3])
    black = on & (alb == 0).all(1)
    lit = on & (alb != 0).any(1)
    assert black.sum() >= 100 and lit.sum() >= 30
    assert (want[black][:, 12] == 0).all() and (want[lit][:, 12] == 1).all()
    got = dbsdf(sweep, rays, wi, u, 31)
    assert biteq(got, want), mismatch(got, want)
