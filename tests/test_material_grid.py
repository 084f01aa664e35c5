"""BSDFs and delta lights across their parameter space (scenes.MATERIAL_GRID, scenes.DELTA_GRID) instead of one preset per material type.

The chain is compiled reference -> fixtures (tests/golden/bsdf_grid_*.npz, light_delta.npz, written by oracle/make_goldens.py) -> CPU
oracle -> device.  The CPU tests here tie the oracle to the fixtures bit for bit (NaN equal to NaN), state on the REFERENCE's numbers the
conditions that keep an all-zero or all-invalid result from passing, and pin the routing of every grid material through compile_material
(number of lobes, shade class, material kind) to a table derived by hand from the reference's material sources.  The function-level GPU
tests on the same fixtures are in tests/test_shading_queries.py; the GPU tests here put the grid through the shade kernels, which the
bsdf query does not run: groups of grid materials on the 2 k-triangle mesh in the Cornell box, rendered by all four integrators and
compared with the oracle's render bit for bit, and a walk through one group by live material edits.  No tolerances anywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import scenes
from conftest import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnxraytracer_amd", "csrc")
MESH2K = os.path.join(GOLDEN, "mesh_2k.3d")
W, H, SPP, DEPTH = 48, 40, 4, 8
SWITCH = "GNXR_NO_MATERIAL_QUEUES"
COUNTS = ("rays_closest", "rays_any", "camera_samples")
NAMES = scenes.MATERIAL_GRID_NAMES

# ---------------------------------------------------------------- what the fixtures must show (by name)
# no lobe at all: black Kd (Matte), black Kr (Mirror), black Kr and Kt (Glass), black Kd and Ks (Plastic)
ALL_BLACK = {"matte_black", "mirror_black", "glass_black_rough", "plastic_black"}
# specular lobes only: f() and Pdf() are 0 by definition, only Sample_f answers
SPECULAR_ONLY = {"mirror_bright", "glass_smooth", "glass_smooth_t", "glass_smooth_r", "glass_smooth_eta1"}
# MicrofacetTransmission at eta == 1: the refracted direction is -wo, wo + eta * wi vanishes and its normalisation is 0 / 0.  The reference
# returns NaN whenever such a material samples (or is asked about) its transmission lobe; the device must return the same records
NAN_MATERIALS = {"glass_rough_eta1", "disney_eta1", "disney_eta1_spectrans08", "disney_thin_eta1"}

# ---------------------------------------------------------------- routing, derived by hand from the reference's material sources
# name -> (lobes with allowMultipleLobes, lobes without (Whitted), shade class, material kind)
#   shade class: 0 at most one Lambert / Oren-Nayar lobe, 1 specular and plain microfacet lobes (and Lambert beside them), 2 any Disney lobe
#   kind (class 1 only): 1 conductor = one microfacet reflection with the conductor Fresnel term; 2 rough dielectric = microfacet reflection /
#   transmission with the dielectric Fresnel term and nothing else; 0 everything else
# MatteMaterial: one lobe unless Kd is black (sigma only picks Lambert or Oren-Nayar).  MirrorMaterial: one specular lobe unless Kr is black.
# GlassMaterial: nothing when Kr and Kt are black; smooth (urough == vrough == 0): FresnelSpecular, or with allowMultipleLobes == false a
# SpecularReflection if Kr and a SpecularTransmission if Kt is not black; rough: MicrofacetReflection if Kr, MicrofacetTransmission if Kt.
# MetalMaterial: always one MicrofacetReflection(FresnelConductor).  PlasticMaterial: Lambert if Kd, MicrofacetReflection(FresnelDielectric
# (1.5, 1)) if Ks is not black -- with a black Kd that single lobe is all a rough dielectric is.  DisneyMaterial: with diffuseWeight =
# (1 - metallic)(1 - specTrans) > 0: DisneyDiffuse (+ DisneyFakeSS when thin), DisneyRetro, DisneySheen if sheen > 0; always the
# MicrofacetReflection(DisneyFresnel); DisneyClearcoat if clearcoat > 0; MicrofacetTransmission if specTrans > 0; LambertianTransmission
# when thin.  No colour test drops a Disney lobe.
MATTE, SPEC, COND, DIEL = (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (2, 2, 1, 2)
NONE = (0, 0, 0, 0)
ROUTING = {
    "matte_sigma0": MATTE, "matte_sigma1": MATTE, "matte_sigma90": MATTE, "matte_sigma200": MATTE, "matte_sigma_neg": MATTE, "matte_black": NONE,
    "matte_kd_clamped": MATTE,
    "mirror_black": NONE, "mirror_bright": SPEC,
    "glass_smooth": (1, 2, 1, 0), "glass_smooth_t": SPEC, "glass_smooth_r": SPEC, "glass_black_rough": NONE, "glass_smooth_eta1": (1, 2, 1, 0),
    "glass_rough_eta1": DIEL, "glass_rough_eta07": DIEL, "glass_u0_remap": DIEL, "glass_u0": DIEL, "glass_rough1_remap": DIEL,
    "glass_rough_t_eta24": (1, 1, 1, 2), "glass_rough_r": (1, 1, 1, 2),
    "metal_001_remap": COND, "metal_0_remap": COND, "metal_0": COND, "metal_aniso": COND, "metal_k0": COND, "metal_eta1_k0": COND, "metal_2_05_remap": COND,
    "plastic_purple": (2, 2, 1, 0), "plastic_black_kd": (1, 1, 1, 2), "plastic_black_ks": MATTE, "plastic_black": NONE, "plastic_u0_remap": (2, 2, 1, 0),
    "plastic_u0": (2, 2, 1, 0), "plastic_u1_remap": (2, 2, 1, 0),
    # diffuse 3 (diffuse, retro, sheen) + specular 1 + clearcoat 1 + transmission 1
    "disney_preset": (6, 6, 2, 0), "disney_metallic1": (3, 3, 2, 0), "disney_opaque": (5, 5, 2, 0), "disney_spectrans1": (3, 3, 2, 0),
    "disney_metallic1_spectrans1": (3, 3, 2, 0), "disney_clearcoat0": (5, 5, 2, 0), "disney_sheen0": (5, 5, 2, 0), "disney_clearcoat1_gloss0": (6, 6, 2, 0),
    "disney_gloss1": (6, 6, 2, 0), "disney_rough0": (6, 6, 2, 0), "disney_rough1": (6, 6, 2, 0), "disney_rough001_aniso1": (6, 6, 2, 0),
    "disney_aniso1": (6, 6, 2, 0), "disney_aniso0": (6, 6, 2, 0), "disney_black": (6, 6, 2, 0), "disney_black_tints1": (6, 6, 2, 0),
    "disney_eta1": (6, 6, 2, 0), "disney_eta1_spectrans08": (6, 6, 2, 0), "disney_spectint1_sheentint0": (6, 6, 2, 0),
    # thin: diffuse 4 (diffuse, fake subsurface, retro, sheen) + specular 1 + clearcoat 1 + transmission 1 + Lambertian transmission 1
    "disney_thin": (8, 8, 2, 0), "disney_thin_flat1_difftrans2": (8, 8, 2, 0), "disney_thin_plain": (7, 7, 2, 0), "disney_thin_trans1": (4, 4, 2, 0),
    "disney_thin_metallic1": (4, 4, 2, 0), "disney_thin_eta1": (8, 8, 2, 0), "disney_thin_eta05": (8, 8, 2, 0), "disney_sheen2_clearcoat2": (6, 6, 2, 0),
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def rows_of(material):
    """per grid material: the slice of its probes in the joined fixture"""
    assert np.array_equal(material, np.repeat(np.arange(len(NAMES)), scenes.MATERIAL_GRID_PROBES))
    return {name: slice(i * scenes.MATERIAL_GRID_PROBES, (i + 1) * scenes.MATERIAL_GRID_PROBES) for i, name in enumerate(NAMES)}


def spot_band(light, ref_p, rec):
    """records of a spot light strictly inside its falloff band: 0 < Li d^2 < I in every channel (d from the light's position, float64)"""
    pos = np.array(light["xf"], np.float32).astype(np.float64)[:3, 3]
    d2 = ((ref_p.astype(np.float64) - pos) ** 2).sum(1)
    q = rec[:, :3].astype(np.float64) * d2[:, None]
    return ((q > 0) & (q < np.array(light["I"], np.float64))).all(1)


# ---------------------------------------------------------------- CPU: fixtures, oracle, routing
def test_material_grid_fixture_and_oracle():
    """The conditions on the reference's numbers, then the oracle against them.  The grid holds every case the routing table names."""
    assert set(ROUTING) == set(NAMES) and len(NAMES) == len(set(NAMES))
    assert ALL_BLACK == {n for n, r in ROUTING.items() if r[0] == 0}
    assert SPECULAR_ONLY == {n for n, r in ROUTING.items() if r[2] == 1 and r[3] == 0 and n.split("_")[0] in ("mirror", "glass")}
    g = scenes.material_grid_golden()
    assert len(g["rays"]) == len(NAMES) * scenes.MATERIAL_GRID_PROBES
    rows = rows_of(g["material"])
    outs = {f: g[f"out_{f}"] for f in scenes.MATERIAL_GRID_FLAGS}
    for f, o in outs.items():
        assert o.shape == (len(g["rays"]), 16) and (o[:, 13] == 1).all(), f         # every aimed ray hits and finds a BSDF
    o31 = outs[31]
    zero, nan = set(), set()
    for name, s in rows.items():
        r = o31[s]
        f_share, pdf_share = float((r[:, :3] > 0).any(1).mean()), float((r[:, 7] > 0).mean())
        print(f"{name}: f > 0 on {f_share:.3f}, sampled pdf > 0 on {pdf_share:.3f}, components {r[0, 12]:.0f}")
        assert (r[:, 12] == ROUTING[name][0]).all(), name                            # BSDF::NumComponents of the reference itself
        if name not in ALL_BLACK and name not in SPECULAR_ONLY:
            assert f_share >= 0.1, (name, f_share)
        if name not in ALL_BLACK:
            assert pdf_share >= 0.4, (name, pdf_share)
        if all((o[s][:, :13] == 0).all() for o in outs.values()):
            zero.add(name)
        if any(np.isnan(o[s]).any() for o in outs.values()):
            nan.add(name)
    assert zero == ALL_BLACK, zero ^ ALL_BLACK
    assert nan == NAN_MATERIALS, nan ^ NAN_MATERIALS
    osc = ol.OracleScene(scenes.material_grid())
    for f, want in outs.items():
        got = osc.bsdf_probe(g["rays"], g["wi"], g["u"], f)
        bad = ~same_bits(got, want).all(1)
        assert not bad.any(), (f, sorted({NAMES[m] for m in g["material"][bad]}), np.nonzero(bad)[0][:5].tolist())


def test_light_delta_fixture_and_oracle():
    g = golden("light_delta.npz")
    b, first = scenes.delta_grid()
    assert int(g["first_light"]) == first and g["out"].shape == (len(scenes.DELTA_GRID), scenes.DELTA_GRID_PROBES, 12)
    osc = ol.OracleScene(b)
    keep = [c for c in range(12) if c != 8]      # column 8 (the selection pdf) is not produced by the reference
    for k, l in enumerate(scenes.DELTA_GRID):
        r, p = g["out"][k], g["refP"][k]
        if l["kind"] == "spot" and l["falloff_start"] < l["total_width"]:
            share = float(spot_band(l, p, r).mean())
            print(f"{l['name']}: {share:.3f} of the records strictly inside the falloff band")
            assert share > 0.1, (l["name"], share)
        got = osc.light_probe(first + k, p, g["refN"], g["u"], g["wiQ"])
        pdf_pos = r[:, 3] > 0                    # the reference leaves P1 unset otherwise
        assert same_bits(got[:, :8], r[:, :8]).all(), l["name"]
        assert same_bits(got[pdf_pos, 9:], r[pdf_pos, 9:]).all(), l["name"]
        assert pdf_pos.mean() > 0.9, l["name"]
    # a light queried at its own position: the reference's records are not finite there, and the fixture holds some for every point / spot light
    for k, l in enumerate(scenes.DELTA_GRID):
        if l["kind"] != "distant":
            assert (~np.isfinite(g["out"][k][:, :7])).any(), l["name"]


def test_compile_material_routing(gx, tmp_path):
    """compile_material on every grid material, in a stand-alone program over the library's host sources (tests/material_routing_check.cpp):
    lobes (both allowMultipleLobes settings), shade class and material kind against ROUTING.  The black-Kd Plastic is a rough dielectric."""
    assert ROUTING["plastic_black_kd"] == (1, 1, 1, 2)
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe, records = str(tmp_path / "material_routing_check"), str(tmp_path / "materials.bin")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "material_routing_check.cpp"), os.path.join(CSRC, "scene_compile.cpp"), os.path.join(CSRC, "scene_builder.cpp"),
                           "-o", exe, "-lpthread"])
    with open(records, "wb") as f:
        for name in NAMES:
            f.write(bytes(scenes.grid_material(name)))
    r = subprocess.run([exe, records], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and len(lines) >= len(NAMES), r.stdout
    got = {NAMES[int(t[0])]: tuple(int(v) for v in t[1:]) for t in (ln.split() for ln in lines[:len(NAMES)])}
    wrong = {n: (got[n], ROUTING[n]) for n in NAMES if got[n] != ROUTING[n]}
    assert not wrong, wrong
    # the records the builder stores are the ones written above
    b = scenes.material_grid()      # (kept alive: the description points into the builder)
    d = b.desc()
    assert d.n_materials == len(NAMES) and all(bytes(d.materials[i]) == bytes(scenes.grid_material(n)) for i, n in enumerate(NAMES))


# ---------------------------------------------------------------- GPU: the grid through the shade kernels
# The eta == 1 materials with a microfacet transmission lobe (NAN_MATERIALS) stay out of every render: their radiance is NaN in the reference
# itself, NaN payloads differ between machines, and images are compared on bit patterns.  They are pinned at function level.
# group -> (materials taken in turn by the mesh's triangles, whether the PathIntegrator's plan gains a shade queue over the shared glossy one)
GROUPS = {
    # class 0 only, the lobe-less black Matte included: k_shade<LM_DIFFUSE>
    "matte": ([n for n in NAMES if n.startswith("matte_")], False),
    # one kind: the conductor kernel runs on the single glossy queue
    "metal": ([n for n in NAMES if n.startswith("metal_")], False),
    # one kind: the rough-dielectric kernel; R only, T only, eta < 1, RoughnessToAlpha(0), the black-Kd Plastic, and a lobe-less Glass beside them
    "rough_dielectric": (["glass_rough_r", "glass_rough_t_eta24", "glass_rough_eta07", "plastic_black_kd", "glass_u0_remap", "glass_u0", "glass_rough1_remap",
                          "glass_black_rough"], False),
    # conductor, rough dielectric and Plastic (class 1, no kind): three glossy queues
    "metal_glass_plastic": (["metal_aniso", "glass_rough_eta07", "plastic_purple", "metal_k0", "glass_u0_remap", "plastic_u0"], True),
    # Plastic across its branches: no kind, rough dielectric (black Kd), class 0 (black Ks), no lobe: two glossy queues
    "plastic": ([n for n in NAMES if n.startswith("plastic_")], True),
    # class 2: the wide kernel
    "disney": ([n for n in NAMES if n.startswith("disney_") and "thin" not in n and n not in NAN_MATERIALS], False),
    "disney_thin": ([n for n in NAMES if n.startswith("disney_thin") and n not in NAN_MATERIALS], False),
    # specular lobes: class 1 without a kind, one queue; Whitted's allowMultipleLobes == false splits smooth glass in two droppable lobes
    "specular": (["glass_smooth", "glass_smooth_r", "glass_smooth_t", "glass_smooth_eta1", "mirror_bright", "mirror_black"], False),
}
INTEGRATORS = {"path": lambda gx: gx.PathIntegrator(DEPTH, 1.0, "spatial"), "volpath": lambda gx: gx.VolPathIntegrator(DEPTH, 1.0, "spatial"),
               "whitted": lambda gx: gx.WhittedIntegrator(DEPTH), "direct_all": lambda gx: gx.DirectLightingIntegrator("all", DEPTH)}


def test_groups_cover_the_grid_and_every_plan():
    """every grid material that can be rendered is in a group; what each group is meant to reach follows from ROUTING"""
    used = {n for names, _ in GROUPS.values() for n in names}
    assert used == set(NAMES) - NAN_MATERIALS and not (used & NAN_MATERIALS)
    kinds = lambda g: {ROUTING[n][3] for n in GROUPS[g][0] if ROUTING[n][2] == 1}
    classes = lambda g: {ROUTING[n][2] for n in GROUPS[g][0]}
    assert classes("matte") == {0} and classes("disney") == {2} and classes("disney_thin") == {2}
    assert kinds("metal") == {1} and kinds("rough_dielectric") == {2} and kinds("specular") == {0}
    assert kinds("metal_glass_plastic") == {0, 1, 2} and kinds("plastic") == {0, 2}
    # a queue is gained exactly where class-1 materials of more than one kind meet
    for g, (_, more) in GROUPS.items():
        assert more == (len(kinds(g)) > 1), g


class GridMeshScene:
    """The 2 k-triangle mesh in the Cornell box with its area light (MeshScene of tests/test_material_queues.py); triangle i of the mesh
    takes material names[i % len(names)] of the grid."""

    def __init__(self, gx, names):
        b = self.b = gx.SceneBuilder()
        white, red, blue = (b.MatteMaterial(c, 60.0) for c in (scenes.WHITE, scenes.RED, scenes.BLUE))
        self.m = [scenes.add_grid_material(b, n) for n in names]
        self.first = b.AddModel(MESH2K, self.m[0])
        d = b.desc()
        self.n = d.n_triangles - self.first
        ids = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))[self.first:self.first + self.n]
        for i, m in enumerate(self.m):
            ids[i::len(self.m)] = m
        b.AddCornell(red, blue, white)
        b.AddAreaLight(white)


def render(integ, scene, split=True):
    old = os.environ.pop(SWITCH, None)
    try:
        if not split:
            os.environ[SWITCH] = "1"   # read per render call
        return integ.Render(scene, W, H, SPP)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def same_render(a, b, what, counts=COUNTS):
    (ia, sa), (ib, sb) = a, b
    ca, cb = [sa[c] for c in counts], [sb[c] for c in counts]
    differ = ~same_bits(ia, ib)
    assert ca == cb and not differ.any(), (what, ca, cb, f"{int(differ.any(-1).sum())} of {W * H} pixels differ, first {np.argwhere(differ.any(-1))[:3].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", list(INTEGRATORS))
@pytest.mark.parametrize("group", list(GROUPS))
def test_grid_group_renders_like_the_oracle(gpu, group, integrator):
    """48 x 40 at 4 spp, maxDepth 8: image, rays_closest, rays_any and camera_samples equal the oracle's, bit for bit.  Under the
    PathIntegrator, whose plan gives material kinds shade queues of their own, the render also equals the one under
    GNXR_NO_MATERIAL_QUEUES (the shared glossy kernel), with more launches exactly where the group gains a queue."""
    names, more_launches = GROUPS[group]
    ms = GridMeshScene(gpu, names)
    integ = INTEGRATORS[integrator](gpu)
    scene = gpu.Scene(ms.b)
    on = render(integ, scene)
    img, st = on
    assert st["rays_closest"] > 0 and np.isfinite(img).all() and img[..., :3].max() > 0
    same_render(on, ol.OracleScene(ms.b).render(integ, W, H, SPP), (group, integrator, "oracle"), COUNTS[:2])   # (the oracle counts no camera samples)
    assert st["camera_samples"] == W * H * SPP
    if integrator == "path":
        off = render(integ, scene, split=False)
        same_render(on, off, (group, "split on / off"))
        if more_launches:
            assert st["kernel_launches"] > off[1]["kernel_launches"], (st["kernel_launches"], off[1]["kernel_launches"])
        else:
            assert st["kernel_launches"] == off[1]["kernel_launches"], (st["kernel_launches"], off[1]["kernel_launches"])


@pytest.mark.gpu
def test_live_edits_walk_the_rough_dielectric_group(gpu):
    """The mesh carries ONE material record, first glass_rough_r; update_materials turns it into every other material of the group in turn
    (rough Glass with one or two lobes, the black-Kd Plastic -- another material type of the same kind --, a lobe-less Glass of class 0)
    and back.  After each step the scene renders as a scene created fresh with that record does, and reports the same per-triangle state."""
    from test_material_update import desc_materials, fresh_scene, with_record
    names = GROUPS["rough_dielectric"][0]
    ms = GridMeshScene(gpu, names[:1])
    m = ms.m[0]
    scene = gpu.Scene(ms.b)
    mats0 = desc_materials(gpu, ms.b)
    integ = INTEGRATORS["path"](gpu)
    first = render(integ, scene)
    seen = [first[0]]
    for name in names[1:] + names[:1]:
        rec = scenes.grid_material(name)
        scene.update_materials([rec], m)
        fresh = fresh_scene(gpu, ms.b, materials=with_record(mats0, m, rec))
        got = render(integ, scene)
        same_render(got, render(integ, fresh), (name, "fresh scene"))
        same_render(got, render(integ, scene, split=False), (name, "split on / off"))
        for x, y in zip(scene.triangle_materials(), fresh.triangle_materials()):
            assert np.array_equal(x, y), name
        cls = scene.triangle_materials()[1][ms.first:ms.first + ms.n]
        assert (cls == ROUTING[name][2]).all(), (name, np.unique(cls))
        assert got[1]["rays_closest"] > 0 and np.isfinite(got[0]).all() and got[0][..., :3].max() > 0
        seen.append(got[0])
    assert same_bits(seen[-1], seen[0]).all()                                        # back at the first material
    assert all(not same_bits(seen[i], seen[i + 1]).all() for i in range(len(seen) - 1))   # every step changed the picture
