"""The MIS half of EstimateDirect, direction first (k_shade with SM_DIR_FIRST / SM_DEFER in csrc/kernels.hip.h; shade_stage in
csrc/api_render.hip.h): where every light is an area light the shade kernels sample the BSDF's direction, ask light_pdf, and evaluate f and
the pdf only at the vertices whose direction reaches the sampled light; those rare vertices wait on a list per wave in LDS and are evaluated
together.

Every GPU case compares bit for bit -- the image and rays_closest, rays_any, camera_samples, rays_closest_nee -- against the oracle (which counts rays_closest and rays_any) and
against the same library with GNXR_NO_MIS_DEFER=1 (k_shade<LM, LT_AREA>, the kernels every other light set runs).  The modes of a case:
the default (a list of up to 64 entries a wave, drained once it is full and after the wave's last vertex), GNXR_MIS_DEFER_DRAIN_AT = 1, 3
(drains between vertices) and GNXR_MIS_DEFER_STEP=1 (direction first without the list)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import scenes
from test_light_update import mesh_light_scene
from test_material_queues import LM_CONDUCTOR, LM_ROUGH_DIELECTRIC, MeshScene, biteq, mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 96, 64, 4, 8
SWITCH, STEP, DRAIN_AT = "GNXR_NO_MIS_DEFER", "GNXR_MIS_DEFER_STEP", "GNXR_MIS_DEFER_DRAIN_AT"
COUNTS = ("rays_closest", "rays_any", "camera_samples", "rays_closest_nee")
ORACLE_COUNTS = COUNTS[:2]   # what the oracle counts (its rays_closest includes the MIS rays, as the device's)
LM_DIFFUSE = 3
LT_AREA, SM_DIR_FIRST, SM_DEFER = 1, 16, 32
MODES = {"default": {}, "drain_at_1": {DRAIN_AT: "1"}, "drain_at_3": {DRAIN_AT: "3"}, "step_1": {STEP: "1"}, "off": {SWITCH: "1"}}


# ---------------------------------------------------------------- helpers
def render(gx, scene, mode, w=W, h=H, spp=SPP, **kw):
    """one render with the environment of `mode` (all three variables are read per render call)"""
    old = {k: os.environ.pop(k, None) for k in (SWITCH, STEP, DRAIN_AT)}
    try:
        os.environ.update(MODES[mode])
        return gx.PathIntegrator(DEPTH, 1.0, "spatial").Render(scene, w, h, spp, **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def same(a, b, counts=COUNTS):
    (ia, sa), (ib, sb) = a, b
    assert [sa[c] for c in counts] == [sb[c] for c in counts], ([sa[c] for c in counts], [sb[c] for c in counts])
    assert biteq(ia[..., :3], ib[..., :3])


def all_matte(gx, **kw):
    """the mesh with the box's white Matte on every triangle (material 0: the first the builder makes)"""
    def assign(ids, m):
        ids[:] = 0
    return MeshScene(gx, ("metal",), assign, **kw)


BUILDERS = {"matte": lambda gx: all_matte(gx).b, "metal_glass": lambda gx: mixed(gx, ("metal", "glass")).b,
            "sphere": lambda gx: mixed(gx, ("metal", "glass"), sphere="metal").b, "mesh_light": lambda gx: mesh_light_scene()}
_cache = {}


def case(gx, name):
    """the builder, the scene, the oracle's render and the render with the switch set, computed once per scene and left unchanged"""
    if name not in _cache:
        b = BUILDERS[name](gx)
        scene = gx.Scene(b)
        oracle = ol.OracleScene(b).render(gx.PathIntegrator(DEPTH, 1.0, "spatial"), W, H, SPP)
        off = render(gx, scene, "off")
        same(off, oracle, ORACLE_COUNTS)
        assert off[1]["rays_closest_nee"] > 0 and np.isfinite(off[0]).all() and off[0][..., :3].max() > 0
        _cache[name] = (b, scene, oracle, off)
    return _cache[name]


# ---------------------------------------------------------------- CPU: the kernels as compiled
def test_reordered_kernels_hold_three_waves_and_the_others_are_the_parents(gx):
    """tools/kernel_regs.py on libgnxr.so against profiles/kernel_regs_material_queues.txt (the report of the parent's k_shade kernels):
    the diffuse, conductor and rough-dielectric kernels for area lights with SM_DIR_FIRST and SM_DEFER hold three waves per SIMD with no
    more scratch than the parent's kernel for that material, and every k_shade without the mode bits has the parent's line."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = kernel_regs.kernels(gx.LIB_PATH)

    def line(k):
        return (k["vgpr"], k["agpr"], k["sgpr"], k["sgpr_spill"], k["vgpr_spill"], k["scratch"], k["lds"], k["waves_per_simd"])
    parent = {}
    for ln in open(os.path.join(ROOT, "profiles", "kernel_regs_material_queues.txt")):
        if "gnxr::k_shade<" in ln:
            f = ln.split()
            name = ln[ln.index("void gnxr::k_shade<"):].split("(")[0].strip()
            parent[name] = (int(f[0][:-1]), int(f[1][:-1]), int(f[2][:-1]), int(f[5]), int(f[7]), int(f[9]), int(f[11]), int(f[13]))
    assert len(parent) == 25
    mine = {k["name"].split("(")[0].strip(): k for k in ks if "gnxr::k_shade<" in k["name"]}
    for name, p in parent.items():
        assert name in mine and line(mine[name]) == p, (name, p, mine.get(name))
    failures = []
    for lm in (LM_DIFFUSE, LM_CONDUCTOR, LM_ROUGH_DIELECTRIC):
        base = parent["void gnxr::k_shade<%du, %d, false, false>" % (lm, LT_AREA)]
        for mode in (SM_DIR_FIRST, SM_DEFER):
            k = mine["void gnxr::k_shade<%du, %d, false, false>" % (lm, LT_AREA | mode)]
            print(lm, mode, line(k), "parent", base)
            if not (k["waves_per_simd"] >= 3 and k["scratch"] <= base[5]):
                failures.append((lm, mode, k["waves_per_simd"], k["scratch"], base[5]))
    assert not failures, failures


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "drain_at_1", "drain_at_3", "step_1"])
@pytest.mark.parametrize("name", ["matte", "metal_glass", "sphere"])
def test_three_kernels(gpu, name, mode):
    """the 2 k-triangle mesh in the Cornell box -- all matte (the diffuse kernel alone), metal and rough glass triangle by triangle (three
    class kernels), and with a sphere (the SPH kernels, one glossy queue): a few hundredths of the vertices have a MIS ray, so with the
    default threshold a wave's list drains once, partly filled, after its last vertex"""
    b, scene, oracle, off = case(gpu, name)
    on = render(gpu, scene, mode)
    same(on, off)
    same(on, oracle, ORACLE_COUNTS)
    assert on[1]["kernel_launches"] == off[1]["kernel_launches"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "drain_at_3", "step_1"])
def test_a_light_table_beyond_lds(gpu, mode):
    """302 lights (an emissive sheet of 300 triangles): the light table stays in global memory, the list sits behind the other tables"""
    b, scene, oracle, off = case(gpu, "mesh_light")
    on = render(gpu, scene, mode)
    same(on, off)
    same(on, oracle, ORACLE_COUNTS)


@pytest.mark.gpu
def test_other_light_sets_keep_their_kernels(gpu):
    """with an InfiniteAreaLight the plan launches k_shade<LM, LT_AREA | LT_ENV>: the switch changes nothing, not even the launches"""
    scene = gpu.Scene(mixed(gpu, ("metal", "glass"), env=True).b)
    on, off = render(gpu, scene, "default"), render(gpu, scene, "off")
    same(on, off)
    assert on[1]["kernel_launches"] == off[1]["kernel_launches"] and on[1]["rays_closest_nee"] > 0


def sheet_scene():
    """the glass + metal mesh in the box under a flat emissive quad as wide as emissive_sheet() of tests/test_light_update.py"""
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=os.path.join(ROOT, "tests", "golden", "mesh_2k.3d"))
    v = np.array([[-1.6, 1.5, -1.2], [-1.6, 1.5, 1.4], [1.6, 1.5, 1.4], [1.6, 1.5, -1.2]], np.float32)
    b.add_emissive_mesh(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), 0, (0.4, 0.35, 0.3), n_samples=1)
    return b


def sheet_integrator():
    import gnxraytracer_amd as gx
    return gx.PathIntegrator(DEPTH, 1.0, "spatial")


SW, SH, SSPP = 256, 192, 8


def child(out):
    """the renders of test_frequent_hits_drain_inside_the_loop, in a process with GNXR_SHADE_BLOCKS_PER_CU=1 (read once per process)"""
    import torch  # noqa: F401  (before libgnxr.so is loaded)
    import gnxraytracer_amd as gx
    gx.init(0)
    scene = gx.Scene(sheet_scene())
    res = {}
    for tag, env in (("off", {SWITCH: "1"}), ("at4", {DRAIN_AT: "4"}), ("at64", {DRAIN_AT: "64"}), ("step1", {STEP: "1"})):
        for k in (SWITCH, STEP, DRAIN_AT):
            os.environ.pop(k, None)
        os.environ.update(env)
        img, st = sheet_integrator().Render(scene, SW, SH, SSPP)
        res[tag] = img
        res[tag + "_counts"] = np.array([st[c] for c in COUNTS], np.int64)
    np.savez(out, **res)


@pytest.mark.gpu
def test_frequent_hits_drain_inside_the_loop(gpu, tmp_path):
    """a light as wide as the box's ceiling, 256 x 192 at 8 spp on one block per CU: 393 k paths on 65 536 lanes, six vertices a lane and
    384 a wave, of which 3 % or more append -- with GNXR_MIS_DEFER_DRAIN_AT=4 a wave drains several times between vertices, with 64
    (nearly) only after its last one"""
    out = str(tmp_path / "sheet.npz")
    env = dict(os.environ, GNXR_SHADE_BLOCKS_PER_CU="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    for k in (SWITCH, STEP, DRAIN_AT):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    oimg, ost = ol.OracleScene(sheet_scene()).render(sheet_integrator(), SW, SH, SSPP)
    off = dict(zip(COUNTS, (int(v) for v in z["off_counts"])))
    print("counts", off, "MIS share %.3f" % (off["rays_closest_nee"] / off["rays_any"]))
    # (the oracle does not count the MIS rays apart: the bar is checked on the render with the switch set, k_shade<LM, LT_AREA>)
    assert off["rays_closest_nee"] >= 0.03 * off["rays_any"]
    for tag in ("off", "at4", "at64", "step1"):
        assert list(z[tag + "_counts"]) == list(z["off_counts"]), (tag, list(z[tag + "_counts"]), off)
        assert [int(v) for v in z[tag + "_counts"][:2]] == [ost[c] for c in ORACLE_COUNTS], (tag, ost)
        assert biteq(z[tag][..., :3], oimg[..., :3]), tag
        assert biteq(z[tag], z["off"]), tag


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert sys.argv[1] == "--child"
    child(sys.argv[2])
