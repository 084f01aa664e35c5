"""One shade queue per kind of glossy material (plan_shade_queues in csrc/api_render.hip.h, material_kind in csrc/scene_compile.cpp): Metal
(conductor) and rough Glass (rough dielectric) hits are binned apart and shaded by k_shade<LM_CONDUCTOR> / k_shade<LM_ROUGH_DIELECTRIC>.

The reference of every GPU case is the same library with GNXR_NO_MATERIAL_QUEUES set, which forces the plan with ONE glossy queue and
k_shade<LM_GLOSSY> -- the plan that the parity suites tie to the oracle.  Every comparison is bit for bit: the image and the three counts
rays_closest, rays_any, camera_samples.  Where the plan gains a queue, kernel_launches must be larger with the split than without, so that no
case passes because the split never ran; where it falls back, or where the scene has one kind only (the narrow kernel then runs on the one
glossy queue: no launch more), kernel_launches must be equal.  The 2 k-triangle mesh of the refit tests in the Cornell box, 96 x 64 at
4 spp, maxDepth 8."""
import os
import sys

import numpy as np
import pytest

import scenes
from gnxraytracer_amd import _abi as A
from test_material_update import desc_materials, fresh_scene, with_record
from test_scene_update import ENV, MESH2K, biteq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 96, 64, 4, 8
SWITCH = "GNXR_NO_MATERIAL_QUEUES"
COUNTS = ("rays_closest", "rays_any", "camera_samples")
# device_bsdf.h: lobe_bit(LOBE_MICRO_REFL = 5) | lobe_bit(LOBE_MICRO_TRANS = 6) | fresnel_bit(k) = 1 << (16 + k), DIELECTRIC = 1, CONDUCTOR = 2
LM_GLOSSY, LM_CONDUCTOR, LM_ROUGH_DIELECTRIC = 458879, (1 << 5) | (1 << 18), (1 << 5) | (1 << 6) | (1 << 17)


# ---------------------------------------------------------------- helpers
class MeshScene:
    """The mesh in the Cornell box with the materials `names` in the scene's table (the plan counts the materials of the table, used or
    not); `assign(ids, m)` fills the mesh's per-triangle material ids from the dictionary of material indices."""

    def __init__(self, gx, names, assign, env=False, sphere=None):
        b = self.b = gx.SceneBuilder()
        white, red, blue = (b.MatteMaterial(c, 60.0) for c in (scenes.WHITE, scenes.RED, scenes.BLUE))
        make = {"glass": b.getWhiteGlassMaterial, "metal": b.getYelloMetalMaterial, "plastic": b.getPurplePlasticMaterial,
                "disney": lambda: scenes.disney_preset(b),
                "sglass": lambda: b.add_material(type=A.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0)}
        self.m = m = {n: make[n]() for n in names}
        self.first = b.AddModel(MESH2K, m[names[0]])
        d = b.desc()
        self.n = d.n_triangles - self.first
        ids = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
        assign(ids[self.first:self.first + self.n], m)
        b.AddCornell(red, blue, white)
        b.AddAreaLight(white)
        if env:
            b.AddInfLight(ENV)
        if sphere:
            b.AddSphere((0.6, -1.5, 0.2), 0.5, m[sphere])

    def ids(self):
        d = self.b.desc()
        return np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,)).copy()


def interleave(names):
    """triangle i gets material names[i % len(names)]"""
    def assign(ids, m):
        for i, n in enumerate(names):
            ids[i::len(names)] = m[n]
    return assign


def mixed(gx, names, **kw):
    return MeshScene(gx, names, interleave(names), **kw)


METAL_GLASS = ("metal", "glass")


def render(gx, scene, split, w=W, h=H, spp=SPP, **kw):
    old = os.environ.pop(SWITCH, None)
    try:
        if not split:
            os.environ[SWITCH] = "1"   # read per render call
        return gx.PathIntegrator(DEPTH, 1.0, "spatial").Render(scene, w, h, spp, **kw)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def same(a, b):
    (ia, sa), (ib, sb) = a, b
    assert [sa[c] for c in COUNTS] == [sb[c] for c in COUNTS], ([sa[c] for c in COUNTS], [sb[c] for c in COUNTS])
    assert np.array_equal(ia, ib) and biteq(ia, ib)


def both_plans(gx, scene, more_launches, **kw):
    """split on == split off; returns the image"""
    on, off = render(gx, scene, True, **kw), render(gx, scene, False, **kw)
    same(on, off)
    assert on[1]["rays_closest"] > 0 and np.isfinite(on[0]).all() and on[0][..., :3].max() > 0
    if more_launches:
        assert on[1]["kernel_launches"] > off[1]["kernel_launches"], (on[1]["kernel_launches"], off[1]["kernel_launches"])
    else:
        assert on[1]["kernel_launches"] == off[1]["kernel_launches"], (on[1]["kernel_launches"], off[1]["kernel_launches"])
    return on[0]


# ---------------------------------------------------------------- CPU: the narrow kernels as compiled
def test_narrow_kernels_hold_three_waves_without_more_scratch(gx):
    """k_shade<LM_CONDUCTOR> and k_shade<LM_ROUGH_DIELECTRIC> for area lights exist in libgnxr.so, hold three waves per SIMD, and need no more
    scratch than k_shade<LM_GLOSSY> (tools/kernel_regs.py; profiles/kernel_regs_material_queues.txt is the report of this build)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = kernel_regs.kernels(gx.LIB_PATH)

    def one(lm):
        k = [k for k in ks if "k_shade<%du, 1, false, false>" % lm in k["name"]]
        assert len(k) == 1, (lm, k)
        return k[0]
    glossy = one(LM_GLOSSY)
    for lm in (LM_CONDUCTOR, LM_ROUGH_DIELECTRIC):
        k = one(lm)
        assert k["waves_per_simd"] >= 3 and k["scratch"] <= glossy["scratch"], (k, glossy)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_alternating_metal_and_glass(gpu):
    """metal and rough glass triangle by triangle: every wave of the shared glossy queue is mixed, the two queues' lengths are no multiples
    of 64; also a pipelined call (sub-passes of one sample, several in flight: the queues hold slots of several regions)"""
    scene = gpu.Scene(mixed(gpu, METAL_GLASS).b)
    both_plans(gpu, scene, True)
    one = render(gpu, scene, False, 48, 40, 7, samples_per_pass=7)
    for inflight in (1, 3, 8):
        on = render(gpu, scene, True, 48, 40, 7, samples_per_pass=1, passes_in_flight=inflight)
        assert on[1]["passes"] == 7 and on[1]["passes_in_flight"] == min(inflight, 7)
        same(on, one)
    both_plans(gpu, scene, True, w=48, h=40, spp=7, samples_per_pass=1, passes_in_flight=3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["metal", "glass"])
def test_one_kind_only(gpu, name):
    """an all-metal and an all-rough-glass mesh: the narrow kernel runs on the one glossy queue"""
    both_plans(gpu, gpu.Scene(mixed(gpu, (name,)).b), False)


@pytest.mark.gpu
def test_a_handful_of_metal_triangles(gpu):
    """five metal triangles among glass: the conductor queue is empty in most loop turns (launches with n == 0, the blocks' early exit)"""
    def assign(ids, m):
        ids[:] = m["glass"]
        ids[100:105] = m["metal"]
    both_plans(gpu, gpu.Scene(MeshScene(gpu, ("glass", "metal"), assign).b), True)


@pytest.mark.gpu
def test_four_queues_with_plastic(gpu):
    """metal + rough glass + Plastic: diffuse, conductor, rough dielectric and the shared glossy kernel for Plastic are four queues"""
    both_plans(gpu, gpu.Scene(mixed(gpu, ("metal", "glass", "plastic")).b), True)


@pytest.mark.gpu
def test_five_queues_fall_back(gpu):
    """metal + rough glass + Plastic + Disney would need five queues: today's plan"""
    both_plans(gpu, gpu.Scene(mixed(gpu, ("metal", "glass", "plastic", "disney")).b), False)


@pytest.mark.gpu
def test_environment_light_takes_the_fourth_queue(gpu):
    """metal + rough glass under an InfiniteAreaLight: the escape queue is the fourth output, the split applies (LT_AREA | LT_ENV kernels);
    with Plastic as well five queues would be needed: today's plan"""
    both_plans(gpu, gpu.Scene(mixed(gpu, METAL_GLASS, env=True).b), True)
    both_plans(gpu, gpu.Scene(mixed(gpu, ("metal", "glass", "plastic"), env=True).b), False)


@pytest.mark.gpu
def test_smooth_glass_is_no_kind(gpu):
    """smooth glass has specular lobes: kind 0, k_shade<LM_GLOSSY>; beside metal it keeps the shared kernel on a queue of its own"""
    both_plans(gpu, gpu.Scene(mixed(gpu, ("sglass",)).b), False)
    both_plans(gpu, gpu.Scene(mixed(gpu, ("sglass", "metal")).b), True)


@pytest.mark.gpu
def test_a_sphere_keeps_todays_plan(gpu):
    """sphere hits get their class from the traversal kernels, which know no kinds: one glossy queue"""
    both_plans(gpu, gpu.Scene(mixed(gpu, METAL_GLASS, sphere="metal").b), False)


@pytest.mark.gpu
def test_live_edits_move_triangles_between_the_queues(gpu):
    """update_materials turns the metal into rough glass and back, set_triangle_materials moves triangles between the two, then the BVH is
    rebuilt: after each step split on == split off == a fresh scene, and triangle_materials() still reports class 1"""
    ms = mixed(gpu, METAL_GLASS)
    b, m = ms.b, ms.m
    mesh = slice(ms.first, ms.first + ms.n)
    scene = gpu.Scene(b)
    mats0 = desc_materials(gpu, b)
    first = both_plans(gpu, scene, True)

    def check(more_launches, **fresh_kw):
        img = both_plans(gpu, scene, more_launches)
        fresh = fresh_scene(gpu, b, **fresh_kw)
        same(render(gpu, scene, True), render(gpu, fresh, True))
        assert (scene.triangle_materials()[1][mesh] == 1).all()
        return img

    # the metal record becomes a copy of the rough glass: one kind left
    as_glass = with_record(mats0, m["metal"], mats0[m["glass"]])
    scene.update_materials([as_glass[m["metal"]]], m["metal"])
    assert not biteq(check(False, materials=as_glass), first)
    scene.update_materials([mats0[m["metal"]]], m["metal"])
    assert biteq(check(True, materials=mats0), first)
    # triangles change sides: the first third all metal, the rest all glass
    ids = ms.ids()
    ids[ms.first:ms.first + ms.n // 3] = m["metal"]
    ids[ms.first + ms.n // 3:ms.first + ms.n] = m["glass"]
    scene.set_triangle_materials(ids)
    assert not biteq(check(True, tri_material=ids), first)
    scene.rebuild_bvh()
    check(True, tri_material=ids, split="hlbvh")
