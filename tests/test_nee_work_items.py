"""The traversal kernels' work list holds ONE item per light-sampling (NEE) vertex (TraceWork, csrc/trace_kernel.hip.h): the item's set-up
reads the flags of the vertex's shadow record, sets the shadow ray up and -- for the lanes whose vertex has one -- the MIS ray in a batch of
its own (k_trace4) or right after the shadow ray (k_trace).  A ray's result does not depend on the lane or the batch that carries it, so
every frame below must equal the oracle's (or the same samples through another plan) in image bits and in both ray counts.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first)

import oracle_lib as ol
import scenes

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 48, 40, 8, 5
RAY_KEYS = ("rays_closest", "rays_any")


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def emissive_box(gx):
    """A closed box around the camera whose six walls are area lights (12 DiffuseAreaLights facing inwards), with a matte box and a rough-glass
    ball on its floor.  A vertex has a MIS ray only when its BSDF sample hits the very triangle its light sample chose (estimate_direct_record,
    csrc/kernels.hip.h: lightPdf == 0 otherwise), so the box is a low, wide slab (80 x 2 x 86): from most points one ceiling or floor triangle fills
    most of the hemisphere, and the spatial light distribution chooses it.  63 % of the vertices with a shadow ray then have a MIS ray
    too (the tests print the share)."""
    x0, x1, y0, y1, z0, z1 = -40.0, 40.0, -1.0, 1.0, -40.0, 46.0
    b = gx.SceneBuilder()
    white = b.MatteMaterial(scenes.WHITE, 60.0)
    red = b.MatteMaterial(scenes.RED, 0.0)
    rough_glass = b.add_material(type=gx._abi.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.3, vrough=0.2)

    def wall(p, q, r, s):   # triangles (p q s), (q r s); the normal Cross(p0 - p2, p1 - p2) points into the box
        b.add_emissive_mesh(np.array([p, q, r, s], np.float32), np.array([[0, 1, 3], [1, 2, 3]], np.int32), white, (1.5, 1.2, 0.9), n_samples=1)

    A, B, C, D = (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)      # floor corners
    E, F, G, K = (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)      # ceiling corners
    wall(C, B, A, D)   # floor
    wall(G, K, E, F)   # ceiling
    wall(A, B, F, E)   # back
    wall(C, D, K, G)   # front (behind the camera)
    wall(D, A, E, K)   # left
    wall(B, C, G, F)   # right
    s = 0.4
    v, t = scenes.box_mesh((-2.0, y0, -1.5), (-0.5, y0 + 2.1 * s, 0.2))
    b.add_mesh(v, t, red)
    v, t, _, _ = scenes.uv_sphere_mesh((0.8, y0 + 1.2 * s, 1.2), 1.1 * s, 8, 12)
    b.add_mesh(v, t, rough_glass)
    return b


@pytest.fixture(scope="module")
def box_reference(gx):
    """the oracle's frame of the all-emissive box: rendered once, read by both kernels' tests"""
    b = emissive_box(gx)
    img, st = ol.OracleScene(b).render(gx.PathIntegrator(DEPTH, 1.0, "spatial"), W, H, SPP)
    img.setflags(write=False)
    return b, img, st


def against_oracle(gpu, b, oimg=None, ost=None, integ=None):
    integ = integ or gpu.PathIntegrator(DEPTH, 1.0, "spatial")
    if oimg is None:
        oimg, ost = ol.OracleScene(b).render(integ, W, H, SPP)
    img, st = integ.Render(gpu.Scene(b), W, H, SPP)
    print(f"device rays {st['rays_closest']}+{st['rays_any']} (MIS {st['rays_closest_nee']} = {st['rays_closest_nee'] / max(1, st['rays_any']):.3f} of the shadow rays)   "
          f"oracle {ost['rays_closest']}+{ost['rays_any']}")
    assert tuple(st[k] for k in RAY_KEYS) == tuple(ost[k] for k in RAY_KEYS)
    assert img[..., :3].any() and biteq(img[..., :3], oimg[..., :3])
    return st


def test_all_emissive_box_both_rays_per_vertex(gpu, box_reference):
    """Nearly every vertex item has a shadow ray and a MIS ray: a batch of 64 items yields more rays than the wave's 64-record queue holds,
    so the MIS rays go through the batch of their own"""
    b, oimg, ost = box_reference
    st = against_oracle(gpu, b, oimg, ost)
    assert 2 * st["rays_closest_nee"] > st["rays_any"], (st["rays_closest_nee"], st["rays_any"])


def test_plain_cornell_rare_mis_rays(gpu):
    st = against_oracle(gpu, scenes.cornell())
    assert 0 < st["rays_closest_nee"] < st["rays_any"] // 4


def test_delta_lights(gpu):
    """point / spot / distant lights: their vertices never have a MIS ray (Integrator.cpp:157-158)"""
    against_oracle(gpu, scenes.delta_cornell())


@pytest.mark.parametrize("size", [256, 640])
def test_multi_chunk_frame_against_single_sample_passes(gpu, size):
    """One frame of 16 spp through the default plan against the same samples as passes of one sample per pixel.
    256 x 256: launches of 1 - 2 M items on 5120 waves -- chunk_plan gives no 512-item chunks (big = 0), the whole list goes out through the
    cursor in 128- and 64-item chunks, which hold NEE items.
    640 x 640: 6.5 M paths per launch, above waves * 384 + 512 = 2.0 M items: 512-item chunks, then the step to 128- and to 64-item chunks
    inside the NEE range, as in the headline plan."""
    scene = gpu.Scene(scenes.dragon_cornell(2000, "glass+metal"))
    integ = gpu.PathIntegrator(8, 1.0, "spatial")
    img, st = integ.Render(scene, size, size, 16)
    ref, rst = integ.Render(scene, size, size, 16, samples_per_pass=1, passes_in_flight=1)
    print(f"default plan: passes={st['passes']} rays {st['rays_closest']}+{st['rays_any']}   1 spp per pass: passes={rst['passes']} rays {rst['rays_closest']}+{rst['rays_any']}")
    assert st["passes"] < rst["passes"] == 16
    assert size * size * 16 // st["passes"] > (5120 * 384 + 512 if size > 256 else 0)
    assert tuple(st[k] for k in RAY_KEYS + ("rays_closest_nee",)) == tuple(rst[k] for k in RAY_KEYS + ("rays_closest_nee",))
    assert st["rays_closest_nee"] > 0 and biteq(img, ref)


def test_all_emissive_box_on_the_binary_tree_kernel(gpu, box_reference):
    """the counting run walks the reference's binary tree with k_trace, which takes the same work list"""
    b, oimg, ost = box_reference
    try:
        gpu.lib().gnxr_set_profiling(2)
        st = against_oracle(gpu, b, oimg, ost)
    finally:
        gpu.lib().gnxr_set_profiling(0)
    assert st["nodes_visited"] > 0 and 2 * st["rays_closest_nee"] > st["rays_any"]
