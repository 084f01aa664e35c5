"""Light estimates added inside the traversal launch (k_trace4's set-up batches, csrc/trace4_kernel.hip.h) or by the sweep after it
(k_nee_combine, csrc/trace_kernel.hip.h): both call nee_apply, a vertex is added by exactly one of them (byte 3 of its nee_vis word), and
L += beta * Ld is the same statement wherever it runs.  So every frame below must be the same in image bits and ray counts with the default
library and with GNXR_NO_TRACE_NEE_APPLY=1 (all by sweep, the parent's behaviour), and equal the oracle's where tests/test_nee_work_items.py
compares to it.  The two counters of gnxr_scene_nee_apply_counts must sum to the number of queued NEE vertices -- what the sweep counts when
it does them all -- and the in-trace one is 0 with the switch set.

Which vertices the traversal kernel can reach follows from the hand-out plan of a launch (chunk_plan): a wave adds a vertex kNeeLag = 128
items after it set it up, inside the chunk it owns, so only the 512-item chunks of launches above waves * 384 items have any.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first)

import oracle_lib as ol
import scenes
from conftest import GOLDEN
from test_nee_work_items import DEPTH, H, RAY_KEYS, SPP, W, biteq, emissive_box

pytestmark = pytest.mark.gpu

SWITCH = "GNXR_NO_TRACE_NEE_APPLY"
COUNTS = RAY_KEYS + ("rays_closest_nee", "camera_samples")
# the multi-chunk frame: four sub-passes of 8 spp in flight (3.3 M paths each: launches of 10 - 16 M items on 5120 waves, i.e. several 512-item
# chunks per wave, then the 128- and 64-item chunks of the tail), 34 spp = four whole sub-passes and a ragged one of 2 spp
BIG = dict(w=640, h=640, spp=34, samples_per_pass=8, passes_in_flight=4)


def render(gx, scene, off, depth=DEPTH, w=W, h=H, spp=SPP, **kw):
    """one render with the switch set or unset (it is read per render call); returns (image, stats, (in trace, by sweep))"""
    old = os.environ.pop(SWITCH, None)
    try:
        if off:
            os.environ[SWITCH] = "1"
        img, st = gx.PathIntegrator(depth, 1.0, "spatial").Render(scene, w, h, spp, **kw)
        return img, st, scene.nee_apply_counts()
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def both_routes(gx, b, oracle=False, **kw):
    """the frame with the in-trace route and with the sweep alone: same bits, same counts, every queued vertex added once"""
    scene = gx.Scene(b)
    img, st, (in_trace, by_sweep) = render(gx, scene, False, **kw)
    ref, rst, (off_trace, queued) = render(gx, scene, True, **kw)
    print(f"NEE vertices queued {queued}: in trace {in_trace} ({in_trace / max(1, queued):.3f}), by sweep {by_sweep};   rays {st['rays_closest']}+{st['rays_any']} "
          f"(MIS {st['rays_closest_nee']})")
    assert off_trace == 0
    # with the switch set the sweep adds, and counts, every entry of every launch's NEE queue: between the vertices with a shadow ray and
    # the vertices with either ray
    assert rst["rays_any"] <= queued <= rst["rays_any"] + rst["rays_closest_nee"] and queued > 0
    assert in_trace + by_sweep == queued, (in_trace, by_sweep, queued)
    assert tuple(st[k] for k in COUNTS) == tuple(rst[k] for k in COUNTS)
    assert biteq(img, ref)
    if oracle:
        assert not kw   # the oracle's frame is the small default one
        oimg, ost = ol.OracleScene(b).render(gx.PathIntegrator(DEPTH, 1.0, "spatial"), W, H, SPP)
        assert tuple(st[k] for k in RAY_KEYS) == tuple(ost[k] for k in RAY_KEYS)
        assert img[..., :3].any() and biteq(img[..., :3], oimg[..., :3])
    return img, st, in_trace, queued


def test_all_emissive_box_both_rays_per_vertex(gpu):
    """63 % of the vertices have a shadow ray and a MIS ray: both done bits must be there before a vertex is added"""
    img, st, in_trace, queued = both_routes(gpu, emissive_box(gpu), oracle=True)
    assert 2 * st["rays_closest_nee"] > st["rays_any"]


def test_plain_cornell(gpu):
    both_routes(gpu, scenes.cornell(), oracle=True)


def test_delta_lights_no_mis_ray_anywhere(gpu):
    img, st, in_trace, queued = both_routes(gpu, scenes.delta_cornell(), oracle=True)


def test_environment_light_mis_rays_that_expect_a_miss(gpu):
    """the open Cornell box under an InfiniteAreaLight: a vertex that samples it gets a MIS ray that expects to hit nothing"""
    b = scenes.cornell()
    b.AddInfLight(os.path.join(GOLDEN, "env_100x50.hdr"))
    img, st, in_trace, queued = both_routes(gpu, b)
    plain = gpu.PathIntegrator(DEPTH, 1.0, "spatial").Render(gpu.Scene(scenes.cornell()), W, H, SPP)[1]
    print(f"MIS rays with the environment light {st['rays_closest_nee']}, without {plain['rays_closest_nee']}")
    assert st["rays_closest_nee"] > plain["rays_closest_nee"] and np.isfinite(img).all() and img[..., :3].max() > 0


def test_thin_frame_has_no_chunk_longer_than_the_lag(gpu):
    """48 x 40 x 8 spp: launches of at most 31 k items on 5120 waves go out in 128- and 64-item chunks (chunk_plan: big = 0), none of which
    has an item 128 behind another: everything is left to the sweep"""
    img, st, in_trace, queued = both_routes(gpu, scenes.cornell())
    assert W * H * SPP * 2 < 5120 * 384 and in_trace == 0


def test_multi_chunk_frame_with_tail_and_ragged_last_sub_pass(gpu):
    img, st, in_trace, queued = both_routes(gpu, scenes.dragon_cornell(2000, "glass+metal"), depth=8, **BIG)
    assert st["passes"] == 5 and st["passes_in_flight"] == 4
    assert BIG["w"] * BIG["h"] * BIG["samples_per_pass"] * 3 > 5120 * (384 + 2 * 512)   # three sub-passes alive already make several 512-item chunks per wave
    assert in_trace > 0 and np.isfinite(img).all()


def test_non_finite_beta_is_added_not_skipped(gpu):
    """A Lambertian box of reflectance 1e20: beta is infinite from the second bounce on, k_shade says so in bit 7 of the record's flags, and a
    vertex whose rays both fail (a slab under the light shadows the floor) must still run L += beta * (0 / pdf) = NaN as the reference
    does -- on both routes, hence in a frame whose launches have 512-item chunks."""
    b = gpu.SceneBuilder()
    hot = b.MatteMaterial((1e20, 1e20, 1e20), 0.0)
    b.AddCornell(hot, hot, hot)
    b.AddAreaLight(hot)
    v, t = scenes.box_mesh((-1.6, 0.2, -1.6), (1.6, 0.5, 1.6))
    b.add_mesh(v, t, hot)
    img, st, in_trace, queued = both_routes(gpu, b, depth=8, **BIG)
    assert in_trace > 0
    assert np.isnan(img[..., :3]).any(), "no path of this frame took the branch the case is about"
