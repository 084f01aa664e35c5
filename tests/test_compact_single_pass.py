"""The single-pass queue compaction (k_compact, csrc/compact_kernel.hip.h) at the shapes the small frames of the other tests do not reach: a
queue that spans more tiles than the compaction grid has blocks, so that every block takes several tickets and looks back over tiles of
earlier rounds.  Each case renders the same samples twice -- once through the default plan, once as single-region passes whose queues fit in
a few tiles -- and asks for identical image bits and ray counts: the order-preserving binning may not depend on how a queue is cut into tiles.
"""
import math
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first)

import scenes
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _constant(name, header):
    """a constexpr integer of the library's sources (the C ABI exports neither the tile size nor the CU count)"""
    text = open(os.path.join(ROOT, "gnxraytracer_amd", "csrc", header)).read()
    m = re.search(r"\b" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return int(eval(m.group(1).replace("ll", ""), {}))   # "64 << 20", "512", ...


# the smallest square frame whose 2-spp passes still fill a few (<= 8) tiles: W * H = 4 tiles
W = H = math.isqrt(4 * _constant("kCompactBlock", "compact_kernel.hip.h") * _constant("kCompactChunks", "compact_kernel.hip.h")) // 16 * 16


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def tile_entries():
    return _constant("kCompactBlock", "compact_kernel.hip.h") * _constant("kCompactChunks", "compact_kernel.hip.h")


def grid_blocks():
    return torch.cuda.get_device_properties(0).multi_processor_count * _constant("kCompactBlocksPerCu", "compact_kernel.hip.h")


def sub_pass_spp():
    """samples per pixel of an automatic sub-pass of the PathIntegrator at W x H"""
    return _constant("kSubPassPaths", "api_render.hip.h") // (W * H)


def both_plans(integ, scene, spp, small, **kw):
    img, st = integ.Render(scene, W, H, spp, **kw)
    ref, rst = integ.Render(scene, W, H, spp, samples_per_pass=small, passes_in_flight=1, **kw)
    print(f"default plan: passes={st['passes']} in flight={st['passes_in_flight']}  rays {st['rays_closest']}+{st['rays_any']}   "
          f"{small} spp per pass: passes={rst['passes']}  rays {rst['rays_closest']}+{rst['rays_any']}")
    assert (st["rays_closest"], st["rays_any"]) == (rst["rays_closest"], rst["rays_any"])
    assert biteq(img, ref)
    return st, rst


def test_cfg3_queue_spans_more_tiles_than_blocks(gpu):
    """cfg 3's scene, three automatic sub-passes (the last one partial) with several regions alive, against passes of 2 spp."""
    k = sub_pass_spp()
    first_bounce = W * H * k   # the queue of a sub-pass's camera rays
    assert first_bounce > tile_entries() * grid_blocks() and first_bounce > 2 * tile_entries(), (first_bounce, tile_entries(), grid_blocks())
    scene = gpu.Scene(scenes.dragon_cornell(100000, "glass+metal"))
    st, rst = both_plans(gpu.PathIntegrator(8, 1.0, "spatial"), scene, 2 * k + 64, 2)
    assert st["passes"] == 3 and st["passes_in_flight"] > 1
    assert W * H * 2 <= 8 * tile_entries() and rst["passes_in_flight"] == 1


def test_cfg4_style_four_class_queues(gpu):
    """Environment light + the material zoo: four class outputs (the escape queue) and the forked shade streams."""
    k = sub_pass_spp()
    scene = gpu.Scene(scenes.dragon_cornell(100000, "zoo", env=scenes.synthetic_env_path(1000, 500)))
    st, _ = both_plans(gpu.PathIntegrator(8, 1.0, "spatial"), scene, k + 64, 2)
    assert st["passes"] == 2 and st["passes_in_flight"] > 1


def test_volpath_host_counts_and_state_binning(gpu):
    """A small VolPath render: counts on the host, binning by path state, one pass against passes of one sample."""
    scene = gpu.Scene(scenes.volume_cornell())
    integ = gpu.VolPathIntegrator(8, 1.0, "spatial")
    img, st = integ.Render(scene, W, H, 8)
    ref, rst = integ.Render(scene, W, H, 8, samples_per_pass=1)
    assert st["passes"] == 1 and rst["passes"] == 8
    assert W * H * 8 > 2 * tile_entries()
    assert (st["rays_closest"], st["rays_any"]) == (rst["rays_closest"], rst["rays_any"])
    assert biteq(img, ref)
