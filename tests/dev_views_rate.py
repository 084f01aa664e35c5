"""Development measurement (MI355X): V views in one gnxr_render_views_device call against V x (gnxr_scene_set_camera + gnxr_render_device)
(not run by pytest).

    python tests/dev_views_rate.py [--n-tris 100000] [--views 64] [--sizes 128,512] [--spp 16] [--reps 7]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")), V cameras on a circle around the box,
all looking at its centre.  Per size (square images of that edge, --spp samples per pixel):
  sequential  V x (Scene.set_camera + RenderDevice into image v of one device tensor): the only way without the views call
  batched     one RenderViews into a second tensor of the same shape
Both arms run in this process after gnxr_render_reserve and one warm-up each; they alternate --reps times and the medians are reported:
device events on the current stream around each arm, and wall clock.  Rays per second count every ray traced (rays_closest + rays_any
of the stats).  `identical`: the two tensors hold the same bits.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    st = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    gx.init(0)
    V, spp = a.views, a.spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    ring = [dict(eye=(5.0 * math.sin(2 * math.pi * v / V), 0.0, 5.0 * math.cos(2 * math.pi * v / V)), look=(0, 0, 0), up=(0, 1, 0), fov=90.0) for v in range(V)]
    cams = [gx.camera(**c) for c in ring]
    stream = torch.cuda.current_stream()
    out = {"n_tris": a.n_tris, "views": V, "spp": spp, "reps": a.reps, "sizes": []}
    for size in (int(s) for s in a.sizes.split(",")):
        W = H = size
        seq = torch.zeros((V, H, W, 4), dtype=torch.float32, device="cuda")
        bat = torch.zeros((V, H, W, 4), dtype=torch.float32, device="cuda")
        integ.Reserve(scene, W, H, spp)

        def run_sequential():
            rays = 0
            for v in range(V):
                scene.set_camera(**ring[v])
                st = integ.RenderDevice(scene, seq[v].data_ptr(), W, H, spp, stream=stream.cuda_stream)
                rays += st["rays_closest"] + st["rays_any"]
            return rays

        def run_batched():
            st = integ.RenderViews(scene, cams, W, H, spp, out=bat)[1]
            return st["rays_closest"] + st["rays_any"]

        timed(run_sequential)
        timed(run_batched)
        ev_a, ev_b, wall_a, wall_b = [], [], [], []
        for _ in range(a.reps):
            ms, wall, rays_a = timed(run_sequential)
            ev_a.append(ms); wall_a.append(wall)
            ms, wall, rays_b = timed(run_batched)
            ev_b.append(ms); wall_b.append(wall)
        torch.cuda.synchronize()
        identical = bool((seq.view(torch.int32) == bat.view(torch.int32)).all().item()) and bool(seq[..., :3].any().item())
        ma, mb = statistics.median(ev_a), statistics.median(ev_b)
        out["sizes"].append({"width": W, "height": H, "paths": V * W * H * spp, "sequential_ms": ma, "batched_ms": mb, "ratio": mb / ma,
                             "sequential_wall_ms": statistics.median(wall_a), "batched_wall_ms": statistics.median(wall_b),
                             "wall_ratio": statistics.median(wall_b) / statistics.median(wall_a),
                             "sequential_mrays_s": rays_a / ma * 1e-3, "batched_mrays_s": rays_b / mb * 1e-3, "same_ray_counts": rays_a == rays_b,
                             "identical": identical, "sequential_ms_all": ev_a, "batched_ms_all": ev_b})
        del seq, bat
    print(json.dumps(out), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
