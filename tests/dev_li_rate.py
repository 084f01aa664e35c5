"""Development measurement (MI355X): the rate of PathIntegrator.Li on caller rays against the render of the same samples (not run by pytest).

    python tests/dev_li_rate.py [--n-tris 100000] [--spp-range 8] [--reps 5] [--quick]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial"), HaltonSampler(1024)) at 1920 x 1080.
Work: samples [0, --spp-range) of every pixel -- 8 by default, 16.6 M paths.
  li      PathIntegrator.Li over the camera rays of those samples (gnxr_camera_rays) and their gnxr_li_sample records, in device memory
          (rays 32 B and records 16 B per path in, 16 B of L out)
  render  PathIntegrator.RenderDevice over the same samples (spp_begin = 0, spp_end = --spp-range) into a device image
Call time: device events around each call on the current stream, the two alternating, median of --reps after one warm-up of each.
Rays per second count every ray traced (rays_closest + rays_any of the call's stats).  `identical`: the Li results summed in sample order
and divided by spp equal the render's image bit for bit.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--spp-range", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="480 x 270 (for a profiler run)")
    a = ap.parse_args()
    gx.init(0)
    W, H = (480, 270) if a.quick else (1920, 1080)
    spp, k = 1024, a.spp_range
    b = scenes.dragon_cornell(a.n_tris, "glass+metal")
    scene = gx.Scene(b)
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    s, py, px = (v.reshape(-1) for v in np.meshgrid(np.arange(k), np.arange(H), np.arange(W), indexing="ij"))
    o, d = gx.camera_rays(b.desc().camera, W, H, px, py, s)
    rays = torch.from_numpy(gx.make_rays(o, d)).cuda()
    samples = gx.li_samples(torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda(), torch.from_numpy(s).cuda())
    del o, d, px, py, s
    n = rays.shape[0]
    L = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    run_li = lambda: integ.Li(scene, rays, samples, W, H, spp, out=L)[1]
    run_render = lambda: integ.RenderDevice(scene, img.data_ptr(), W, H, spp, stream=stream.cuda_stream, spp_begin=0, spp_end=k)
    timed(run_li)
    timed(run_render)
    t_li, t_r = [], []
    for _ in range(a.reps):
        ms, st_li = timed(run_li)
        t_li.append(ms)
        ms, st_r = timed(run_render)
        t_r.append(ms)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    Lv = L.view(k, H, W, 4)
    for j in range(k):
        acc += Lv[j, :, :, :3]
    res = acc / np.float32(spp)
    identical = bool((res.view(torch.int32) == img[..., :3].contiguous().view(torch.int32)).all().item())
    rays_li = st_li["rays_closest"] + st_li["rays_any"]
    rays_r = st_r["rays_closest"] + st_r["rays_any"]
    ms_li, ms_r = statistics.median(t_li), statistics.median(t_r)
    out = {"n_tris": a.n_tris, "width": W, "height": H, "samples": k, "paths": n,
           "li_ms": ms_li, "render_ms": ms_r, "li_mrays_s": rays_li / ms_li * 1e-3, "render_mrays_s": rays_r / ms_r * 1e-3,
           "ratio": (rays_li / ms_li) / (rays_r / ms_r), "same_ray_counts": rays_li == rays_r, "identical": identical,
           "li_ms_all": t_li, "render_ms_all": t_r, "passes_in_flight": st_li["passes_in_flight"], "loop_iterations_li": st_li["loop_iterations"],
           "loop_iterations_render": st_r["loop_iterations"]}
    print(json.dumps(out), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
