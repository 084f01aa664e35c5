"""Development measurement (MI355X): the time of a light-probe bake and of its parts (not run by pytest).

    python tests/dev_lightprobe_time.py [--n-tris 100000] [--grid 16] [--spp 1024] [--samples-per-pass 0] [--reps 5] [--quick]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")).  Probes: a --grid^3 lattice over
[-2, 2]^3 inside the box (16^3 = 4096), --spp samples each.
  bake        PathIntegrator.BakeLightProbes: the whole call; `bake_li_ms` is the part of it its Li sub-batches report (stats:
              seconds_render), `bake_around_li_ms` the rest: ray generation, the projection, the scaling, and the host's turn-around
              between sub-batches
  the parts, through the layered calls on the same records (probes x spp, probe-major):
  raygen      lightprobe_rays over all records in one call
  li          PathIntegrator.Li over those rays in one call: gnxr_li_device alone on the same rays
  project     sh_project over all records in one call; `project_gb_s`: the bytes it reads (32 per ray, of which it needs 16, + 16 per L)
              over its time
  copy        a plain device-to-device copy of the projection's two input arrays (it reads the same bytes and writes them too);
              `project_over_copy` compares the two
Call time: device events around each call on the current stream after one warm-up; median, minimum and maximum of --reps runs.
`identical`: the coefficients the parts give equal the bake bit for bit.  One JSON line."""
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
import lightprobe_reference as lr  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def runs_ms(fn, reps):
    """(median, [min, max], the last result) of `reps` timed calls after one warm-up"""
    timed(fn)
    runs = [timed(fn) for _ in range(reps)]
    ms = [r[0] for r in runs]
    return statistics.median(ms), [min(ms), max(ms)], runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--samples-per-pass", type=int, default=0, help="paths per sub-batch of the bake (0: the library's choice); the parts always run as one call")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="4^3 probes x 128 spp")
    a = ap.parse_args()
    gx.init(0)
    g = 4 if a.quick else a.grid
    spp = 128 if a.quick else a.spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    axis = np.linspace(-2, 2, g, dtype=np.float32)
    pos_np = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = torch.from_numpy(np.ascontiguousarray(pos_np)).cuda()
    n_probes = pos.shape[0]
    W = min(n_probes, 1024)
    H = -(-n_probes // W)

    bake = lambda: integ.BakeLightProbes(scene, pos, spp, samples_per_pass=a.samples_per_pass)
    timed(bake)
    runs = sorted((timed(bake) for _ in range(a.reps)), key=lambda r: r[0])
    ms_bake, (sh, st) = runs[len(runs) // 2]   # the median run, with its own stats
    bake_spread = [runs[0][0], runs[-1][0]]

    k = torch.arange(n_probes, device="cuda", dtype=torch.int32).repeat_interleave(spp).contiguous()
    s = torch.arange(spp, device="cuda", dtype=torch.int32).repeat(n_probes).contiguous()
    px, py = (k % W).contiguous(), (k // W).contiguous()
    p = pos.repeat_interleave(spp, dim=0).contiguous()
    n = k.shape[0]
    out = (torch.empty((n, 8), device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda"))
    ms_rays, rays_spread, (rays, samples) = runs_ms(lambda: gx.lightprobe_rays(scene, p, px, py, s, W, H, out=out), a.reps)
    L = torch.empty((n, 4), device="cuda")
    ms_li, li_spread, (_, st_li) = runs_ms(lambda: integ.Li(scene, rays, samples, W, H, spp, out=L), a.reps)
    sums = torch.empty((n_probes, 9, 4), device="cuda")
    ms_proj, proj_spread, _ = runs_ms(lambda: gx.sh_project(rays, L, n_probes, out=sums), a.reps)
    rays2, L2 = torch.empty_like(rays), torch.empty_like(L)
    ms_copy, copy_spread, _ = runs_ms(lambda: (rays2.copy_(rays), L2.copy_(L)), a.reps)
    parts = (sums * torch.tensor(lr.FOUR_PI, device="cuda")) / torch.tensor(np.float32(spp), device="cuda")
    identical = bool((parts.view(torch.int32) == sh.view(torch.int32)).all().item())
    bake_li_ms = st["seconds_render"] * 1e3
    in_bytes = n * 48
    print(json.dumps({"n_tris": scene.n_triangles, "probes": n_probes, "spp": spp, "paths": n, "samples_per_pass": a.samples_per_pass, "bake_sub_batches": st["passes"], "reps": a.reps,
                      "bake_ms": ms_bake, "bake_ms_min_max": bake_spread, "bake_li_ms": bake_li_ms, "bake_around_li_ms": ms_bake - bake_li_ms,
                      "bake_around_li_share": (ms_bake - bake_li_ms) / ms_bake,
                      "raygen_ms": ms_rays, "raygen_ms_min_max": rays_spread, "li_ms": ms_li, "li_ms_min_max": li_spread,
                      "project_ms": ms_proj, "project_ms_min_max": proj_spread, "project_gb_s": in_bytes / ms_proj * 1e-6,
                      "copy_ms": ms_copy, "copy_ms_min_max": copy_spread, "copy_gb_s_read": in_bytes / ms_copy * 1e-6, "project_over_copy": ms_proj / ms_copy,
                      "bake_over_li": ms_bake / ms_li, "identical": identical}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
