"""Development measurement (MI355X): the time of a lightmap bake and of its parts (not run by pytest).

    python tests/dev_bake_time.py [--n-tris 100000] [--size 1024] [--spp 64] [--dilate 2] [--samples-per-pass 0] [--reps 3] [--quick]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")).  Atlas: a generated grid of square
charts, two triangles each, over all triangles of the scene (tests/bake_reference.py: grid_atlas) at --size x --size.
  bake        PathIntegrator.BakeLightmap: the whole call; `bake_li_ms` is the part of it its Li sub-batches report (stats: seconds_render),
              `bake_around_li_ms` the rest: rasterisation, the list of covered texels, ray generation, the ordered sums, dilation, and
              the host's turn-around between sub-batches
  the parts, through the layered calls on the same records (covered texels x spp, sample-major):
  rasterise   bake_texels
  raygen      surface_rays over all records in one call
  li          PathIntegrator.Li over those rays in one call: gnxr_li_device alone on the same number of rays
  reduce      the ordered sum over the samples, / spp * pi (torch, one add per sample)
  dilate      bake_dilate
Call time: device events around each call on the current stream, median of --reps after one warm-up.  `identical`: the image the parts
give equals the bake bit for bit.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bake_reference as br  # noqa: E402
import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def median_ms(fn, reps):
    timed(fn)
    runs = [timed(fn) for _ in range(reps)]
    return statistics.median(ms for ms, _ in runs), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--samples-per-pass", type=int, default=0, help="paths per sub-batch of the bake (0: the library's choice); the parts always run as one call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="256 x 256 x 8 spp")
    a = ap.parse_args()
    gx.init(0)
    W = H = 256 if a.quick else a.size
    spp = 8 if a.quick else a.spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    nt = scene.n_triangles
    uv = torch.from_numpy(br.grid_atlas(nt, max(1, math.ceil(math.sqrt((nt + 1) // 2))))).cuda()

    timed(lambda: integ.BakeLightmap(scene, uv, W, H, spp, dilate=a.dilate, samples_per_pass=a.samples_per_pass))
    runs = sorted((timed(lambda: integ.BakeLightmap(scene, uv, W, H, spp, dilate=a.dilate, samples_per_pass=a.samples_per_pass)) for _ in range(a.reps)), key=lambda r: r[0])
    ms_bake, (img, st) = runs[len(runs) // 2]   # the median run, with its own stats

    ms_raster, (tri, bary) = median_ms(lambda: gx.bake_texels(scene, uv, W, H), a.reps)
    texel = torch.nonzero(tri.reshape(-1) >= 0).reshape(-1)
    n_cov = texel.shape[0]
    t = tri.reshape(-1)[texel].repeat(spp).contiguous()
    bb = bary.reshape(-1, 2)[texel].repeat(spp, 1).contiguous()
    px = (texel % W).to(torch.int32).repeat(spp).contiguous()
    py = (texel // W).to(torch.int32).repeat(spp).contiguous()
    s = torch.arange(spp, device="cuda", dtype=torch.int32).repeat_interleave(n_cov).contiguous()
    n = t.shape[0]
    out = (torch.empty((n, 8), device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda"), torch.empty((n, 8), device="cuda"))
    ms_rays, (rays, samples, _) = median_ms(lambda: gx.surface_rays(scene, t, bb, px, py, s, W, H, out=out), a.reps)
    L = torch.empty((n, 4), device="cuda")
    ms_li, (_, st_li) = median_ms(lambda: integ.Li(scene, rays, samples, W, H, spp, out=L), a.reps)

    def reduce():
        acc = torch.zeros((n_cov, 3), device="cuda")
        Lv = L.view(spp, n_cov, 4)
        for j in range(spp):
            acc += Lv[j, :, :3]
        res = torch.zeros((H * W, 4), device="cuda")
        res[texel, :3] = (acc / np.float32(spp)) * float(br.PI)
        res[texel, 3] = 1
        return res.view(H, W, 4)

    ms_reduce, flat = median_ms(reduce, a.reps)
    ms_dilate, parts = median_ms(lambda: gx.bake_dilate(flat, a.dilate), a.reps)
    identical = bool((parts.view(torch.int32) == img.view(torch.int32)).all().item())
    bake_li_ms = st["seconds_render"] * 1e3
    print(json.dumps({"n_tris": nt, "width": W, "height": H, "spp": spp, "dilate": a.dilate, "samples_per_pass": a.samples_per_pass, "bake_sub_batches": st["passes"], "covered_texels": n_cov, "paths": n,
                      "bake_ms": ms_bake, "bake_li_ms": bake_li_ms, "bake_around_li_ms": ms_bake - bake_li_ms, "bake_around_li_share": (ms_bake - bake_li_ms) / ms_bake,
                      "rasterise_ms": ms_raster, "raygen_ms": ms_rays, "li_ms": ms_li, "reduce_ms": ms_reduce, "dilate_ms": ms_dilate,
                      "bake_over_li": ms_bake / ms_li, "bake_mrays_s": (st["rays_closest"] + st["rays_any"]) / ms_bake * 1e-3,
                      "li_mrays_s": (st_li["rays_closest"] + st_li["rays_any"]) / ms_li * 1e-3, "same_ray_counts": st["rays_closest"] + st["rays_any"] == st_li["rays_closest"] + st_li["rays_any"],
                      "identical": identical}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
