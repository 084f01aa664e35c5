"""Development measurement (MI355X): the fused feature-buffer call against the composition a caller had to write before it, and against
the beauty pass at the same shape (not run by pytest).

    python tests/dev_aov_rate.py [--n-tris 100000] [--reps 7]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal).  Shapes: one 1920 x 1080 frame at 16 spp, and 64 views of 256 x 256 on a
circle around the box at 4 spp.  Per shape, alternating --reps times after one warm-up each, medians of device-event times:
  fused_all / fused_depth   integrator.RenderAOV with every channel / with depth alone
  composed                  per view and sample camera_rays_device + Scene.intersect, then a torch sum over the samples in order and the
                            division by spp, for depth and normal (albedo and the shading normal cannot be composed at all); the rays and
                            hits of one view's samples are resident at a time: 64 bytes per camera sample + the pixel indices
  views                     integrator.RenderViews (PathIntegrator(8, 1.0, "spatial")) at the same shape: the beauty pass
Rates are camera samples per second.  resident bytes: stats["state_bytes"] of the fused call; for the composition the tensors it holds.
`identical`: the fused depth and normal carry the bits of the composed ones.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    gx.init(0)
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    ring = lambda V: [dict(eye=(5.0 * math.sin(2 * math.pi * v / V), 0.0, 5.0 * math.cos(2 * math.pi * v / V)), look=(0, 0, 0), up=(0, 1, 0), fov=90.0) for v in range(V)]
    out = {"n_tris": a.n_tris, "reps": a.reps, "shapes": []}
    for V, W, H, spp in ((1, 1920, 1080, 16), (64, 256, 256, 4)):
        cams = [gx.camera(**c) for c in ring(V)]
        n = W * H
        py, px = torch.meshgrid(torch.arange(H, dtype=torch.int32, device="cuda"), torch.arange(W, dtype=torch.int32, device="cuda"), indexing="ij")
        px, py = px.reshape(-1).contiguous(), py.reshape(-1).contiguous()
        s_all = torch.arange(spp, dtype=torch.int32, device="cuda").repeat_interleave(n).contiguous()   # sample-major, as the fused call
        pxs, pys = px.repeat(spp).contiguous(), py.repeat(spp).contiguous()
        c_depth = torch.zeros((V, H, W), dtype=torch.float32, device="cuda")
        c_normal = torch.zeros((V, H, W, 4), dtype=torch.float32, device="cuda")
        hits_buf = torch.empty((n * spp, 8), dtype=torch.float32, device="cuda")
        composed_bytes = n * spp * (32 + 32 + 16) + 3 * n * spp * 4   # rays, hits, sample records of camera_rays_device, px / py / s

        def run_composed():
            for v in range(V):
                rays, _ = gx.camera_rays_device(cams[v], W, H, pxs, pys, s_all)
                hits = scene.intersect(rays, out=hits_buf).hits.view(spp, n, 8)
                acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
                for s in range(spp):
                    acc = acc + torch.cat([hits[s, :, 5:8], hits[s, :, 1:2]], 1)
                acc = acc / float(spp)
                c_depth[v] = acc[:, 3].view(H, W)
                c_normal[v, ..., :3] = acc[:, :3].view(H, W, 3)

        full = {}

        def run_all():
            r, st = integ.RenderAOV(scene, W, H, spp, cameras=cams)
            full.update(r)
            return st

        run_depth = lambda: integ.RenderAOV(scene, W, H, spp, cameras=cams, channels=("depth",))[1]
        integ.Reserve(scene, W, H, spp)
        beauty = torch.zeros((V, H, W, 4), dtype=torch.float32, device="cuda")
        run_views = lambda: integ.RenderViews(scene, cams, W, H, spp, out=beauty)[1]
        arms = {"fused_all": run_all, "fused_depth": run_depth, "composed": run_composed, "views": run_views}
        ms = {k: [] for k in arms}
        st = {}
        for k, fn in arms.items():
            timed(fn)
        for _ in range(a.reps):
            for k, fn in arms.items():
                t, st[k] = timed(fn)
                ms[k].append(t)
        torch.cuda.synchronize()
        identical = bool((full["depth"].view(torch.int32) == c_depth.view(torch.int32)).all().item()) and \
            bool((full["normal"].view(torch.int32) == c_normal.view(torch.int32)).all().item()) and bool(c_depth.any().item())
        med = {k: statistics.median(v) for k, v in ms.items()}
        samples = V * n * spp
        out["shapes"].append({"views": V, "width": W, "height": H, "spp": spp, "camera_samples": samples,
                              **{k + "_ms": v for k, v in med.items()}, **{k + "_msamples_s": samples / v * 1e-3 for k, v in med.items()},
                              "fused_all_state_bytes": st["fused_all"]["state_bytes"], "fused_depth_state_bytes": st["fused_depth"]["state_bytes"],
                              "fused_all_passes": st["fused_all"]["passes"], "composed_resident_bytes": composed_bytes,
                              "fused_all_over_composed": med["fused_all"] / med["composed"], "fused_all_over_views": med["fused_all"] / med["views"],
                              "identical": identical, "ms_all": ms})
        del hits_buf, beauty, c_depth, c_normal, full
    print(json.dumps(out), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
