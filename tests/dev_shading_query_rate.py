"""Development measurement (MI355X): queries per second of Scene.bsdf beside Scene.intersect on the same rays (not run by pytest).

    python tests/dev_shading_query_rate.py [--reps 11] [--quick]

Workloads:
  zoo      the 8192 probes of tests/golden/bsdf_zoo.npz on the material zoo (one material of each kind), replicated to 2^24 rays
  camera   the 1920 x 1080 camera rays of sample 0 on the cfg 3 scene (Cornell box + the synthetic 100 k-triangle mesh, Glass + Metal),
           wi and u random
Per workload: Scene.intersect (k_trace4 + k_query_finish: the floor, the traversal is shared) and Scene.bsdf (k_trace4 + k_bsdf_query +
the three-column integer conversion of the Python layer) in one process; device events around each call on a synchronised stream after one
warm-up, median of --reps.  The per-kernel split comes from running this script under `rocprofv3 --kernel-trace --stats` (a run of its
own, with --quick).  One JSON line per workload."""
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
from dev_query_rate import camera_rays, event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--quick", action="store_true", help="2^20 zoo probes and 480 x 270 camera rays (for a profiler run)")
    a = ap.parse_args()
    gx.init(0)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bsdf_zoo.npz"))
    rep = (1 << (20 if a.quick else 24)) // len(g["rays"])
    zoo = [torch.from_numpy(np.tile(g[k], (rep, 1))).cuda() for k in ("rays", "wi", "u")]
    W, H = (480, 270) if a.quick else (1920, 1080)
    b3 = scenes.dragon_cornell(100000, "glass+metal")
    cam = torch.from_numpy(camera_rays(b3, W, H)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    wi = torch.nn.functional.normalize(torch.randn((cam.shape[0], 3), device="cuda", generator=gen), dim=1)
    u = torch.rand((cam.shape[0], 2), device="cuda", generator=gen)
    for name, b, (rays, wi_, u_) in (("zoo", scenes.material_zoo(), zoo), ("camera", b3, (cam, wi, u))):
        scene = gx.Scene(b)
        n = rays.shape[0]
        hits = torch.empty((n, 8), device="cuda")
        out = torch.empty((n, 16), device="cuda")
        t_hit = event_ms(lambda: scene.intersect(rays, out=hits), a.reps)
        t_bsdf = event_ms(lambda: scene.bsdf(rays, wi_, u_, out=out), a.reps)
        print(json.dumps({"workload": name, "n_rays": n, "intersect_ms": t_hit, "intersect_mrays_s": n / t_hit * 1e-3, "bsdf_ms": t_bsdf,
                          "bsdf_mqueries_s": n / t_bsdf * 1e-3, "bsdf_over_intersect": t_bsdf / t_hit,
                          "valid_fraction": float((out[:, 13] == 1).float().mean())}), flush=True)
        scene.close()


if __name__ == "__main__":
    main()
