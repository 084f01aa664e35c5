"""Development measurement (MI355X): rays per second of the batched ray queries (not run by pytest).

    python tests/dev_query_rate.py [--sizes 100000 1000000] [--reps 5] [--quick]

Scenes: the cfg 3 scene (Cornell box + the synthetic mesh of that many triangles, Glass + Metal).  Workloads:
  random   2^24 incoherent rays (tests/scenes.py random_rays: origins uniform in the box, uniform directions, tmax = inf), closest hit
  camera   the 1920 x 1080 camera rays of sample 0 (gnxr_camera_rays), closest hit
  ao       one ambient-occlusion ray per camera-ray hit: from the hit point (offset along the normal that faces the camera), cosine-
           distributed about that normal, tmax = 0.25 (a tenth of the box's half width), any hit
Paths, all on the same rays:
  device   Scene.intersect / Scene.occluded: k_trace4 in its query mode (+ k_query_finish for closest hits), rays and results in
           device memory
  binary   the same device call on a scene created with GNXR_BINARY_BVH: k_trace_closest_api / k_trace_any_api, the reference's binary
           walk, one ray per lane, on the same device buffers
  host     Scene.Intersect / Scene.IntersectP: gnxr_trace_closest / gnxr_trace_any from host memory, their copies and allocations included
Call time: device events around each call on a synchronised stream (median of --reps after one warm-up); host path: host clock around the
synchronous call.  Kernel time is not taken here: run the script under `rocprofv3 --kernel-trace --stats` for it (a separate run).
One JSON line per scene and workload."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def event_ms(fn, reps):
    """median milliseconds between two device events around fn() on the current stream (after one warm-up call)"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def host_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def camera_rays(b, W, H):
    px, py = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    o, d = gx.camera_rays(b.desc().camera, W, H, px.reshape(-1), py.reshape(-1), np.zeros(W * H, np.int64))
    return gx.make_rays(o, d)


def ao_rays(rays, hits, seed=1, radius=0.25):
    """torch: one cosine-distributed occlusion ray per hit of `rays` (a RayHits of Scene.intersect)"""
    m = hits.prim >= 0
    o, d = rays[m, 0:3], rays[m, 4:7]
    n = hits.n[m]
    n = torch.where(((n * d).sum(1, keepdim=True) > 0), -n, n)       # the side the ray came from
    p = o + hits.t[m, None] * d + 1e-4 * n
    g = torch.Generator(device=rays.device).manual_seed(seed)
    u1, u2 = torch.rand(p.shape[0], device=rays.device, generator=g), torch.rand(p.shape[0], device=rays.device, generator=g)
    r, phi = torch.sqrt(u1), 2 * np.pi * u2
    a = torch.where(n[:, 0:1].abs() > 0.9, torch.tensor([[0.0, 1.0, 0.0]], device=rays.device), torch.tensor([[1.0, 0.0, 0.0]], device=rays.device))
    t1 = torch.nn.functional.normalize(torch.cross(a, n, dim=1), dim=1)
    t2 = torch.cross(n, t1, dim=1)
    w = (r * torch.cos(phi))[:, None] * t1 + (r * torch.sin(phi))[:, None] * t2 + torch.sqrt(1 - u1)[:, None] * n
    return gx.rays_tensor(p, w, radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="2^20 random rays and 480 x 270 camera rays (for a profiler run)")
    a = ap.parse_args()
    gx.init(0)
    n_random = 1 << (20 if a.quick else 24)
    W, H = (480, 270) if a.quick else (1920, 1080)
    for n_tris in a.sizes:
        b = scenes.dragon_cornell(n_tris, "glass+metal")
        wide = gx.Scene(b)
        os.environ["GNXR_BINARY_BVH"] = "1"
        try:
            binary = gx.Scene(b)
        finally:
            del os.environ["GNXR_BINARY_BVH"]
        cam = torch.from_numpy(camera_rays(b, W, H)).cuda()
        first = wide.intersect(cam)
        work = {"random": (torch.from_numpy(scenes.random_rays(n_random, seed=3)).cuda(), False),
                "camera": (cam, False),
                "ao": (ao_rays(cam, first), True)}
        torch.cuda.synchronize()
        for name, (rays, any_hit) in work.items():
            n = rays.shape[0]
            host = rays.cpu().numpy()
            out = {"n_tris": n_tris, "workload": name, "n_rays": n, "query": "any" if any_hit else "closest"}
            res = {}
            for path, s in (("device", wide), ("binary", binary)):
                buf = torch.empty(n, dtype=torch.uint8, device="cuda") if any_hit else torch.empty((n, 8), dtype=torch.float32, device="cuda")
                fn = (lambda s=s, buf=buf: s.occluded(rays, out=buf)) if any_hit else (lambda s=s, buf=buf: s.intersect(rays, out=buf))
                ms = event_ms(fn, a.reps)
                res[path] = buf.cpu().numpy()
                out[path + "_ms"] = ms
                out[path + "_mrays_s"] = n / ms * 1e-3
            hfn = (lambda: wide.IntersectP(host)) if any_hit else (lambda: wide.Intersect(host))
            ms = host_ms(hfn, max(1, a.reps // 2))
            out["host_ms"] = ms
            out["host_mrays_s"] = n / ms * 1e-3
            out["device_equals_binary"] = bool((res["device"].view(np.uint32 if not any_hit else np.uint8) ==
                                                res["binary"].view(np.uint32 if not any_hit else np.uint8)).all())
            out["hit_fraction"] = float((res["device"] != 0).mean() if any_hit else (res["device"][:, 0].view(np.int32) >= 0).mean())
            print(json.dumps(out), flush=True)
        wide.close()
        binary.close()


if __name__ == "__main__":
    main()
