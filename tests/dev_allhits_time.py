"""Development measurement (MI355X): the time of all-hits ray queries and of what they are compared with (not run by pytest).

    python tests/dev_allhits_time.py [--n-tris 100000,1000000] [--log2-rays 20] [--reps 9] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Ray sets of 2^20 rays from uniform origins
inside the world bound in random directions, in random order: `finite` with tmax = the scene's extent, `inf` with tmax = +inf.
Per set, median / min / max of --reps event-bracketed calls after a warm-up:
  a   Scene.all_hits with K = 1 against Scene.intersect on the same rays (the yardstick), with the nodes visited, own-box tests and
      triangle tests per ray of both K = 1 (the counting form) -- the walk never shrinks tmax, and the counters say what that costs
  b   K = 0, 8, 32 against K = 1: the price of the list and of the output traffic
  c   the same rays sorted by a 30-bit Morton key of their origin by the caller, and the sort itself (key, torch.sort, gather), which is
      what binning inside the call would have to beat
  d   Scene.contains and Scene.signed_distance on 2^20 points against their parts (count_hits on ready-made rays, closest_point)
The lists and counts of the first 4096 rays of every timed call are compared on bytes with a call on those 4096 rays alone.  One JSON
line per scene."""
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
from dev_closest_time import morton30, runs_ms  # noqa: E402


def same_as_small_batch(scene, rays, K, res, m=4096):
    """the first m rays of a timed call against a call on them alone: records and counts on bytes"""
    small = scene.all_hits(rays[:m].contiguous(), K)
    torch.cuda.synchronize()
    return bool(torch.equal(small.records.view(torch.int32), res.records[:m].view(torch.int32)) and torch.equal(small.count, res.count[:m]))


def measure(n_tris, n_rays, reps):
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32, copy=True)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    tv = torch.from_numpy(v).to(dev)
    lo, hi = tv.min(dim=0).values, tv.max(dim=0).values
    extent = float((hi - lo).max())
    o = (lo + torch.rand((n_rays, 3), device=dev, generator=gen) * (hi - lo)).contiguous()
    dirs = torch.randn((n_rays, 3), device=dev, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    res = {"n_tris": scene.n_triangles, "n_rays": n_rays, "reps": reps, "stack4_need": scene.bvh4()[2], "extent": extent, "sets": {}}

    def sort_by_morton(rays):
        return rays[torch.sort(morton30(rays[:, 0:3], lo, hi)).indices].contiguous()

    for name, tmax in (("finite", extent), ("inf", float("inf"))):
        rays = gx.rays_tensor(o, dirs, tmax)
        r = {}
        hits = torch.empty((n_rays, 8), device=dev)
        r["intersect"] = runs_ms(lambda: scene.intersect(rays, out=hits), reps)
        counts = torch.empty(n_rays, dtype=torch.int32, device=dev)
        ok = True
        for K in (1, 0, 8, 32):
            out = torch.empty((n_rays, K, 4), device=dev)
            r[f"K{K}"] = runs_ms(lambda: scene.all_hits(rays, K, out=out, counts_out=counts), reps)
            ok = ok and same_as_small_batch(scene, rays, K, scene.all_hits(rays, K, out=out, counts_out=counts))
        r["small_batch_same_bytes"] = ok
        r["mean_count"] = float(counts.float().mean())
        r["max_count"] = int(counts.max())
        r["K1_over_intersect"] = r["K1"]["median_ms"] / r["intersect"]["median_ms"]
        for K in (0, 8, 32):
            r[f"K{K}_over_K1"] = r[f"K{K}"]["median_ms"] / r["K1"]["median_ms"]
        work = torch.zeros(3, dtype=torch.int64, device=dev)
        scene.all_hits(rays, 1, counts=work)
        torch.cuda.synchronize()
        r["nodes_per_ray"], r["box_tests_per_ray"], r["tri_tests_per_ray"] = (float(x) / n_rays for x in work.cpu())
        # c: the caller sorts by a Morton key of the origin
        r["morton_sort"] = runs_ms(lambda: sort_by_morton(rays), reps)
        sorted_rays = sort_by_morton(rays)
        out = torch.empty((n_rays, 1, 4), device=dev)
        r["K1_morton_sorted"] = runs_ms(lambda: scene.all_hits(sorted_rays, 1, out=out, counts_out=counts), reps)
        r["caller_order_over_sorted"] = r["K1"]["median_ms"] / r["K1_morton_sorted"]["median_ms"]
        r["caller_order_over_sorted_plus_sort"] = r["K1"]["median_ms"] / (r["K1_morton_sorted"]["median_ms"] + r["morton_sort"]["median_ms"])
        res["sets"][name] = r
    # d: containment and signed distance, and their parts
    pts = o
    ready = gx.rays_tensor(pts, torch.tensor(gx.CONTAINS_DIRECTION, device=dev).expand(n_rays, 3).contiguous())
    q = torch.cat([pts, torch.full((n_rays, 1), float("inf"), device=dev)], dim=1).contiguous()
    res["contains"] = runs_ms(lambda: scene.contains(pts), reps)
    res["count_hits_ready_rays"] = runs_ms(lambda: scene.count_hits(ready), reps)
    res["signed_distance"] = runs_ms(lambda: scene.signed_distance(pts), reps)
    res["closest_point"] = runs_ms(lambda: scene.closest_point(q), reps)
    res["inside_fraction"] = float(scene.contains(pts).float().mean())
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-rays", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 rays")
    a = ap.parse_args()
    gx.init(0)
    sizes, nr = ([5000], 1 << 14) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_rays)
    for n_tris in sizes:
        print(json.dumps(measure(n_tris, nr, a.reps)), flush=True)


if __name__ == "__main__":
    main()
