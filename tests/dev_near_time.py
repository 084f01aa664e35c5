"""Development measurement (MI355X): the time of neighbour queries against closest_point on the same points (not run by pytest).

    python tests/dev_near_time.py [--n-tris 100000,1000000] [--log2-queries 20] [--reps 9] [--sample 4096] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Queries: tests/dev_closest_time.py's set (a), 2^20
surface samples of the mesh jittered by 1 % of its extent, in random order (the same generator and seed).  The radius is chosen so that the
mean number of triangles within it is about 8 on the first --sample queries, by bisection over the 64 smallest dist2 per query of a
chunked torch brute force over all triangles (the restatement's formula, dev_closest_time.torch_dist2); the device's own mean count on
the sample is printed beside it.
Per call -- within at K = 8 and count_within at that radius, nearest at K = 1 and K = 8 unbounded, nearest at K = 8 inside that radius
(within's lists at the NEAREST mode's price) -- median / min / max of --reps
event-bracketed timings after a warm-up, twice: with the call's own binning switched off (GNXR_CLOSEST_BIN_MIN) and as shipped
(`binned`), each as a ratio to closest_point timed the same way in the same run, and, in a run of their own through the counting
instantiation, nodes visited and triangles tested per query.  One JSON line per scene."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402
from dev_closest_time import runs_ms, torch_dist2  # noqa: E402


def smallest_dist2(tv, ti, pts, keep=64, chunk=16):
    """the `keep` smallest dist2 of each point against all triangles, ascending (torch, on the device; NaN counts as far)"""
    a, b, c = (tv[ti[:, k]][None] for k in range(3))
    out = torch.empty((len(pts), keep), device=pts.device)
    for s in range(0, len(pts), chunk):
        d2 = torch_dist2(a, b, c, pts[s:s + chunk, None]).nan_to_num(nan=float("inf"))
        out[s:s + chunk] = torch.topk(d2, keep, dim=1, largest=False).values
    return out


def radius_for_mean_count(d2, target):
    lo, hi = 0.0, float(d2[:, -1].sqrt().max())
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if float((d2 <= float(np.float32(mid) * np.float32(mid))).sum(dim=1).float().mean()) < target:
            lo = mid
        else:
            hi = mid
    return hi


def measure(n_tris, n_queries, reps, sample):
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32, copy=True)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int64, copy=True)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    tv, ti = torch.from_numpy(v).to(dev), torch.from_numpy(idx).to(dev)
    mesh_v = tv[: int(idx[:-12].max()) + 1]   # AddModel comes first: the mesh without the box
    extent = float((mesh_v.max(dim=0).values - mesh_v.min(dim=0).values).max())
    tri = ti[torch.randint(0, len(idx) - 12, (n_queries,), device=dev, generator=gen)]
    u = torch.rand((n_queries, 2), device=dev, generator=gen)
    u = torch.where((u.sum(dim=1) > 1)[:, None], 1 - u, u)
    pa = tv[tri[:, 0]] + u[:, 0:1] * (tv[tri[:, 1]] - tv[tri[:, 0]]) + u[:, 1:2] * (tv[tri[:, 2]] - tv[tri[:, 0]])
    pa = (pa + (torch.rand((n_queries, 3), device=dev, generator=gen) * 2 - 1) * (0.01 * extent)).contiguous()

    m = min(sample, n_queries)
    radius = radius_for_mean_count(smallest_dist2(tv, ti, pa[:m]), 8.0)
    free = torch.cat([pa, torch.full((n_queries, 1), float("inf"), device=dev)], dim=1).contiguous()
    ball = torch.cat([pa, torch.full((n_queries, 1), radius, device=dev)], dim=1).contiguous()
    res = {"n_tris": scene.n_triangles, "n_queries": n_queries, "reps": reps, "stack4_need": scene.bvh4()[2], "radius": radius, "radius_over_extent": radius / extent,
           "sample": m, "sample_mean_count_device": float(scene.count_within(ball[:m].contiguous(), None).float().mean())}
    out1, out8 = torch.empty((n_queries, 8), device=dev), torch.empty((n_queries, 8, 8), device=dev)
    out_k1 = torch.empty((n_queries, 1, 8), device=dev)
    cnt = torch.empty((n_queries,), dtype=torch.int32, device=dev)
    calls = {"closest_point": lambda **kw: scene.closest_point(free, out=out1, **kw),
             "within_k8": lambda **kw: scene.within(ball, None, 8, out=out8, counts_out=cnt, **kw),
             "count_within": lambda **kw: scene.count_within(ball, None, **kw),
             "nearest_k1": lambda **kw: scene.nearest(free, 1, out=out_k1, counts_out=cnt, **kw),
             "nearest_k8": lambda **kw: scene.nearest(free, 8, out=out8, counts_out=cnt, **kw),
             "nearest_k8_in_radius": lambda **kw: scene.nearest(ball, 8, out=out8, counts_out=cnt, **kw)}
    for name, call in calls.items():
        os.environ["GNXR_CLOSEST_BIN_MIN"] = str(1 << 62)   # the walk in the order the queries arrive in
        r = runs_ms(call, reps)
        del os.environ["GNXR_CLOSEST_BIN_MIN"]                # the call as shipped: binned by Morton key inside
        r["binned"] = runs_ms(call, reps)
        for x in (r, r["binned"]):
            x["ns_per_query"] = x["median_ms"] * 1e6 / n_queries
        work = torch.zeros(2, dtype=torch.int64, device=dev)
        call(counts=work)
        torch.cuda.synchronize()
        r["nodes_per_query"], r["tris_per_query"] = (float(x) / n_queries for x in work.cpu())
        res[name] = r
    base = res["closest_point"]
    for name in calls:
        res[name]["over_closest_point"] = res[name]["median_ms"] / base["median_ms"]
        res[name]["binned"]["over_closest_point"] = res[name]["binned"]["median_ms"] / base["binned"]["median_ms"]
    res["mean_count_within"] = float(scene.count_within(ball, None).float().mean())
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 queries")
    a = ap.parse_args()
    gx.init(0)
    sizes, nq = ([5000], 1 << 14) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_queries)
    for n_tris in sizes:
        print(json.dumps(measure(n_tris, nq, a.reps, a.sample)), flush=True)


if __name__ == "__main__":
    main()
