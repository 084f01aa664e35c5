"""Development measurement (MI355X): the time of closest-point queries and of what they are compared with (not run by pytest).

    python tests/dev_closest_time.py [--n-tris 100000,1000000] [--log2-queries 20] [--reps 9] [--brute-queries 4096] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Query sets of 2^20 points:
  a   surface samples of the mesh jittered by 1 % of its extent, in random order (contact against a deforming mesh)
  b   the same points sorted by a 30-bit Morton key of their position (what binning inside the call would buy; the sort itself is timed
      separately as `morton_sort_ms`: key, torch.sort and gather on the device)
  c   uniform in the world bound, unbounded (distance-field sampling; far points keep more of the tree alive)
Per set: median / min / max of --reps event-bracketed timings of Scene.closest_point after a warm-up and ns per query, twice -- with the
call's own binning switched off (GNXR_CLOSEST_BIN_MIN: the walk in the order the queries arrive in) and as shipped (`binned`: key, radix
sort and permuted walk inside the call) -- and, in a run of their own through the counting instantiation, nodes visited and triangles
tested per query.
Yardsticks, timed in the same run: Scene.intersect on 2^20 rays from the points of (a) in random directions (one ray walk through the same
tree), and for scenes of at most 100 k triangles a chunked torch brute force over all triangles with the restatement's formula (dist2
alone, --brute-queries of the points of (a); checked against the call's dist2).  One JSON line per scene."""
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
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def runs_ms(fn, reps):
    timed(fn)
    ms = [timed(fn)[0] for _ in range(reps)]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def morton30(p, lo, hi):
    """30-bit Morton key of points (torch, on the device): 10 bits per axis over [lo, hi]"""
    g = ((p - lo) / (hi - lo) * 1023.0).clamp(0, 1023).to(torch.int64)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return spread(g[:, 0]) | (spread(g[:, 1]) << 1) | (spread(g[:, 2]) << 2)


def torch_dist2(a, b, c, q):
    """dist2 of the restatement (tests/closest_reference.py) in torch: queries (m, 1, 3) against triangles (1, t, 3)"""
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
    ab, ac, ap = b - a, c - a, q - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = q - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = q - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    denom = 1.0 / ((va + vb) + vc)
    p = (a + (vb * denom)[..., None] * ab) + (vc * denom)[..., None] * ac
    w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    p = torch.where(((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0))[..., None], b + w6[..., None] * (c - b), p)
    p = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + (d2 / (d2 - d6))[..., None] * ac, p)
    p = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c, p)
    p = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + (d1 / (d1 - d3))[..., None] * ab, p)
    p = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b, p)
    p = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a, p)
    lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)
    p = torch.where(p < lo, lo, torch.where(p > hi, hi, p))
    d = q - p
    return dot(d, d)


def measure(n_tris, n_queries, reps, brute_queries):
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32, copy=True)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int64, copy=True)
    scene = gx.Scene(b)
    need = scene.bvh4()[2]
    dev = torch.device("cuda", scene.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    tv, ti = torch.from_numpy(v).to(dev), torch.from_numpy(idx).to(dev)
    mesh_v = tv[: int(idx[:-12].max()) + 1]   # AddModel comes first: the mesh without the box
    extent = float((mesh_v.max(dim=0).values - mesh_v.min(dim=0).values).max())
    lo, hi = tv.min(dim=0).values, tv.max(dim=0).values
    tri = ti[torch.randint(0, len(idx) - 12, (n_queries,), device=dev, generator=gen)]
    u = torch.rand((n_queries, 2), device=dev, generator=gen)
    u = torch.where((u.sum(dim=1) > 1)[:, None], 1 - u, u)
    pa = tv[tri[:, 0]] + u[:, 0:1] * (tv[tri[:, 1]] - tv[tri[:, 0]]) + u[:, 1:2] * (tv[tri[:, 2]] - tv[tri[:, 0]])
    pa = (pa + (torch.rand((n_queries, 3), device=dev, generator=gen) * 2 - 1) * (0.01 * extent)).contiguous()

    def sort_by_morton():
        return pa[torch.sort(morton30(pa, lo, hi)).indices].contiguous()
    sort_ms = runs_ms(sort_by_morton, reps)
    sets = {"a_surface_random": pa, "b_surface_morton": sort_by_morton(),
            "c_uniform": (lo + torch.rand((n_queries, 3), device=dev, generator=gen) * (hi - lo)).contiguous()}
    out = torch.empty((n_queries, 8), device=dev)
    res = {"n_tris": scene.n_triangles, "n_queries": n_queries, "reps": reps, "stack4_need": need, "morton_sort_ms": sort_ms, "sets": {}}
    for name, pts in sets.items():
        q = torch.cat([pts, torch.full((n_queries, 1), float("inf"), device=dev)], dim=1).contiguous()
        os.environ["GNXR_CLOSEST_BIN_MIN"] = str(1 << 62)   # the walk in the order the queries arrive in
        r = runs_ms(lambda: scene.closest_point(q, out=out), reps)
        r["ns_per_query"] = r["median_ms"] * 1e6 / n_queries
        del os.environ["GNXR_CLOSEST_BIN_MIN"]                # the call as shipped: binned by Morton key inside
        r["binned"] = runs_ms(lambda: scene.closest_point(q, out=out), reps)
        r["binned"]["ns_per_query"] = r["binned"]["median_ms"] * 1e6 / n_queries
        r["caller_order_over_binned"] = r["median_ms"] / r["binned"]["median_ms"]
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        scene.closest_point(q, out=out, counts=counts)
        torch.cuda.synchronize()
        r["nodes_per_query"], r["tris_per_query"] = (float(x) / n_queries for x in counts.cpu())
        res["sets"][name] = r
    dirs = torch.randn((n_queries, 3), device=dev, generator=gen)
    rays = gx.rays_tensor(pa, dirs / dirs.norm(dim=1, keepdim=True))
    hits = torch.empty((n_queries, 8), device=dev)
    ray = runs_ms(lambda: scene.intersect(rays, out=hits), reps)
    ray["ns_per_ray"] = ray["median_ms"] * 1e6 / n_queries
    res["ray_walk"] = ray
    a_ms = res["sets"]["a_surface_random"]["median_ms"]
    res["a_over_ray_walk"] = a_ms / ray["median_ms"]
    res["a_binned_over_ray_walk"] = res["sets"]["a_surface_random"]["binned"]["median_ms"] / ray["median_ms"]
    res["a_over_b"] = a_ms / res["sets"]["b_surface_morton"]["median_ms"]
    res["a_over_b_plus_sort"] = a_ms / (res["sets"]["b_surface_morton"]["median_ms"] + sort_ms["median_ms"])
    if scene.n_triangles <= 110000 and brute_queries > 0:
        m = min(brute_queries, n_queries)
        ta, tb, tc = (tv[ti[:, k]][None] for k in range(3))

        def brute():
            best = torch.empty(m, device=dev)
            for s in range(0, m, 128):
                best[s:s + 128] = torch_dist2(ta, tb, tc, pa[s:s + 128, None]).nan_to_num(nan=float("inf")).min(dim=1).values
            return best
        br = runs_ms(brute, max(1, reps // 3))
        scene.closest_point(torch.cat([pa[:m], torch.full((m, 1), float("inf"), device=dev)], dim=1).contiguous(), out=out[:m])
        torch.cuda.synchronize()
        br["queries"] = m
        br["ns_per_query"] = br["median_ms"] * 1e6 / m
        br["max_abs_dist2_difference"] = float((brute() - out[:m, 1]).abs().max())   # (torch may fuse or reorder: not a bit comparison)
        br["brute_over_a_per_query"] = br["ns_per_query"] / res["sets"]["a_surface_random"]["ns_per_query"]
        res["torch_brute_force"] = br
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--brute-queries", type=int, default=4096)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 queries")
    a = ap.parse_args()
    gx.init(0)
    sizes, nq = ([5000], 1 << 14) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_queries)
    for n_tris in sizes:
        print(json.dumps(measure(n_tris, nq, a.reps, a.brute_queries)), flush=True)


if __name__ == "__main__":
    main()
