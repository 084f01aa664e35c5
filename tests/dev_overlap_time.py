"""Development measurement (MI355X): the time of box overlap queries, beside the neighbour queries a caller had before, and of voxelize
(not run by pytest).

    python tests/dev_overlap_time.py [--n-tris 100000,1000000] [--log2-queries 20] [--log2-sweep 16] [--reps 11] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Boxes: cubes centred on 2^20 surface samples of
the mesh jittered by 1 % of its extent, in random order (tests/dev_near_time.py's generator and seed), with an edge of 1 and of 8 mean
triangle edge lengths.  Per size -- count_in_box, overlap_box at K = 8 and K = 32, the CSR form (both walks, the cumsum and the
allocation), and count_within / within at K = 8 and K = 32 on the same centres with the cube's half diagonal as radius, the only route
there was before -- one warm-up, then median / min / max of --reps synchronised calls, the mean counts, their ratio (what a caller
over-reported before) and, through the counting instantiation, nodes visited and triangles tested per query.
Sweep: on 2^--log2-sweep of the centres, cubes sized by bisection for a mean count of about 8, 64 and 512: count_in_box against the CSR form,
whose second walk pays the insertion into rows of that length.
voxelize: 128^3 and 256^3 over the mesh's bounds in the first scene, beside the time of count_in_box alone on the same boxes.
One JSON line per scene."""
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
from dev_closest_time import runs_ms  # noqa: E402


def cubes(centres, edge):
    boxes = torch.zeros((len(centres), 8), device=centres.device)
    boxes[:, 0:3] = centres - 0.5 * edge
    boxes[:, 4:7] = centres + 0.5 * edge
    return boxes


def edge_for_mean_count(scene, centres, target, hi):
    lo = 0.0
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if float(scene.count_in_box(cubes(centres, mid)).float().mean()) < target:
            lo = mid
        else:
            hi = mid
    return hi


def measure(n_tris, n_queries, n_sweep, reps, voxel_dims):
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32, copy=True)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int64, copy=True)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    tv, ti = torch.from_numpy(v).to(dev), torch.from_numpy(idx).to(dev)
    mesh_v = tv[: int(idx[:-12].max()) + 1]   # AddModel comes first: the mesh without the box
    lo, hi = mesh_v.min(dim=0).values, mesh_v.max(dim=0).values
    extent = float((hi - lo).max())
    mesh_t = ti[:-12]
    mean_edge = float(torch.cat([(tv[mesh_t[:, k]] - tv[mesh_t[:, (k + 1) % 3]]).norm(dim=1) for k in range(3)]).mean())
    tri = ti[torch.randint(0, len(idx) - 12, (n_queries,), device=dev, generator=gen)]
    u = torch.rand((n_queries, 2), device=dev, generator=gen)
    u = torch.where((u.sum(dim=1) > 1)[:, None], 1 - u, u)
    pa = tv[tri[:, 0]] + u[:, 0:1] * (tv[tri[:, 1]] - tv[tri[:, 0]]) + u[:, 1:2] * (tv[tri[:, 2]] - tv[tri[:, 0]])
    pa = (pa + (torch.rand((n_queries, 3), device=dev, generator=gen) * 2 - 1) * (0.01 * extent)).contiguous()
    res = {"n_tris": scene.n_triangles, "n_queries": n_queries, "reps": reps, "stack4_need": scene.bvh4()[2], "mean_edge": mean_edge, "mean_edge_over_extent": mean_edge / extent}

    cnt = torch.empty((n_queries,), dtype=torch.int32, device=dev)
    out8, out32 = torch.empty((n_queries, 8), dtype=torch.int32, device=dev), torch.empty((n_queries, 32), dtype=torch.int32, device=dev)
    for edges in (1, 8):
        boxes = cubes(pa, edges * mean_edge)
        ball = torch.cat([pa, torch.full((n_queries, 1), 0.5 * edges * mean_edge * 3 ** 0.5, device=dev)], dim=1).contiguous()
        calls = {"count_in_box": lambda **kw: scene.count_in_box(boxes, **kw),
                 "overlap_box_k8": lambda **kw: scene.overlap_box(boxes, None, 8, out=out8, counts_out=cnt, **kw),
                 "overlap_box_k32": lambda **kw: scene.overlap_box(boxes, None, 32, out=out32, counts_out=cnt, **kw),
                 "overlap_box_csr": lambda **kw: scene.overlap_box(boxes, counts_out=cnt, **kw),
                 "count_within": lambda **kw: scene.count_within(ball, None, **kw)}
        r = {}
        for name, call in calls.items():
            r[name] = runs_ms(call, reps)
            r[name]["ns_per_query"] = r[name]["median_ms"] * 1e6 / n_queries
            work = torch.zeros(2, dtype=torch.int64, device=dev)
            call(counts=work)
            torch.cuda.synchronize()
            r[name]["nodes_per_query"], r[name]["tris_per_query"] = (float(x) / n_queries for x in work.cpu())
        for K in (8, 32):   # their records are 32 bytes: (n, K, 8) floats
            records = torch.empty((n_queries, K, 8), device=dev)
            r[f"within_k{K}"] = runs_ms(lambda: scene.within(ball, None, K, out=records, counts_out=cnt), reps)
            del records
        r["mean_count_in_box"] = float(scene.count_in_box(boxes).float().mean())
        r["mean_count_within"] = float(scene.count_within(ball, None).float().mean())
        r["over_report"] = r["mean_count_within"] / max(r["mean_count_in_box"], 1e-30)
        res[f"edge_x{edges}"] = r

    sweep = pa[:n_sweep].contiguous()
    res["sweep_queries"] = n_sweep
    for target in (8, 64, 512):
        edge = edge_for_mean_count(scene, sweep[:4096].contiguous(), target, extent)
        boxes = cubes(sweep, edge)
        r = {"edge_over_mean_edge": edge / mean_edge, "mean_count": float(scene.count_in_box(boxes).float().mean()),
             "count_in_box": runs_ms(lambda: scene.count_in_box(boxes), reps), "overlap_box_csr": runs_ms(lambda: scene.overlap_box(boxes), reps)}
        r["fill_over_count"] = (r["overlap_box_csr"]["median_ms"] - r["count_in_box"]["median_ms"]) / r["count_in_box"]["median_ms"]
        res[f"csr_rows_{target}"] = r

    for n in voxel_dims:
        origin, cell = tuple(float(x) for x in lo), tuple(float(x) / n for x in (hi - lo))
        boxes = gx.voxel_boxes(origin, cell, (n, n, n), device=dev)
        chunks = [boxes[s:s + (1 << 22)] for s in range(0, len(boxes), 1 << 22)]
        r = {"voxelize": runs_ms(lambda: scene.voxelize(origin, cell, (n, n, n)), reps), "count_in_box_alone": runs_ms(lambda: [scene.count_in_box(c) for c in chunks], reps),
             "set": int(scene.voxelize(origin, cell, (n, n, n)).sum())}
        r["share_outside_the_walk"] = 1 - r["count_in_box_alone"]["median_ms"] / r["voxelize"]["median_ms"]
        r["ns_per_voxel"] = r["voxelize"]["median_ms"] * 1e6 / n ** 3
        res[f"voxelize_{n}"] = r
        del boxes, chunks
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--log2-sweep", type=int, default=16)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 queries, a 32^3 grid")
    a = ap.parse_args()
    gx.init(0)
    sizes, nq, ns = ([5000], 1 << 14, 1 << 12) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_queries, 1 << a.log2_sweep)
    for k, n_tris in enumerate(sizes):
        print(json.dumps(measure(n_tris, nq, ns, a.reps, ((32,) if a.quick else (128, 256)) if k == 0 else ())), flush=True)


if __name__ == "__main__":
    main()
