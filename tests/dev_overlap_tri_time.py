"""Development measurement (MI355X): the time of triangle overlap queries, beside the box queries on the same triangles' bounds -- the
route a caller had before (not run by pytest).

    python tests/dev_overlap_tri_time.py [--n-tris 100000,1000000] [--log2-queries 20] [--reps 11] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Query sets:
  (a) 2^--log2-queries triangles of the scene's own mesh (authoring order, repeated until there are that many) under a small rigid
      motion -- a rotation of 0.02 rad about y through the mesh's centre and a shift of one mean edge length --, in mesh order and in
      random order;
  (b) self_intersections of the scene at rest;
  (c) self_intersections after a sine deformation of the mesh through update_vertices (amplitude 2 % of its extent, 12 periods across).
Per set -- the count-only form, K = 8 and the CSR form (both walks, the cumsum and the allocation), and beside them count_in_box /
overlap_box on the queries' bounds [qlo, qhi], which visit the same nodes -- one warm-up, then median / min / max of --reps synchronised
calls; the mean counts and their ratio (what a caller over-reported before); through the counting instantiation, nodes visited and
triangles taken to the bounds test per query.  For (b) and (c) the boxes are the scene's triangles' in authoring order (the SELF call
walks them in leaf order), and the box count holds the triangle itself and its neighbours, which the skip rule leaves out.
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


def bounds_of(tris):
    """the gnxr_box_query records [qlo, qhi] of (n, 12) triangle records"""
    c = tris.view(-1, 3, 4)[:, :, 0:3]
    boxes = torch.zeros((len(tris), 8), device=tris.device)
    boxes[:, 0:3] = c.min(dim=1).values
    boxes[:, 4:7] = c.max(dim=1).values
    return boxes


def timed_set(scene, n, reps, exact, box):
    """exact(K, **kw), box(K, **kw): the two routes over the same n queries; K = 0, 8 or None"""
    dev = torch.device("cuda", scene.device)
    r = {}
    for route, call in (("tri", exact), ("box", box)):
        for form, K in (("count", 0), ("k8", 8), ("csr", None)):
            t = runs_ms(lambda: call(K), reps)
            t["ns_per_query"] = t["median_ms"] * 1e6 / n
            r[f"{route}_{form}"] = t
        work = torch.zeros(2, dtype=torch.int64, device=dev)
        count = call(0, counts=work).count
        torch.cuda.synchronize()
        r[f"{route}_nodes_per_query"], r[f"{route}_tris_per_query"] = (float(x) / n for x in work.cpu())
        r[f"{route}_mean_count"] = float(count.float().mean())
        r[f"{route}_share_nonzero"] = float((count > 0).float().mean())
    for form in ("count", "k8", "csr"):
        r[f"tri_over_box_{form}"] = r[f"tri_{form}"]["median_ms"] / r[f"box_{form}"]["median_ms"]
    r["over_report"] = r["box_mean_count"] / max(r["tri_mean_count"], 1e-30)
    return r


def measure(n_tris, n_queries, reps):
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32, copy=True)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int64, copy=True)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    tv, ti = torch.from_numpy(v).to(dev), torch.from_numpy(idx).to(dev)
    n_mesh_v = int(idx[:-12].max()) + 1   # AddModel comes first: the mesh without the box
    mesh_v, mesh_t = tv[:n_mesh_v], ti[:-12]
    lo, hi = mesh_v.min(dim=0).values, mesh_v.max(dim=0).values
    extent = float((hi - lo).max())
    mean_edge = float(torch.cat([(tv[mesh_t[:, k]] - tv[mesh_t[:, (k + 1) % 3]]).norm(dim=1) for k in range(3)]).mean())
    res = {"n_tris": scene.n_triangles, "n_queries": n_queries, "reps": reps, "stack4_need": scene.bvh4()[2], "mean_edge": mean_edge, "mean_edge_over_extent": mean_edge / extent}

    # (a) the mesh against a slightly moved copy of itself
    ca, sa = float(np.cos(0.02)), float(np.sin(0.02))
    rot = torch.tensor([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]], device=dev)
    ctr = 0.5 * (lo + hi)
    moved = ((mesh_v - ctr) @ rot.T + ctr + torch.tensor([mean_edge, 0, 0], device=dev)).contiguous()
    order = torch.arange(n_queries, device=dev) % len(mesh_t)
    for name, o in (("moved_mesh_order", order), ("moved_random_order", order[torch.randperm(n_queries, device=dev, generator=gen)])):
        tris = gx.triangle_queries(moved, mesh_t[o].contiguous())
        boxes = bounds_of(tris)
        res[name] = timed_set(scene, n_queries, reps, lambda K, **kw: scene.overlap_triangles(tris, K, **kw), lambda K, **kw: scene.overlap_box(boxes, None, K, **kw))
        del tris, boxes
    res["random_over_mesh_order_count"] = res["moved_random_order"]["tri_count"]["median_ms"] / res["moved_mesh_order"]["tri_count"]["median_ms"]

    # (b), (c) the scene against itself, at rest and folded
    nt = scene.n_triangles
    for name in ("self_at_rest", "self_deformed"):
        if name == "self_deformed":
            bent = (mesh_v + 0.02 * extent * torch.sin((12 * 2 * np.pi / extent) * mesh_v[:, [1, 2, 0]])).contiguous()
            scene.update_vertices(bent)
            tv = torch.cat([bent, tv[n_mesh_v:]])
        boxes = bounds_of(gx.triangle_queries(tv, ti))
        r = timed_set(scene, nt, reps, lambda K, **kw: scene.self_intersections(K, **kw), lambda K, **kw: scene.overlap_box(boxes, None, K, **kw))
        r["pairs"] = runs_ms(lambda: scene.self_intersections(pairs=True), reps)
        r["n_pairs"] = int(scene.self_intersections(pairs=True).shape[0])
        res[name] = r
        del boxes
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 queries")
    a = ap.parse_args()
    gx.init(0)
    sizes, nq = ([5000], 1 << 14) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_queries)
    for n_tris in sizes:
        print(json.dumps(measure(n_tris, nq, a.reps)), flush=True)


if __name__ == "__main__":
    main()
