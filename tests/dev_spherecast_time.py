"""Development measurement (MI355X): the time of sphere casts against intersect and closest_point from the same origins (not run by pytest).

    python tests/dev_spherecast_time.py [--n-tris 100000,1000000] [--log2-casts 20] [--reps 9] [--quick]

Scenes: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal) at each triangle count.  Casts: tests/dev_closest_time.py's set (a) as
origins, 2^20 surface samples of the mesh jittered by 1 % of its extent, in random order (the same generator and seed), with uniformly
random unit directions and tmax = +inf, at radius 0 and at a radius of one mean edge length of the mesh.
Per call -- sphere_cast at each radius, intersect along the same rays and closest_point at the same origins (in caller order, like the
casts, and as shipped, binned) -- median / min / max of --reps event-bracketed timings after a warm-up, all in one run; the casts as a
ratio to intersect and to closest_point; the share of casts that hit and that start in contact; and, in a run of its own through the
counting instantiation, nodes visited and triangles taken to the analytic step per cast.  One JSON line per scene."""
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


def measure(n_tris, n_casts, reps):
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
    tri = ti[torch.randint(0, len(idx) - 12, (n_casts,), device=dev, generator=gen)]
    u = torch.rand((n_casts, 2), device=dev, generator=gen)
    u = torch.where((u.sum(dim=1) > 1)[:, None], 1 - u, u)
    pa = tv[tri[:, 0]] + u[:, 0:1] * (tv[tri[:, 1]] - tv[tri[:, 0]]) + u[:, 1:2] * (tv[tri[:, 2]] - tv[tri[:, 0]])
    pa = (pa + (torch.rand((n_casts, 3), device=dev, generator=gen) * 2 - 1) * (0.01 * extent)).contiguous()
    dirs = torch.randn((n_casts, 3), device=dev, generator=gen)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    mt = ti[:-12]
    edge = float(torch.cat([(tv[mt[:, 1]] - tv[mt[:, 0]]).norm(dim=1), (tv[mt[:, 2]] - tv[mt[:, 1]]).norm(dim=1), (tv[mt[:, 0]] - tv[mt[:, 2]]).norm(dim=1)]).mean())

    inf = torch.full((n_casts, 1), float("inf"), device=dev)
    casts = {name: torch.cat([pa, torch.full((n_casts, 1), r, device=dev), dirs, inf], dim=1).contiguous() for name, r in (("cast_r0", 0.0), ("cast_edge", edge))}
    rays = torch.cat([pa, inf, dirs, torch.zeros((n_casts, 1), device=dev)], dim=1).contiguous()
    points = torch.cat([pa, inf], dim=1).contiguous()
    res = {"n_tris": scene.n_triangles, "n_casts": n_casts, "reps": reps, "stack4_need": scene.bvh4()[2], "mean_edge": edge, "mean_edge_over_extent": edge / extent}
    out = torch.empty((n_casts, 8), device=dev)
    res["intersect"] = runs_ms(lambda: scene.intersect(rays, out=out), reps)
    os.environ["GNXR_CLOSEST_BIN_MIN"] = str(1 << 62)   # the walk in the order the queries arrive in, as the casts run
    res["closest_point_caller_order"] = runs_ms(lambda: scene.closest_point(points, out=out), reps)
    del os.environ["GNXR_CLOSEST_BIN_MIN"]
    res["closest_point"] = runs_ms(lambda: scene.closest_point(points, out=out), reps)
    for name, c in casts.items():
        r = runs_ms(lambda: scene.sphere_cast(c, None, None, out=out), reps)
        r["ns_per_cast"] = r["median_ms"] * 1e6 / n_casts
        for base in ("intersect", "closest_point", "closest_point_caller_order"):
            r["over_" + base] = r["median_ms"] / res[base]["median_ms"]
        work = torch.zeros(2, dtype=torch.int64, device=dev)
        got = scene.sphere_cast(c, None, None, out=out, counts=work)
        torch.cuda.synchronize()
        r["nodes_per_cast"], r["tris_per_cast"] = (float(x) / n_casts for x in work.cpu())
        r["hit_share"] = float((got.prim >= 0).float().mean())
        r["start_in_contact_share"] = float(((got.prim >= 0) & (got.t == 0)).float().mean())
        res[name] = r
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", default="100000,1000000")
    ap.add_argument("--log2-casts", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 2^14 casts")
    a = ap.parse_args()
    gx.init(0)
    sizes, n = ([5000], 1 << 14) if a.quick else ([int(x) for x in a.n_tris.split(",")], 1 << a.log2_casts)
    for n_tris in sizes:
        print(json.dumps(measure(n_tris, n, a.reps)), flush=True)


if __name__ == "__main__":
    main()
