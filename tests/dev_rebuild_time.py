"""gnxr_scene_rebuild_bvh against gnxr_scene_create with HLBVH over the same vertices (dev tool, MI355X):

    python tests/dev_rebuild_time.py [--calls 7]

The synthetic mesh in the Cornell box at 100 k and 1 M triangles, its mesh vertices deformed once (gnxr_scene_update_vertices).  Per size,
in this one process: the median wall time of `--calls` Scene.rebuild_bvh() calls after one warm-up call (the call returns when every
device holds the new tree, so the host clock around it is synchronised), and the median of as many gnxr_scene_create calls with HLBVH on
a description carrying the same vertices, after one warm-up: the way to the same tree without this entry point."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401
import gnxraytracer_amd as gx, scenes
import test_scene_update as tsu

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=7)
args = ap.parse_args()
assert args.calls >= 5
gx.init(0)
for n in (100000, 1000000):
    b = scenes.dragon_cornell(n, "glass+metal")
    nv = tsu.model_vertex_count(gx, scenes.synthetic_mesh_path(n))
    v2 = tsu.deform(tsu.vertices(b), nv, seed=5, amount=0.02)
    scene = gx.Scene(b)                      # SAH, as callers create it
    scene.update_vertices(v2[:nv])
    t_re = []
    for k in range(args.calls + 1):
        torch.cuda.synchronize()
        t = time.perf_counter(); scene.rebuild_bvh(); torch.cuda.synchronize(); t_re.append(time.perf_counter() - t)
    b.set_bvh_split_method("hlbvh")
    d = tsu.Deformed(b, v2)
    t_cr = []
    for k in range(args.calls + 1):
        torch.cuda.synchronize()
        t = time.perf_counter(); fresh = gx.Scene(d.desc()); torch.cuda.synchronize(); t_cr.append(time.perf_counter() - t)
        if k < args.calls:
            del fresh
    same = all((x == y).all() for x, y in zip(scene.bvh()[1:], fresh.bvh()[1:])) and (scene.bvh4()[0] == fresh.bvh4()[0]).all()
    re_ms, cr_ms = statistics.median(t_re[1:]) * 1e3, statistics.median(t_cr[1:]) * 1e3
    print(f"{scene.n_triangles} triangles: rebuild_bvh {re_ms:.2f} ms (min {min(t_re[1:]) * 1e3:.2f}), gnxr_scene_create hlbvh {cr_ms:.2f} ms "
          f"(min {min(t_cr[1:]) * 1e3:.2f}), median of {args.calls} after 1 warm-up; same tree: {same}", flush=True)
    del scene, fresh
