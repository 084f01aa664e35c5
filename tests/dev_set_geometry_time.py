"""gnxr_scene_set_geometry against its floor and against what a caller did without it (dev tool, MI355X):

    python tests/dev_set_geometry_time.py [--calls 7]

The 100 k-triangle synthetic mesh in the Cornell box (cfg 3), its mesh vertices deformed differently for every call.  In this one process,
after one warm-up round, `--calls` rounds run the three arms one after the other (alternating, so that drift reaches all alike); each
figure is the median wall time of an arm's calls, the host clock around work that ends synchronised:

  set_geometry   Scene.set_geometry from device tensors (vertices, indices and every per-triangle array already on the device)
  rebuild_bvh    Scene.rebuild_bvh alone on the same scene: the floor, the shared pipeline without the new front pass and commit
  recreate       what a caller does without the entry point: the arrays copied to the host, Scene.close() and a new Scene with HLBVH
                 (which compiles materials, lights and sampler tables again and uploads everything)

The last scene of the first and the third arm must hold the same tree."""
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
import test_set_geometry as tsg

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--triangles", type=int, default=100000)
args = ap.parse_args()
assert args.calls >= 7
gx.init(0)
b = scenes.dragon_cornell(args.triangles, "glass+metal")
nv = tsu.model_vertex_count(gx, scenes.synthetic_mesh_path(args.triangles))
g = tsg.geometry_of(b)
rounds = args.calls + 1
meshes = []   # per round: the geometry on the device, vertices deformed with the round's seed
for k in range(rounds):
    gk = dict(g)
    gk["vertices"] = tsu.deform(g["vertices"], nv, seed=100 + k, amount=0.02)
    meshes.append(tsg.on_device(gk, 0))
scene = gx.Scene(b)            # SAH, as callers create it
other = gx.Scene(b)            # the handle the third arm replaces
torch.cuda.synchronize()
t_set, t_re, t_new = [], [], []
for k in range(rounds):
    m = meshes[k]
    torch.cuda.synchronize()
    t = time.perf_counter(); scene.set_geometry(**m); torch.cuda.synchronize(); t_set.append(time.perf_counter() - t)
    t = time.perf_counter(); scene.rebuild_bvh(); torch.cuda.synchronize(); t_re.append(time.perf_counter() - t)
    t = time.perf_counter()
    host = {key: (None if x is None else x.cpu().numpy()) for key, x in m.items()}
    other.close()
    keep = tsg.ReGeom(b, host, "hlbvh")
    other = gx.Scene(keep.desc())
    torch.cuda.synchronize()
    t_new.append(time.perf_counter() - t)
same = all((x == y).all() for x, y in zip(scene.bvh()[1:], other.bvh()[1:])) and (scene.bvh4()[0] == other.bvh4()[0]).all()
ms = lambda ts: statistics.median(ts[1:]) * 1e3
a, f, c = ms(t_set), ms(t_re), ms(t_new)
print(f"{scene.n_triangles} triangles, median of {args.calls} after 1 warm-up round, arms alternating:", flush=True)
print(f"  set_geometry (device tensors)        {a:9.2f} ms   (min {min(t_set[1:]) * 1e3:.2f}, max {max(t_set[1:]) * 1e3:.2f})")
print(f"  rebuild_bvh alone (the floor)        {f:9.2f} ms   (min {min(t_re[1:]) * 1e3:.2f}, max {max(t_re[1:]) * 1e3:.2f})")
print(f"  copy to host + close + Scene(hlbvh)  {c:9.2f} ms   (min {min(t_new[1:]) * 1e3:.2f}, max {max(t_new[1:]) * 1e3:.2f})")
print(f"  set_geometry / rebuild_bvh = {a / f:.2f}   recreate / set_geometry = {c / a:.2f}   same tree: {same}", flush=True)
