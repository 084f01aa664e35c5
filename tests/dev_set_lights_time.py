"""gnxr_scene_set_lights against its floor and against what a caller did without it (dev tool, MI355X):

    python tests/dev_set_lights_time.py [--calls 9]

The 100 k-triangle synthetic mesh in the Cornell box (cfg 3: 100 012 triangles, two area lights).  In this one process, after one warm-up
round, `--calls` rounds run the arms one after the other (alternating, so that drift reaches all alike); each figure is the median wall
time of an arm's calls, the host clock around work that ends synchronised:

  set_lights     Scene.set_lights, toggling: first to a mesh light of 500 model triangles, then back to the stock list (both timed)
  update_lights  Scene.update_lights of the whole stock list: the floor for a host-compiled upload of light records
  recreate       what a caller does without the entry point: Scene.close() and a new Scene (which compiles materials, lights and sampler
                 tables again, builds the tree and uploads everything)

The scene of the first arm must end with the light tables of the scene the third arm created last."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
import gnxraytracer_amd as gx, scenes
import test_light_update as tlu
import test_set_lights as tsl

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=9)
ap.add_argument("--triangles", type=int, default=100000)
ap.add_argument("--mesh-light", type=int, default=500)
args = ap.parse_args()
assert args.calls >= 9
gx.init(0)
b = scenes.dragon_cornell(args.triangles, "glass+metal")
stock = tlu.desc_lights(gx, b)
model = tsl.layout(b)[0]
tris = model[3::len(model) // args.mesh_light][:args.mesh_light]
mesh = [tsl.area(t, (3.0, 2.5, 2.0)) for t in tris]
scene = gx.Scene(b)
other = gx.Scene(b)            # the handle the third arm replaces
torch.cuda.synchronize()
t_mesh, t_stock, t_upd, t_new = [], [], [], []
for k in range(args.calls + 1):
    torch.cuda.synchronize()
    t = time.perf_counter(); scene.set_lights(mesh); torch.cuda.synchronize(); t_mesh.append(time.perf_counter() - t)
    t = time.perf_counter(); scene.set_lights(stock); torch.cuda.synchronize(); t_stock.append(time.perf_counter() - t)
    t = time.perf_counter(); scene.update_lights(stock); torch.cuda.synchronize(); t_upd.append(time.perf_counter() - t)
    t = time.perf_counter()
    other.close()
    other = gx.Scene(b)
    torch.cuda.synchronize()
    t_new.append(time.perf_counter() - t)
same = all(np.array_equal(x, y) for x, y in zip(scene.light_tables(), other.light_tables()))
ms = lambda ts: statistics.median(ts[1:]) * 1e3
rng = lambda ts: f"(min {min(ts[1:]) * 1e3:.2f}, max {max(ts[1:]) * 1e3:.2f})"
a, s, u, c = ms(t_mesh), ms(t_stock), ms(t_upd), ms(t_new)
print(f"{scene.n_triangles} triangles, median of {args.calls} after 1 warm-up round, arms alternating:", flush=True)
print(f"  set_lights -> {len(mesh)}-triangle mesh light      {a:9.3f} ms   {rng(t_mesh)}")
print(f"  set_lights -> the stock list ({len(stock)} lights)      {s:9.3f} ms   {rng(t_stock)}")
print(f"  update_lights of the stock list (floor)    {u:9.3f} ms   {rng(t_upd)}")
print(f"  close + Scene(...)                         {c:9.3f} ms   {rng(t_new)}")
print(f"  set_lights(mesh) / update_lights = {a / u:.1f}   recreate / set_lights(mesh) = {c / a:.1f}   recreate / set_lights(stock) = {c / s:.1f}   same tables: {same}", flush=True)
