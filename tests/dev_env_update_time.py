"""gnxr_scene_update_environment against gnxr_scene_create of the same description (dev tool, MI355X):

    python tests/dev_env_update_time.py [--calls 7] [--log profiles/env_update_time.log]

The cfg 4 scene (the 100 k-triangle synthetic mesh in the Cornell box, area light, environment light) with the 1000 x 500 synthetic map.
In this one process, per way of getting the new environment onto the device, the median and the extremes of the wall time of `--calls`
calls after one warm-up (every call returns when every device holds the new tables, so the host clock around it is synchronised):
Scene.update_environment from a device tensor, from a numpy array, rotation only, and gnxr_scene_create of a description carrying the
map, which is what a caller without this entry point does.  build_env alone -- the host build the update replaces -- is recorded as the
difference between creates with and without the environment light.  The one gate: the slowest update from device memory is faster than
the fastest create."""
import argparse
import itertools
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
import gnxraytracer_amd as gx, scenes
import test_environment_update as teu

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--log", default=None)
args = ap.parse_args()
assert args.calls >= 5
gx.init(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    out = []
    for _ in range(args.calls + 1):
        torch.cuda.synchronize()
        t = time.perf_counter(); keep = f(); torch.cuda.synchronize(); out.append(time.perf_counter() - t)
        del keep
    return [x * 1e3 for x in out[1:]]


def row(name, t):
    say(f"{name:<44s} median {statistics.median(t):9.3f} ms   min {min(t):9.3f}   max {max(t):9.3f}")


env_path = scenes.synthetic_env_path()
b = scenes.dragon_cornell(100000, "zoo", env=env_path)
b_plain = scenes.dragon_cornell(100000, "zoo", env=None)
m0 = scenes.synthetic_env()
m1 = np.ascontiguousarray(np.roll(m0, 137, axis=1) * np.float32(0.75))   # the next frame's sky: turned and dimmed
scene = gx.Scene(b)
d_m1 = torch.from_numpy(m1).to(f"cuda:{scene.device}")
created_with = list(scene._env_light.light_to_world)   # the transform of the description
turns = itertools.cycle([teu.ROT, created_with])

say(f"{scene.n_triangles} triangles, environment map {m1.shape[1]} x {m1.shape[0]}, {args.calls} calls after 1 warm-up, {torch.cuda.get_device_name(scene.device)}")
t_dev = timed(lambda: scene.update_environment(d_m1))
t_np = timed(lambda: scene.update_environment(m1))
t_rot = timed(lambda: scene.update_environment(light_to_world=next(turns)))
e = teu.WithEnv(b, m1)
t_create = timed(lambda: gx.Scene(e.desc()))
t_plain = timed(lambda: gx.Scene(b_plain.desc()))
row("update_environment, device tensor", t_dev)
row("update_environment, numpy array", t_np)
row("update_environment, rotation only", t_rot)
row("gnxr_scene_create, same description", t_create)
row("gnxr_scene_create, no environment light", t_plain)
build_env = statistics.median(t_create) - statistics.median(t_plain)
say(f"build_env alone (difference of the create medians): {build_env:.3f} ms; over the device-source update: x{build_env / statistics.median(t_dev):.1f}")
scene.update_environment(m1, light_to_world=created_with)
fresh = gx.Scene(e.desc())
teu.same_tables(scene, fresh)
say("tables after the last update: bit for bit those of the created scene")
gate = max(t_dev) < min(t_create)
say(f"gate (slowest device-source update {max(t_dev):.3f} ms < fastest create {min(t_create):.3f} ms): {'PASS' if gate else 'FAIL'}")
if args.log:
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if gate else 1)
