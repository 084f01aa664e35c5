"""gnxr_scene_update_media against gnxr_scene_create of the same description (dev tool, MI355X):

    python tests/dev_media_update_time.py [--calls 11] [--log profiles/media_update_time.log]

Two grids: cfg 5's 100 x 100 x 40 (scenes.volume_cornell_cfg5) and a 256^3 one in the same scene.  In this one process, per grid and per
way of getting the next frame's density onto the device, the median and the extremes of the wall time of `--calls` calls after one
warm-up (every call returns when every device holds the edit, so the host clock around it is synchronised): Scene.update_media from a
device tensor, from a numpy array, coefficients only, and gnxr_scene_create of a description carrying the grid, which is what a caller
without this entry point does.  The kernel's own time is the one the library takes between two HIP events around k_media_grid
under GNXR_VERBOSE, against the 8 bytes per voxel the kernel moves.  Nothing is gated:
the numbers go to DESIGN.md."""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
import gnxraytracer_amd as gx, scenes
import test_media_update as tmu

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--log", default=None)
args = ap.parse_args()
assert args.calls >= 10
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


def kernel_times(f):
    """us of every k_media_grid launch of `--calls` calls of f after one warm-up, from the lines the library writes under GNXR_VERBOSE"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GNXR_VERBOSE"] = "1"
        try:
            for _ in range(args.calls + 1):
                f()
        finally:
            del os.environ["GNXR_VERBOSE"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        us = [float(m) for m in re.findall(r"k_media_grid: .* voxels, ([0-9.]+) us", tmp.read().decode())]
    assert len(us) == args.calls + 1, us
    return us[1:]


def row(name, t, unit="ms"):
    say(f"  {name:<44s} median {statistics.median(t):10.3f} {unit}   min {min(t):10.3f}   max {max(t):10.3f}")


def measure(name, b, next_grid):
    media, grids0 = tmu.desc_media(b)
    rec = tmu.edited(media[tmu.GRID], next_grid)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    d_next = torch.from_numpy(next_grid).to(dev)
    nv = next_grid.size
    say(f"{name}: {rec.nx} x {rec.ny} x {rec.nz} = {nv} voxels ({nv * 4e-6:.1f} MB), {scene.n_triangles} triangles, {args.calls} calls after 1 warm-up, {torch.cuda.get_device_name(dev)}")
    t_dev = timed(lambda: scene.update_media(rec, d_next))
    t_np = timed(lambda: scene.update_media(rec, next_grid))
    t_coef = timed(lambda: scene.update_media(rec))
    e = tmu.WithMedia(b, [rec, media[tmu.HOM]], [next_grid, None])
    t_create = timed(lambda: gx.Scene(e.desc()))
    t_kernel = kernel_times(lambda: scene.update_media(rec, d_next))
    row("update_media, device tensor", t_dev)
    row("update_media, numpy array", t_np)
    row("update_media, coefficients only", t_coef)
    row("gnxr_scene_create, same description", t_create)
    row("k_media_grid between its own HIP events", t_kernel, "us")
    say(f"  8 B per voxel over the median kernel time: {8.0 * nv / (statistics.median(t_kernel) * 1e-6) * 1e-9:.0f} GB/s; "
        f"create / device-source update: x{statistics.median(t_create) / statistics.median(t_dev):.1f}")
    tmu.same_tables(scene, gx.Scene(e.desc()))
    say("  tables after the last update: bit for bit those of the created scene")


b5 = scenes.volume_cornell_cfg5(0.05)
g5 = scenes.reference_density()
measure("cfg 5", b5, np.ascontiguousarray(np.roll(g5, 3, axis=1) * np.float32(0.9)))   # the next frame's smoke: drifted and thinned
big = np.random.default_rng(1).random((256, 256, 256), dtype=np.float32)
measure("256^3", scenes.volume_cornell(big, sigma_a=(0.5,) * 3, sigma_s=(3.5,) * 3), np.ascontiguousarray(big[::-1] * np.float32(0.5)))
if args.log:
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
