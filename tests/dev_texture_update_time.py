"""gnxr_scene_update_textures against gnxr_scene_create of the same description (dev tool, MI355X):

    python tests/dev_texture_update_time.py [--calls 11] [--log profiles/texture_update_time.log]

Two images for the back wall's texture of scenes.textured_cornell: 2048 x 2048 (a power of two: convert, then the pyramid) and
1000 x 1000 (pads to 1024 x 1024 through both resample passes).  In this one process, per image and per way of getting the next frame's
texels onto the device, the median and the extremes of the wall time of `--calls` calls after one warm-up (every call returns when every
device holds the edit, so the host clock around it is synchronised): Scene.update_textures from a device tensor (a), from a numpy array
(b), parameters only, and destroy + gnxr_scene_create of a description carrying the image (c), which is what a caller without this entry
point does; of (c), the host's time in build_textures alone (d), which the library reports under GNXR_VERBOSE.  The kernels' own times
are those the library takes between two HIP events around every launch under GNXR_VERBOSE, with the bytes each launch moves.  Every update
builds a FRESH packed buffer and swaps it in (that is what makes a refused call leave the scene alone): its allocation, the device to
device copy of the other texture's pyramid and the release of the old buffer are part of (a) and (b).  Nothing is gated: the numbers go
to DESIGN.md."""
import argparse
import collections
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
import gnxraytracer_amd as gx
import test_texture_update as ttu

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


def verbose_lines(f):
    """the lines the library writes on stderr under GNXR_VERBOSE during `--calls` calls of f after one warm-up, as one list per call"""
    sys.stderr.flush()
    keep = os.dup(2)
    out = []
    os.environ["GNXR_VERBOSE"] = "1"
    try:
        for _ in range(args.calls + 1):
            with tempfile.TemporaryFile() as tmp:
                os.dup2(tmp.fileno(), 2)
                try:
                    held = f()
                    del held
                finally:
                    os.dup2(keep, 2)
                tmp.seek(0)
                out.append(tmp.read().decode().splitlines())
    finally:
        del os.environ["GNXR_VERBOSE"]
        os.close(keep)
    return out[1:]


def row(name, t, unit="ms", tail=""):
    say(f"  {name:<52s} median {statistics.median(t):10.3f} {unit}   min {min(t):10.3f}   max {max(t):10.3f}{tail}")


def measure(name, image):
    b = ttu.base()
    recs0, imgs0 = ttu.desc_textures(b)
    rec = ttu.edited(recs0[ttu.WALL], image)
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    d_next = torch.from_numpy(image).to(dev)
    h, w = image.shape[:2]
    say(f"{name}: {w} x {h} texels ({image.size * 4e-6:.1f} MB of RGB fp32), texture {ttu.WALL} of textured_cornell, {args.calls} calls after 1 warm-up, "
        f"{torch.cuda.get_device_name(dev)}")
    t_dev = timed(lambda: scene.update_textures(d_next))
    t_np = timed(lambda: scene.update_textures(image))
    t_par = timed(lambda: scene.update_textures(params=dict(su=1.0)))
    e = ttu.WithTextures(b, [rec, recs0[ttu.FLOOR]], [image, imgs0[ttu.FLOOR]])
    t_create = timed(lambda: gx.Scene(e.desc()).close())
    host = [float(m.group(1)) for call in verbose_lines(lambda: gx.Scene(e.desc()).close()) for ln in call for m in [re.search(r"build_textures: .* ([0-9.]+) ms on the host", ln)] if m]
    assert len(host) == args.calls, host
    row("a. update_textures, device tensor", t_dev)
    row("b. update_textures, numpy array", t_np)
    row("   update_textures, parameters only", t_par)
    row("c. destroy + gnxr_scene_create, same description", t_create)
    row("d. build_textures on the host, inside c", host)
    per_kernel = collections.OrderedDict()
    for call in verbose_lines(lambda: scene.update_textures(d_next)):
        seen = collections.Counter()
        for ln in call:
            m = re.search(r"\[gnxr\] (k_tex_\w+): device \d+, texture \d+, (\d+) texels, ([0-9.]+) us, (\d+) bytes", ln)
            if m:
                key = f"{m.group(1)} #{seen[m.group(1)]} ({int(m.group(2))} texels out)"
                seen[m.group(1)] += 1
                per_kernel.setdefault(key, ([], int(m.group(4))))[0].append(float(m.group(3)))
    total = 0.0
    for key, (us, nbytes) in per_kernel.items():
        assert len(us) == args.calls, (key, us)
        med = statistics.median(us)
        total += med
        row(key, us, "us", f"   {nbytes * 1e-6:9.3f} MB, {nbytes / (med * 1e-6) * 1e-9:7.0f} GB/s")
    say(f"  sum of the median kernel times {total:.1f} us; d / a: x{statistics.median(host) / statistics.median(t_dev):.1f}, d / b: x{statistics.median(host) / statistics.median(t_np):.1f}, "
        f"c / a: x{statistics.median(t_create) / statistics.median(t_dev):.1f}")
    ttu.same_tables(scene, gx.Scene(e.desc()))
    say("  tables after the last update: bit for bit those of the created scene")


measure("2048 x 2048", ttu.picture(2048, 2048, 1))
measure("1000 x 1000", ttu.picture(1000, 1000, 2))
if args.log:
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
