"""Development measurement (MI355X): the denoiser (gnxr_denoise_device) against its floor and the render it accompanies (not run by pytest).

    python tests/dev_denoise_time.py [--n-tris 100000] [--width 1920 --height 1080] [--spp 16] [--reps 15] [--profile-run]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")).  The two halves of an spp-sample
render and the feature buffers are made once; every arm then runs in this process as one warm-up call and --reps synchronised calls,
of which the median and the extremes of the device time (events on the current stream around the call) are reported:
  (a) denoise_<k>     gx.denoise with both shares and all guides, k = 1 .. 5 iterations; the step from k - 1 to k is the a-trous kernel
                      of step 2^(k-1) (the last one of a call also remodulates); denoise_5 is the call that is compared
  (b) denoise_5_one_image, denoise_5_no_guides
                      the variants without the second image (no variance window) and without guides (no guide record per tap)
  (c) copy            a device-to-device copy of the call's unique bytes -- 68 read (two shares, albedo, normal, depth) + 16 written per
                      pixel: the floor of any implementation
  (d) render          RenderDevice at --spp samples: the work the filter accompanies
One JSON line per arm, then one summary line with both ratios.  --profile-run: only a warm-up and --reps calls of denoise_5, for
`rocprofv3 --kernel-trace --stats -- python tests/dev_denoise_time.py --profile-run` (per-kernel times, in a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def arm(name, fn, reps, **extra):
    timed(fn)   # warm-up
    ev = [timed(fn) for _ in range(reps)]
    row = {"arm": name, "median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "all_ms": ev}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    gx.init(0)
    W, H, spp = a.width, a.height, a.spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    stream = torch.cuda.current_stream().cuda_stream
    halves = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    integ.Reserve(scene, W, H, spp)
    integ.RenderDevice(scene, halves[0].data_ptr(), W, H, spp, stream=stream, spp_begin=0, spp_end=spp // 2)
    integ.RenderDevice(scene, halves[1].data_ptr(), W, H, spp, stream=stream, spp_begin=spp // 2, spp_end=spp)
    aov, _ = integ.RenderAOV(scene, W, H, spp, channels=("albedo", "shading_normal", "depth"))
    guides = dict(albedo=aov["albedo"], normal=aov["shading_normal"], depth=aov["depth"])
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    full = lambda k: gx.denoise(halves[0], halves[1], iterations=k, out=out, **guides)
    if a.profile_run:
        for _ in range(a.reps + 1):
            full(5)
        torch.cuda.synchronize()
        scene.close()
        return

    rows = {}
    for k in range(1, 6):
        rows[k] = arm(f"denoise_{k}", lambda: full(k), a.reps, iterations=k)
    arm("denoise_5_one_image", lambda: gx.denoise(halves[0], iterations=5, out=out, **guides), a.reps)
    arm("denoise_5_no_guides", lambda: gx.denoise(halves[0], halves[1], iterations=5, out=out), a.reps)
    unique = (68 + 16) * W * H
    src = torch.zeros((unique,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    copy = arm("copy", lambda: dst.copy_(src), a.reps, bytes=unique)
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    render = arm("render", lambda: integ.RenderDevice(scene, image.data_ptr(), W, H, spp, stream=stream), a.reps, spp=spp)
    d = rows[5]
    steps = [rows[1]["median_ms"]] + [rows[k]["median_ms"] - rows[k - 1]["median_ms"] for k in range(2, 6)]
    print(json.dumps({"summary": True, "width": W, "height": H, "spp": spp, "n_tris": a.n_tris, "reps": a.reps,
                      "denoise_ms": [d["min_ms"], d["median_ms"], d["max_ms"]], "copy_ms": [copy["min_ms"], copy["median_ms"], copy["max_ms"]],
                      "render_ms": [render["min_ms"], render["median_ms"], render["max_ms"]],
                      "prepare_and_first_iteration_ms": steps[0], "added_ms_per_further_iteration": steps[1:],
                      "denoise_over_copy": d["median_ms"] / copy["median_ms"], "denoise_over_render": d["median_ms"] / render["median_ms"],
                      "ns_per_pixel": d["median_ms"] * 1e6 / (W * H)}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
