"""Development measurement (MI355X): adaptive sampling (gnxr_render_adaptive_device) against the fixed-spp render (not run by pytest).

    python tests/dev_adaptive_time.py [--n-tris 100000] [--width 1920 --height 1080] [--spp 1024] [--reps 7]
                                      [--steps 32,64,128] [--thresholds 0.05,0.1,0.2] [--schedules 16:16,64:64]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")).  All arms run in this process after
gnxr_render_reserve; each is one warm-up call and then --reps synchronised calls, of which the median and the extremes of the device
time (events on the current stream around the call) are reported, with the wall clock's median:
  (a) render           RenderDevice, the fixed-spp path
  (b) adaptive_full    RenderAdaptive with min_spp == spp: the same path work through the pixel list and k_adaptive_accum; `identical`:
                       its image holds the bits of (a)'s
  (c) rounds_<step>    threshold 0 with min_spp = step_spp = <step>: only pixels whose e is exactly 0 stop, so this prices the round
                       boundaries (each round ends with the drain of the persistent traversal launches and one 4-byte read-back)
  (d) threshold_<t>_<min_spp>_<step_spp>
                       practical thresholds under every schedule of --schedules (min_spp:step_spp): the fraction of the budget's samples
                       taken and the time; `gate`: a run that took at most half of the budget's samples must beat the fastest repetition of (a)
One JSON line per arm, then one summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    st = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, st


def arm(name, fn, reps, extra=None):
    timed(fn)   # warm-up
    ev, wall, st = [], [], None
    for _ in range(reps):
        ms, w, st = timed(fn)
        ev.append(ms); wall.append(w)
    row = {"arm": name, "median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "wall_median_ms": statistics.median(wall), "all_ms": ev}
    for k in ("rounds", "samples", "pixels_at_budget", "kernel_launches", "passes", "passes_in_flight", "rays_closest", "rays_any"):
        if st and k in st:
            row[k] = st[k]
    if extra:
        row.update(extra(st))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="32,64,128")
    ap.add_argument("--thresholds", default="0.05,0.1,0.2")
    ap.add_argument("--schedules", default="16:16,64:64")
    a = ap.parse_args()
    gx.init(0)
    W, H, spp = a.width, a.height, a.spp
    budget = W * H * spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    stream = torch.cuda.current_stream()
    ref = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    integ.Reserve(scene, W, H, spp)
    share = lambda st: {"sample_share": st["samples"] / budget}

    rows = [arm("render", lambda: integ.RenderDevice(scene, ref.data_ptr(), W, H, spp, stream=stream.cuda_stream), a.reps)]
    base = rows[0]
    rows.append(arm("adaptive_full", lambda: integ.RenderAdaptive(scene, W, H, spp, 0.0, min_spp=spp, out=img, count_out=cnt)[2], a.reps, share))
    torch.cuda.synchronize()
    identical = bool((ref.view(torch.int32) == img.view(torch.int32)).all().item()) and bool(ref[..., :3].any().item())
    for step in (int(s) for s in a.steps.split(",") if s):
        rows.append(arm(f"rounds_{step}", lambda: integ.RenderAdaptive(scene, W, H, spp, 0.0, min_spp=step, step_spp=step, guard=0, out=img, count_out=cnt)[2], a.reps, share))
    gate = []
    for lo, step in ((int(v) for v in sch.split(":")) for sch in a.schedules.split(",") if sch):
        for t in (float(s) for s in a.thresholds.split(",") if s):
            r = arm(f"threshold_{t:g}_{lo}_{step}", lambda: integ.RenderAdaptive(scene, W, H, spp, t, min_spp=lo, step_spp=step, out=img, count_out=cnt)[2], a.reps, share)
            rows.append(r)
            if r["sample_share"] <= 0.5:
                gate.append({"arm": r["arm"], "sample_share": r["sample_share"], "max_ms": r["max_ms"], "median_ms": r["median_ms"], "render_min_ms": base["min_ms"],
                             "passes": r["max_ms"] < base["min_ms"]})
    full = rows[1]
    print(json.dumps({"summary": True, "width": W, "height": H, "spp": spp, "n_tris": a.n_tris, "reps": a.reps, "identical_full_budget": identical,
                      "render_ms": [base["min_ms"], base["median_ms"], base["max_ms"]], "adaptive_full_ms": [full["min_ms"], full["median_ms"], full["max_ms"]],
                      "adaptive_full_over_render": full["median_ms"] / base["median_ms"],
                      "adaptive_full_inside_render_spread": base["min_ms"] <= full["median_ms"] <= base["max_ms"], "gate": gate,
                      "gate_passes": bool(gate) and all(g["passes"] for g in gate)}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
