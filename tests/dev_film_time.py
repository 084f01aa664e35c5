"""Development measurement (MI355X): what the film costs a render, and that it costs a plain render nothing (not run by pytest).

    python tests/dev_film_time.py [--parent-lib PATH] [--n-tris 100000] [--width 1920 --height 1080] [--spp 64] [--reps 5] [--rounds 3]
    python tests/dev_film_time.py --profile-run            (for rocprofv3: Gaussian 2 alone)

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")) at --width x --height, --spp samples.
Every arm runs in a process of its own (GNXR_LIB selects the build), as one warm-up call and --reps synchronised calls; the device time
of a call is taken from events on the stream around it.
  (a) plain_parent / plain_this   RenderDevice with the library of the parent commit (--parent-lib: a build of the commit before the
                                  film, e.g. ab_libs/libgnxr_parent.so) and with this tree's, alternating --rounds times: the spread of
                                  the alternation is the yardstick for "the plain render did not change"
  (b) box_0.5, gaussian_2, mitchell_4
                                  RenderFiltered on this tree's library; stats' seconds_shade of the same process's plain render is
                                  printed beside them (gnxr_set_profiling(1): a run of its own, not the timed one)
One JSON line per arm and round, then a summary: medians, the spread of the alternation, each filter's overhead as a share of the plain
render.  Without --parent-lib arm (a) alternates this tree's library with itself (the spread alone)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FILTERS = {"box_0.5": ("box", 0.5), "gaussian_2": ("gaussian", 2.0), "mitchell_4": ("mitchell", 4.0)}


def child(a):
    import torch

    import gnxraytracer_amd as gx
    import scenes
    if a.child == "plain_parent":   # a library from before the film exports none of its symbols
        for name in [n for n in gx._abi.PROTOTYPES if "film" in n or "filtered" in n]:
            del gx._abi.PROTOTYPES[name]
    gx.init(0)
    W, H, spp = a.width, a.height, a.spp
    scene = gx.Scene(scenes.dragon_cornell(a.n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    stream = torch.cuda.current_stream().cuda_stream
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    integ.Reserve(scene, W, H, spp)
    if a.child.startswith("plain"):
        fn = lambda: integ.RenderDevice(scene, image.data_ptr(), W, H, spp, stream=stream)
    else:
        f = gx.film_filter(*FILTERS[a.child])
        fn = lambda: integ.RenderFiltered(scene, W, H, spp, f, out=image)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed()   # warm-up
    ev = [timed() for _ in range(a.reps)]
    row = {"arm": a.child, "median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "all_ms": ev}
    if a.child == "plain_this":   # the shade stage of the same render, from a profiled run of its own
        gx.lib().gnxr_set_profiling(1)
        st = integ.RenderDevice(scene, image.data_ptr(), W, H, spp, stream=stream)
        gx.lib().gnxr_set_profiling(0)
        row.update(shade_ms=st["seconds_shade"] * 1e3, trace_ms=st["seconds_trace"] * 1e3)
    print(json.dumps(row), flush=True)
    scene.close()


def run_child(a, arm, lib=None):
    env = dict(os.environ)
    if lib:
        env["GNXR_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--n-tris", str(a.n_tris), "--width", str(a.width), "--height", str(a.height), "--spp", str(a.spp),
           "--reps", str(a.reps)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if out.returncode != 0:   # nothing more is started on the GPU after a child that failed
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"{arm}: exit status {out.returncode}")
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default="")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    if a.profile_run:
        a.child = "gaussian_2"
    if a.child:
        return child(a)
    plain = {"plain_parent": [], "plain_this": []}
    for _ in range(a.rounds):
        plain["plain_parent"].append(run_child(a, "plain_parent" if a.parent_lib else "plain_this", a.parent_lib or None))
        plain["plain_this"].append(run_child(a, "plain_this"))
    filtered = {name: run_child(a, name) for name in FILTERS}
    med = {k: [r["median_ms"] for r in v] for k, v in plain.items()}
    this = statistics.median(med["plain_this"])
    every = med["plain_parent"] + med["plain_this"]
    shade = statistics.median(r["shade_ms"] for r in plain["plain_this"])
    print(json.dumps({"summary": True, "width": a.width, "height": a.height, "spp": a.spp, "n_tris": a.n_tris, "reps": a.reps, "rounds": a.rounds,
                      "parent_lib": bool(a.parent_lib), "plain_parent_ms": med["plain_parent"], "plain_this_ms": med["plain_this"],
                      "this_over_parent": this / statistics.median(med["plain_parent"]), "alternation_spread": (max(every) - min(every)) / this,
                      "shade_ms_of_plain": shade,
                      "filtered_ms": {k: r["median_ms"] for k, r in filtered.items()},
                      "overhead_ms": {k: r["median_ms"] - this for k, r in filtered.items()},
                      "overhead_share_of_plain": {k: (r["median_ms"] - this) / this for k, r in filtered.items()}}), flush=True)


if __name__ == "__main__":
    main()
