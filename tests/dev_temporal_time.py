"""Development measurement (MI355X): the time of the temporal stage and of what it is compared with (not run by pytest).

    python tests/dev_temporal_time.py [--n-tris 100000] [--width 1920] [--height 1080] [--spp 4] [--reps 9] [--inner 20] [--quick]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")), one view.
  accumulate  temporal_accumulate on synthetic buffers: a history that every tap accepts (one primitive, one normal, one depth), so that
              all four taps of every pixel are read and weighed, under a smooth fractional motion of a few pixels (what a moving camera
              gives: an offset that varies slowly over the image); `accumulate_gb_s`: the unique bytes (52 of history + 52 of this
              frame + 32 written = 136 per pixel) over its time.  `accumulate_scattered_*`: the same under a motion drawn per pixel
              from [-3, 3]^2, which no camera produces: neighbouring lanes then read taps up to six pixels and six rows apart
  copy        a plain device-to-device copy that moves the same 136 bytes per pixel (68 read, 68 written) in the same process;
              `accumulate_over_copy` compares the two
              Both are queued --inner times between two events and the time divided: neither call waits for the GPU, and one call's
              argument checks (ten pointer queries) then overlap the kernel before it, as they do in a frame loop.
  motion      Scene.motion through the scene's camera, the previous camera moved and turned by a few degrees; all three channels
  intersect   Scene.intersect alone on the same pixel-centre rays (generated on the host, resident on the device);
              `motion_over_intersect` compares the two
  render      RenderDevice of the frame at --spp samples: `stage_share_of_frame` = (motion + accumulate) / render
Call time: device events around each call on the current stream after one warm-up; median, minimum and maximum of --reps runs.
One JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402
import temporal_reference as tr  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def runs_ms(fn, reps, inner=1):
    """(median, [min, max], the last result) of `reps` timings after one warm-up; a timing is `inner` calls between two events, divided"""
    def many():
        for _ in range(inner):
            r = fn()
        return r
    timed(many)
    runs = [timed(many) for _ in range(reps)]
    ms = [r[0] / inner for r in runs]
    return statistics.median(ms), [min(ms), max(ms)], runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-tris", type=int, default=100000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20, help="calls per timing of the two calls that do not wait for the GPU")
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 320 x 180")
    a = ap.parse_args()
    gx.init(0)
    W, H, n_tris = (320, 180, 5000) if a.quick else (a.width, a.height, a.n_tris)
    npix = W * H
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    # ---- accumulate against a copy of its unique bytes
    rng = np.random.default_rng(20261020)
    yy, xx = np.mgrid[0:H, 0:W]
    flow = lambda dx, dy: np.stack([xx + 0.5 + dx, yy + 0.5 + dy, np.full((H, W), 2.0), np.ones((H, W))], -1).astype(np.float32)
    motion = flow(2.37 + 1.5 * np.sin(yy / 97.0) + xx / W, -1.62 + 1.2 * np.cos(xx / 131.0) - yy / H)
    scattered = flow(rng.uniform(-3, 3, (H, W)), rng.uniform(-3, 3, (H, W)))
    guide = np.tile(np.array([0, 0, 1, 2], np.float32), (H, W, 1))
    stat = np.tile(np.array([0.5, 0.3, 8, 0.05], np.float32), (H, W, 1))
    color, hcolor = rng.random((H, W, 4)).astype(np.float32), rng.random((H, W, 4)).astype(np.float32)
    prim = np.zeros((H, W), np.int32)
    d = {k: dev(v) for k, v in dict(color=color, motion=motion, guide=guide, prim=prim).items()}
    hist = {"color": dev(hcolor), "stat": dev(stat), "guide": dev(guide.copy()), "prim": dev(prim.copy())}
    out = {"color": torch.empty((H, W, 4), device="cuda"), "stat": torch.empty((H, W, 4), device="cuda")}
    ms_acc, acc_spread, res = runs_ms(lambda: gx.temporal_accumulate(d["color"], d["motion"], d["guide"], d["prim"], history=hist, out=out), a.reps, a.inner)
    four_taps = float((res["stat"][..., 2] > 8.5).float().mean().item())   # a pixel whose taps all count ends at N = 9
    src, dst = torch.empty((npix, 17), device="cuda"), torch.empty((npix, 17), device="cuda")   # 68 bytes per pixel read, 68 written
    ms_copy, copy_spread, _ = runs_ms(lambda: dst.copy_(src), a.reps, a.inner)
    d_scattered = dev(scattered)
    ms_scat, scat_spread, _ = runs_ms(lambda: gx.temporal_accumulate(d["color"], d_scattered, d["guide"], d["prim"], history=hist, out=out), a.reps, a.inner)

    # ---- motion against the traversal alone, and the stage as a share of a frame
    b = scenes.dragon_cornell(n_tris, "glass+metal")
    scene = gx.Scene(b)
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    cam = scene.camera
    prev = gx.camera(eye=(0.2, 0.1, 5.2), look=(-0.15, 0.05, 0.0), up=(0.03, 1, 0), fov=cam.fov_deg)
    mo_out = {"motion": torch.empty((H, W, 4), device="cuda"), "guide": torch.empty((H, W, 4), device="cuda"), "prim": torch.empty((H, W), dtype=torch.int32, device="cuda")}
    ms_motion, motion_spread, mo = runs_ms(lambda: scene.motion(W, H, prev, out=mo_out), a.reps)
    rays = dev(tr.centre_rays(gx, cam, W, H))
    hits = torch.empty((npix, 8), device="cuda")
    ms_isect, isect_spread, h = runs_ms(lambda: scene.intersect(rays, out=hits), a.reps)
    same_hits = bool(torch.equal(h.prim.reshape(H, W), mo["prim"]))
    img = torch.zeros((H, W, 4), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms_render, render_spread, _ = runs_ms(lambda: integ.RenderDevice(scene, img.data_ptr(), W, H, a.spp, stream=st), a.reps)
    flagged = float((mo["motion"][..., 3] == 1).float().mean().item())
    print(json.dumps({"n_tris": scene.n_triangles, "width": W, "height": H, "spp": a.spp, "reps": a.reps,
                      "accumulate_ms": ms_acc, "accumulate_ms_min_max": acc_spread, "accumulate_gb_s": npix * 136 / ms_acc * 1e-6, "accumulate_four_tap_share": four_taps,
                      "copy_ms": ms_copy, "copy_ms_min_max": copy_spread, "copy_gb_s_moved": npix * 136 / ms_copy * 1e-6, "accumulate_over_copy": ms_acc / ms_copy,
                      "accumulate_scattered_ms": ms_scat, "accumulate_scattered_ms_min_max": scat_spread, "accumulate_scattered_over_copy": ms_scat / ms_copy, "inner": a.inner,
                      "motion_ms": ms_motion, "motion_ms_min_max": motion_spread, "intersect_ms": ms_isect, "intersect_ms_min_max": isect_spread,
                      "motion_over_intersect": ms_motion / ms_isect, "motion_prims_equal_intersect": same_hits, "motion_flagged_share": flagged,
                      "render_ms": ms_render, "render_ms_min_max": render_spread, "stage_ms": ms_motion + ms_acc,
                      "stage_share_of_frame": (ms_motion + ms_acc) / ms_render}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
