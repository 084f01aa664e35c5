"""Development measurement (MI355X): the time of the display stage and of what it is compared with (not run by pytest).

    python tests/dev_display_time.py [--n-tris 100000] [--width 1920] [--height 1080] [--spp 4] [--reps 9] [--inner 20] [--quick]

Scene: cfg 3 (Cornell box + the synthetic mesh, Glass + Metal, PathIntegrator(8, 1.0, "spatial")), one view: the frame
tests/dev_temporal_time.py renders.
  render      RenderDevice of the frame at --spp samples; its image is the "noisy" input of everything below
  histogram   luminance_histogram on two inputs: the render, and a constant image (every lane of a wave on one LDS word, the weak case
              of one LDS atomic per pixel).  `histogram_copy_ms`: a plain device-to-device copy that moves the 16 bytes per pixel the
              histogram reads (8 read + 8 written per pixel)
  exposure    auto_exposure on the render's histogram, in place
  tonemap     tonemap (ACES, sRGB, rounded) with the exposure read on the device; `tonemap_copy_ms`: a copy that moves the same 20
              bytes per pixel (10 read + 10 written)
  present     Display.present: the three calls; `present_copy_ms`: a copy of the 36 bytes per pixel the stage reads and writes;
              `stage_share_of_frame` = present / render
Every call is queued --inner times between two device events and the time divided (no call waits for the GPU, and one call's argument
checks then overlap the kernel before it, as they do in a frame loop); median, minimum and maximum of --reps such timings after one
warm-up.  One JSON line."""
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
    ap.add_argument("--inner", type=int, default=20, help="calls per timing")
    ap.add_argument("--quick", action="store_true", help="5000 triangles, 320 x 180")
    a = ap.parse_args()
    gx.init(0)
    W, H, n_tris = (320, 180, 5000) if a.quick else (a.width, a.height, a.n_tris)
    npix = W * H

    scene = gx.Scene(scenes.dragon_cornell(n_tris, "glass+metal"))
    integ = gx.PathIntegrator(8, 1.0, "spatial")
    img = torch.zeros((H, W, 4), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms_render, render_spread, _ = runs_ms(lambda: integ.RenderDevice(scene, img.data_ptr(), W, H, a.spp, stream=st), a.reps)
    img.zero_()
    integ.RenderDevice(scene, img.data_ptr(), W, H, a.spp, stream=st)
    torch.cuda.synchronize()

    constant = torch.full_like(img, 0.18)
    hist = torch.empty((1, 260), dtype=torch.int32, device="cuda")

    # ---- the three calls and the whole stage
    rec = torch.empty((1, 4), device="cuda")
    rgba8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    ms_hist, hist_spread, _ = runs_ms(lambda: gx.luminance_histogram(img, out=hist), a.reps, a.inner)
    ms_hist_c, hist_c_spread, _ = runs_ms(lambda: gx.luminance_histogram(constant, out=hist), a.reps, a.inner)
    gx.luminance_histogram(img, out=hist)
    gx.auto_exposure(hist, out=rec)
    ms_exp, exp_spread, _ = runs_ms(lambda: gx.auto_exposure(hist, prev=rec, out=rec, rate=0.1), a.reps, a.inner)
    ms_tone, tone_spread, _ = runs_ms(lambda: gx.tonemap(img, exposure=rec, out=rgba8), a.reps, a.inner)
    display = gx.Display(W, H, rate=0.1)
    ms_present, present_spread, shown = runs_ms(lambda: display.present(img), a.reps, a.inner)
    exposure = [float(x) for x in shown["exposure"][0].cpu()]

    def copy_ms(bytes_per_pixel):   # a copy that moves bytes_per_pixel per pixel: half read, half written
        n = npix * bytes_per_pixel // 8
        src, dst = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        return runs_ms(lambda: dst.copy_(src), a.reps, a.inner)[:2]

    (c16, c16_spread), (c20, c20_spread), (c36, c36_spread) = copy_ms(16), copy_ms(20), copy_ms(36)
    print(json.dumps({"n_tris": scene.n_triangles, "width": W, "height": H, "spp": a.spp, "reps": a.reps, "inner": a.inner,
                      "histogram_ms": ms_hist, "histogram_ms_min_max": hist_spread, "histogram_constant_ms": ms_hist_c, "histogram_constant_ms_min_max": hist_c_spread,
                      "histogram_gb_s": npix * 16 / ms_hist * 1e-6, "histogram_copy_ms": c16, "histogram_copy_ms_min_max": c16_spread, "histogram_over_copy": ms_hist / c16,
                      "exposure_ms": ms_exp, "exposure_ms_min_max": exp_spread,
                      "tonemap_ms": ms_tone, "tonemap_ms_min_max": tone_spread, "tonemap_gb_s": npix * 20 / ms_tone * 1e-6, "tonemap_copy_ms": c20,
                      "tonemap_copy_ms_min_max": c20_spread, "tonemap_over_copy": ms_tone / c20,
                      "present_ms": ms_present, "present_ms_min_max": present_spread, "present_copy_ms": c36, "present_copy_ms_min_max": c36_spread,
                      "present_over_copy": ms_present / c36, "exposure_record": exposure,
                      "render_ms": ms_render, "render_ms_min_max": render_spread, "stage_share_of_frame": ms_present / ms_render}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
