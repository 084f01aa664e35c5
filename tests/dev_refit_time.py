"""Development measurement (MI355X): gnxr_scene_update_vertices against gnxr_scene_create, and what refit quality costs.

    python tests/dev_refit_time.py [--sizes 100000 1000000] [--calls 25]

Per size (the cfg 3 scene with the synthetic mesh of that many triangles, model vertices displaced by 2 % noise plus a translation):
  * wall time of gnxr_scene_create with the SAH and the HLBVH build (median of 3, host clock around the call)
  * wall time of gnxr_scene_update_vertices from host memory (median of --calls calls after 3 warm-up calls, host clock around the
    synchronous call; the calls alternate between two vertex sets so that every one changes the tree)
  * seconds_trace of a 1080p 16-spp Path render (SAH tree) refitted onto the deformed vertices versus built fresh on them
One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402
from test_scene_update import Deformed, deform, model_vertex_count, vertices  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    gx.init(0)
    for n_tris in a.sizes:
        b = scenes.dragon_cornell(n_tris, "glass+metal")
        nv = model_vertex_count(gx, scenes.synthetic_mesh_path(n_tris))
        v = vertices(b)
        v2 = deform(v, nv, seed=5, amount=0.02)
        v3 = deform(v, nv, seed=6, amount=0.02)
        create = {}
        for split in ("sah", "hlbvh"):
            b.set_bvh_split_method(split)
            ts = []
            for _ in range(3):
                t, s = timed(lambda: gx.Scene(b))
                s.close()
                ts.append(t)
            create[split] = statistics.median(ts)
        b.set_bvh_split_method("sah")
        scene = gx.Scene(b)
        sets = [np.ascontiguousarray(v2[:nv]), np.ascontiguousarray(v3[:nv])]
        for k in range(3):
            scene.update_vertices(sets[k % 2])
        ts = [timed(lambda: scene.update_vertices(sets[k % 2]))[0] for k in range(a.calls)]
        scene.update_vertices(sets[0])   # the refitted scene holds v2
        dv = Deformed(b, v2)   # (keeps v2 alive while the scene is created from it)
        fresh = gx.Scene(dv.desc())
        integ = gx.PathIntegrator(5, 1.0, "spatial")
        trace = {}
        for name, s in (("refit", scene), ("fresh", fresh)):
            integ.Reserve(s, 1920, 1080, a.spp)
            integ.Render(s, 1920, 1080, 1)   # warm-up (light table, clocks)
            gx.lib().gnxr_set_profiling(1)   # per-kernel timing: seconds_trace
            _, st = integ.Render(s, 1920, 1080, a.spp)
            gx.lib().gnxr_set_profiling(0)
            trace[name] = {"seconds_trace": st["seconds_trace"], "seconds_render": st["seconds_render"], "rays": st["rays_closest"] + st["rays_any"]}
        print(json.dumps({"n_tris": n_tris, "n_model_vertices": nv, "update_ms_median": 1e3 * statistics.median(ts), "update_ms_min": 1e3 * min(ts),
                          "update_calls": len(ts), "create_sah_ms": 1e3 * create["sah"], "create_hlbvh_ms": 1e3 * create["hlbvh"],
                          "render_1080p_spp": a.spp, "trace": trace}), flush=True)
        scene.close()
        fresh.close()


if __name__ == "__main__":
    main()
