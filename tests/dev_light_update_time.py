"""Development measurement (MI355X): what GNXR_UPDATE_MOVE_LIGHTS adds to gnxr_scene_update_vertices.

    python tests/dev_light_update_time.py [--calls 25]

Two scenes: cfg 3 (the 100 k-triangle synthetic mesh in the Cornell box, 2 area lights) and the 2 k-triangle Cornell scene with a
300-triangle emissive sheet (302 lights).  Per scene the wall time of Scene.update_vertices over the model's vertices (host memory, host
clock around the synchronous call, median of --calls calls after 3 warm-up calls, alternating between two vertex sets) without the flag
(k_refit_check runs, the lights stay) and with it (k_refit_lights recomputes every area light and the records come back with the root box),
and, with the flag, over every vertex of the scene with the emissive ones displaced.  Both variants are timed on this library: without the
flag the call is the code path gnxr_scene_update_vertices had before the flag existed.  One JSON line per scene."""
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
from test_light_update import mesh_light_scene  # noqa: E402
from test_scene_update import MESH2K, deform, emissive_vertices, model_vertex_count, vertices  # noqa: E402


def median_ms(fn, calls):
    for k in range(3):
        fn(k)
    ts = []
    for k in range(calls):
        t0 = time.perf_counter()
        fn(k)
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts), 1e3 * min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    a = ap.parse_args()
    gx.init(0)
    cases = [("cfg3_100k", scenes.dragon_cornell(100000, "glass+metal"), model_vertex_count(gx, scenes.synthetic_mesh_path(100000))),
             ("mesh2k_300_lights", mesh_light_scene(), model_vertex_count(gx, MESH2K))]
    for name, b, nv in cases:
        v = vertices(b)
        sets = [deform(v, nv, seed=5, amount=0.02), deform(v, nv, seed=6, amount=0.02)]
        ev = emissive_vertices(b)
        moved = []
        for s in sets:   # the same, with every emissive vertex displaced too
            m = s.copy()
            m[ev] += np.array([0.05, -0.2, 0.03], np.float32)
            moved.append(m)
        scene = gx.Scene(b)
        model = [np.ascontiguousarray(s[:nv]) for s in sets]
        plain = median_ms(lambda k: scene.update_vertices(model[k % 2]), a.calls)
        flag = median_ms(lambda k: scene.update_vertices(model[k % 2], move_lights=True), a.calls)
        everything = median_ms(lambda k: scene.update_vertices(moved[k % 2], move_lights=True), a.calls)
        print(json.dumps({"scene": name, "n_triangles": scene.n_triangles, "n_lights": int(b.desc().n_lights), "n_model_vertices": nv, "n_vertices": len(v),
                          "calls": a.calls, "update_ms_median": plain[0], "update_ms_min": plain[1], "move_lights_ms_median": flag[0], "move_lights_ms_min": flag[1],
                          "move_lights_all_vertices_ms_median": everything[0], "move_lights_all_vertices_ms_min": everything[1]}), flush=True)
        scene.close()


if __name__ == "__main__":
    main()
