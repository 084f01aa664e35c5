"""Development measurement (MI355X): a material edit of a live scene against creating the scene again.

    python tests/dev_material_update_time.py [--calls 25]

cfg 3 (the 100 k-triangle synthetic mesh in the Cornell box).  Wall time, host clock around the synchronous call, median of --calls calls
after 3 warm-up calls, alternating between two states:

  - Scene.update_materials of one record whose type changes (the model's Glass <-> a Plastic): the material tables and one pass of
    k_material_tris over every triangle;
  - Scene.set_triangle_materials over every triangle from a device tensor (every other model triangle moves to another material and back);
  - gnxr_scene_create on the edited description, in the same run: what a caller paid for either edit before (creation is the same code).

One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402
from test_material_update import desc_materials, fresh_scene, tri_materials, with_record  # noqa: E402


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
    ap.add_argument("--creates", type=int, default=5)
    a = ap.parse_args()
    gx.init(0)
    A = gx._abi
    b = scenes.dragon_cornell(100000, "glass+metal")
    mats0 = desc_materials(gx, b)
    glass = next(i for i, m in enumerate(mats0) if m.type == A.MAT_GLASS)
    records = [gx.material(type=A.MAT_PLASTIC, kd=(0.3, 0.1, 0.6), ks=(0.5, 0.5, 0.5), urough=0.1, vrough=0.1, remap_roughness=1), mats0[glass]]
    ids0 = tri_materials(b)
    ids1 = ids0.copy()
    ids1[0:100000:2] = 1
    scene = gx.Scene(b)
    dev = torch.device("cuda", scene.device)
    tensors = [torch.from_numpy(x).to(dev) for x in (ids1, ids0)]
    torch.cuda.synchronize(dev)
    one = median_ms(lambda k: scene.update_materials([records[k % 2]], glass), a.calls)
    full = median_ms(lambda k: scene.set_triangle_materials(tensors[k % 2]), a.calls)
    edited = with_record(mats0, glass, records[0])

    def create(k):
        fresh_scene(gx, b, materials=edited, tri_material=ids1).close()

    created = median_ms(create, a.creates)
    print(json.dumps({"scene": "cfg3_100k", "n_triangles": scene.n_triangles, "n_materials": len(mats0), "calls": a.calls, "update_one_material_ms_median": one[0],
                      "update_one_material_ms_min": one[1], "set_triangle_materials_ms_median": full[0], "set_triangle_materials_ms_min": full[1],
                      "scene_create_ms_median": created[0], "scene_create_ms_min": created[1], "creates": a.creates}), flush=True)
    scene.close()


if __name__ == "__main__":
    main()
