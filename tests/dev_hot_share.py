"""Dev tool: the share of k_trace4's triangle loads that the block's LDS copy of the hot leaves serves (gnxr_scene_hot_leaf_counts), on
the benchmark's scenes at its resolution, through the counting 4-wide walk (gnxr_set_profiling(4)): a run of its own, never a timed one.

usage: python tests/dev_hot_share.py [cfg3|cfg4 ...] [--spp N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before libgnxr.so is loaded)

import gnxraytracer_amd as gx  # noqa: E402
import scenes  # noqa: E402


def main(argv):
    spp = int(argv[argv.index("--spp") + 1]) if "--spp" in argv else 32
    workloads = [a for a in argv if a in ("cfg3", "cfg4")] or ["cfg3", "cfg4"]
    gx.init(0)
    for wl in workloads:
        env = scenes.synthetic_env_path(1000, 500) if wl == "cfg4" else None
        b = scenes.dragon_cornell(100000, "zoo" if wl == "cfg4" else "glass+metal", env=env)
        scene = gx.Scene(b)
        integ = gx.PathIntegrator(8, 1.0, "spatial")
        gx.lib().gnxr_set_profiling(4)
        try:
            _, st = integ.Render(scene, 1920, 1080, spp)
        finally:
            gx.lib().gnxr_set_profiling(0)
        hot, loaded = scene.hot_leaf_counts()
        rays = st["rays_closest"] + st["rays_any"]
        print(f"{wl} {spp} spp at 1920 x 1080: {rays} rays, {st['nodes_visited']} node visits ({st['nodes_from_memory']} from memory), "
              f"{loaded} triangles loaded = {loaded / rays:.3f} per ray, {hot} of them from LDS = {hot / max(1, loaded):.4f}, {st['leaf_retests']} leaf re-tests")


if __name__ == "__main__":
    main(sys.argv[1:])
