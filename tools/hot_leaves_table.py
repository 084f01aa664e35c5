"""Dev tool (no GPU): the leaves that the first 64 4-wide nodes of the benchmark's scene reference -- what k_trace4's hot-leaf region has to hold.
Writes the mesh of scenes.dragon_cornell (cfg 3 and cfg 4 share it: they differ in materials and lights) to a file, builds
tools/hot_leaves_table.cpp with the host compiler against the library's scene compiler and runs it.

usage: python tools/hot_leaves_table.py [n_tris]
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnxraytracer_amd", "csrc")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scenes  # noqa: E402


def main(n_tris):
    b = scenes.dragon_cornell(n_tris, "glass+metal")   # (owns the arrays of its description)
    d = b.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.n_vertices, 3)).astype(np.float32)
    idx = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).astype(np.int32)
    with tempfile.TemporaryDirectory() as td:
        mesh, exe = os.path.join(td, "mesh.bin"), os.path.join(td, "hot_leaves_table")
        with open(mesh, "wb") as f:
            f.write(np.array([len(v), len(idx)], np.int32).tobytes()); f.write(v.tobytes()); f.write(idx.tobytes())
        cxx = shutil.which("g++") or shutil.which("c++")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "hot_leaves_table.cpp"),
                               os.path.join(CSRC, "scene_compile.cpp"), os.path.join(CSRC, "scene_builder.cpp"), "-o", exe, "-lpthread"])
        subprocess.check_call([exe, mesh])


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100000)
