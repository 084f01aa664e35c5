"""The cost-driven 4-wide collapse on the host (scene_compile.cpp, wide_collapse.h), checked by a stand-alone program.

tests/wide_collapse_check.cpp links the library's scene compiler with the host compiler alone, builds seeded soups of 1, 2, 3, 4, 5, 7,
8, 13, 64 and 2 049 triangles and one of geometrically growing triangles (chain cuts), and checks for each: every leaf reachable exactly
once, child boxes equal to their node4_src node's, order byte and 4-bit code of every node and octant against the near-first order
computed by recursion on the binary tree, stack4_need against the longest root path, the summed root area against the two-level rule
(<=) and against an exhaustive search over all cuts (equal, soups of <= 13 triangles), that both shapes of four and cuts of three and
two occur, and that 65 536 triangles on one centroid are refused with the checked error.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnxraytracer_amd", "csrc")


def test_wide_collapse_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "wide_collapse_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "wide_collapse_check.cpp"), os.path.join(CSRC, "scene_compile.cpp"), os.path.join(CSRC, "scene_builder.cpp"),
                           "-o", exe, "-lpthread"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout
