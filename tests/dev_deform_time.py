"""The deformation loop against gnxr_scene_set_geometry, the only earlier route to correct normals on a deformed mesh (dev tool, MI355X):

    python tests/dev_deform_time.py [--calls 11] [--sizes 100000,1000000]

The synthetic mesh in the Cornell box with per-vertex normals, skinned by 32 bones (four weights per vertex) and two blend shapes.  Per
size, in this one process, after one warm-up each, the median and the extremes of `--calls` synchronised calls (host clock around a call
that returns when the device holds its result, or that is followed by a device synchronise):
  (a) skin_vertices                      (b) update_vertices from the device tensor          (c) recompute_normals
  (d) the first recompute_normals of the topology, once: it also builds the vertex -> corner table
  (e) set_geometry with the same vertices and normals computed on the host beforehand (their numpy time is printed apart)
and, between HIP events on one stream, the device work of (a) and (c) beside a plain device copy that moves as many bytes as the kernels
must (each array they read or write counted once; half of the copy's bytes are read, half written).  The gate, of the kind the
environment, media and texture edits used: the slowest (b) + (c) of the run is below the fastest (e) of the same run."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401
import gnxraytracer_amd as gx, scenes
import test_scene_update as tsu

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--sizes", default="100000,1000000")
args = ap.parse_args()
assert args.calls >= 5
gx.init(0)
dev = torch.device("cuda", 0)
f32 = np.float32


def host_normals(v, idx):
    """area-weighted vertex normals with numpy (what a caller of set_geometry computes): (V, 3) per vertex, (T, 9) per-corner rows; a
    vertex whose faces cancel or that no triangle names gets (0, 0, 1)"""
    p = v[idx]
    F = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(f32)
    N = np.zeros_like(v)
    for k in range(3):
        np.add.at(N, idx[:, k], F)
    length = np.linalg.norm(N, axis=1, keepdims=True)
    N = np.where(length > 0, N / np.maximum(length, 1e-30), np.array([0, 0, 1], f32)).astype(f32)
    return N, np.ascontiguousarray(N[idx].reshape(-1, 9), f32)


def wall(fn, calls):
    out = []
    for _ in range(calls + 1):   # the first one is the warm-up
        torch.cuda.synchronize()
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append((time.perf_counter() - t) * 1e3)
    return out[1:]


def events(fn, calls):
    out = []
    for _ in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out[1:]


def fmt(ms):
    return f"{statistics.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


for n in (int(x) for x in args.sizes.split(",")):
    tmp = gx.SceneBuilder()
    tmp.AddModel(scenes.synthetic_mesh_path(n), tmp.MatteMaterial(scenes.WHITE, 60.0))
    mv, midx = tsu.vertices(tmp), tsu.indices(tmp)
    b = gx.SceneBuilder()
    white = b.MatteMaterial(scenes.WHITE, 60.0)
    b.AddCornell(b.MatteMaterial(scenes.RED, 60.0), b.MatteMaterial(scenes.BLUE, 60.0), white)
    first_v = b.desc().n_vertices
    first_t = b.add_mesh(mv, midx, b.add_material(type=gx._abi.MAT_METAL, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), urough=0.1, vrough=0.1, remap_roughness=1),
                         normals=host_normals(mv, midx)[0])
    b.AddAreaLight(white)
    scene = gx.Scene(b)
    v, idx = tsu.vertices(b), tsu.indices(b)
    V, T = len(mv), len(midx)
    counts = np.bincount(midx.reshape(-1), minlength=V)
    rng = np.random.default_rng(1)
    B, M = 32, 2
    bones = np.tile(np.eye(3, 4, dtype=f32), (B, 1, 1)) + rng.normal(size=(B, 3, 4)).astype(f32) * f32(0.01)
    bi = rng.integers(0, B, size=(V, 4)).astype(np.int32)
    bw = rng.random((V, 4), dtype=f32); bw /= bw.sum(1, keepdims=True)
    md = rng.normal(size=(M, V, 3)).astype(f32) * f32(0.005)
    mw = np.array([0.3, 0.6], f32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_rest, d_bi, d_bw, d_bones, d_md, d_mw = t(mv), t(bi), t(bw), t(bones), t(md), t(mw)
    d_out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)

    skin = lambda: gx.skin_vertices(d_rest, d_bi, d_bw, d_bones, d_md, d_mw, out=d_out, stream=stream)
    t_a = wall(skin, args.calls)
    t_b = wall(lambda: scene.update_vertices(d_out, first_vertex=first_v, stream=stream), args.calls)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); scene.recompute_normals(stream=stream); torch.cuda.synchronize(); t_d = (time.perf_counter() - t0) * 1e3
    t_c = wall(lambda: scene.recompute_normals(stream=stream), args.calls)
    ev_a, ev_c = events(skin, args.calls), events(lambda: scene.recompute_normals(stream=stream), args.calls)
    bytes_a = V * (12 + 16 + 16 + 12) + B * 48 + M * (V * 12 + 4)
    nt, nv = scene.n_triangles, scene.n_vertices
    # (c): DTri 48, tri_n read 48 and written 48, corner table 12, corner list 12, face normals 16 written and read; per vertex offsets 4, sums 16 written and read
    bytes_c = nt * (48 + 48 + 48 + 12 + 12 + 32) + nv * (4 + 32)
    copies = {}
    for name, nbytes in (("a", bytes_a), ("c", bytes_c)):
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        copies[name] = events(lambda: dst.copy_(src), args.calls)
        del src, dst
    moved = d_out.cpu().numpy()
    v2 = v.copy(); v2[first_v:first_v + V] = moved
    t0 = time.perf_counter(); rows = host_normals(v2, idx)[1]; t_host2 = (time.perf_counter() - t0) * 1e3
    own = np.zeros(nt, bool); own[first_t:first_t + T] = True
    rows[~own] = 0
    mat = np.ctypeslib.as_array(b.desc().tri_material, shape=(nt,)).copy()
    light = np.ctypeslib.as_array(b.desc().tri_light, shape=(nt,)).copy()
    t_e = wall(lambda: scene.set_geometry(v2, idx, mat, tri_light=light, normals=rows), args.calls)
    bc = [x + y for x, y in zip(t_b, t_c)]
    print(f"{nt} triangles, {nv} vertices ({T} / {V} skinned, {B} bones, {M} blend shapes; valence median {int(np.median(counts))}, max {int(counts.max())}); "
          f"median (min, max) of {args.calls} calls after 1 warm-up", flush=True)
    print(f"  (a) skin_vertices                      {fmt(t_a)}")
    print(f"  (b) update_vertices (device tensor)    {fmt(t_b)}")
    print(f"  (c) recompute_normals                  {fmt(t_c)}")
    print(f"  (d) first recompute_normals            {t_d:9.3f} ms (once: builds the vertex -> corner table)")
    print(f"  (e) set_geometry, host normals given   {fmt(t_e)}   [numpy normals on the host: {t_host2:.1f} ms, not included]")
    print(f"  (b) + (c) per call                     {fmt(bc)}")
    for name, ev, nbytes in (("a", ev_a, bytes_a), ("c", ev_c, bytes_c)):
        k, c = statistics.median(ev), statistics.median(copies[name])
        print(f"  ({name}) between events {k:8.3f} ms (min {min(ev):.3f}) for {nbytes / 1e6:.1f} MB = {nbytes / k / 1e6:.0f} GB/s; device copy moving as many bytes {c:.3f} ms "
              f"(min {min(copies[name]):.3f}); ratio {k / c:.2f}")
    print(f"  gate: slowest (b) + (c) {max(bc):.3f} ms < fastest (e) {min(t_e):.3f} ms: {'holds' if max(bc) < min(t_e) else 'DOES NOT HOLD'}", flush=True)
    del scene
