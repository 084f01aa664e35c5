"""All-hits ray queries (include/gnxr.h, "All-hits ray queries"): the numpy restatement (tests/allhits_reference.py) pinned to the oracle's
Intersect on one-triangle scenes and on hand-made cases, then gnxr_trace_all_device / gnxr_trace_all and Scene.all_hits / count_hits /
contains / signed_distance on the GPU against the restatement's brute force over all triangles.  Every comparison of records and counts
is on their bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import allhits_reference as ar
import scenes
from conftest import ROOT
from query_cases import binary_depth, chain_scene, concentric_mesh, dragon, mesh_of, mesh_scene

ERR_INVALID = -1
F = np.float32
INF = F(np.inf)


# ---------------------------------------------------------------- helpers
def rays_of(o, d, tmax=np.inf):
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    r = np.zeros((len(o), 8), F)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o, tmax, d
    return r


def device_lists(scene, rays, K, **kw):
    """(records (n, K) as RECORD, counts) of Scene.all_hits after the stream has finished"""
    res = scene.all_hits(torch.from_numpy(np.array(rays, F)).cuda(), K, **kw)
    torch.cuda.synchronize()
    return res.records.cpu().numpy().view(ar.RECORD).reshape(len(rays), K), res.count.cpu().numpy()


def assert_same(got, want):
    """records and counts, each on bytes"""
    (grec, gcnt), (wrec, wcnt) = got, want
    assert gcnt.dtype == np.int32 and gcnt.shape == wcnt.shape
    if gcnt.tobytes() != wcnt.tobytes():
        bad = np.flatnonzero(gcnt != wcnt)
        raise AssertionError(f"{len(bad)} of {len(wcnt)} counts differ; first {bad[0]}: got {gcnt[bad[0]]}, want {wcnt[bad[0]]}")
    assert grec.shape == wrec.shape and grec.dtype.itemsize == 16
    if grec.tobytes() != wrec.tobytes():
        bad = np.flatnonzero((grec.view(np.uint8).reshape(len(grec), -1) != wrec.view(np.uint8).reshape(len(wrec), -1)).any(axis=1))
        raise AssertionError(f"rows of {len(bad)} of {len(wrec)} rays differ; first {bad[0]} (count {wcnt[bad[0]]}): got {grec[bad[0]]}, want {wrec[bad[0]]}")


def aimed_rays(lo, hi, n, rng, scale=2.0):
    """from a shell around [lo, hi] through points inside it: rays that cross the whole scene"""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = c + scale * np.linalg.norm(h) * d
    target = rng.uniform(c - h, c + h, (n, 3))
    return rays_of(o, target - o)


class Case:
    """a mesh, a ray set and the pair tables of the brute force: computed once, shared, never written"""
    def __init__(self, v, idx, rays):
        self.v, self.idx, self.rays = v, idx, rays
        self.tables = ar.pair_tables(v, idx, rays)
        for x in (v, idx, rays) + tuple(self.tables):
            x.setflags(write=False)
        self._want = {}

    def want(self, K):
        if K not in self._want:
            self._want[K] = ar.all_hits(self.v, self.idx, self.rays, K, tables=self.tables)
        return self._want[K]


_cases = {}


def case(name):
    if name not in _cases:
        rng = np.random.default_rng(31)
        if name == "cornell":
            v, idx = mesh_of(scenes.cornell())
        else:
            v, idx = mesh_of(dragon())
        lo, hi = v.min(axis=0), v.max(axis=0)
        rays = np.concatenate([np.array(scenes.random_rays(2048, seed=7), F).reshape(-1, 8), aimed_rays(lo, hi, 512, rng)])
        rays[::5, 3] = rng.uniform(0.5, 4.0, len(rays[::5]))   # a fifth with a finite tmax inside the scene
        _cases[name] = Case(v, idx, rays)
    return _cases[name]


_deep_tree_cache = []


def deep_tree_case(gx):
    """(rays, brute force with K = 32) of chain_scene(36): rays along and around the x axis through the chain; computed once, shared, never
    written"""
    if not _deep_tree_cache:
        v, idx = mesh_of(chain_scene(gx))
        rng = np.random.default_rng(8)
        n = 1024
        # from just beyond the small end, so that the watertight test's error bound (which grows with the distance) keeps every triangle
        o = np.stack([-(2.0 ** -rng.uniform(30, 44, n)), np.zeros(n), np.zeros(n)], axis=1)
        o[:64, 0] = -(2.0 ** -40)
        d = np.stack([np.ones(n), np.zeros(n), np.zeros(n)], axis=1)
        o[64:, 1:] = rng.normal(0, 0.2, (n - 64, 2)) * 2.0 ** -rng.uniform(0, 40, (n - 64, 1))   # off the axis: the small triangles are missed
        d[512:, 1:] = rng.normal(0, 0.1, (n - 512, 2))
        rays = rays_of(o, d)
        want = ar.all_hits(v, idx, rays, 32)
        for x in (rays,) + tuple(want):
            x.setflags(write=False)
        _deep_tree_cache.extend([rays, want])
    return _deep_tree_cache


def box_mesh_closed(lo=(-1, -1, -1), hi=(1, 1, 1)):
    return scenes.box_mesh(lo, hi)


def sphere_mesh(radius=1.0, n_lat=16, n_lon=32):
    """a closed latitude / longitude tessellation with its vertices on the sphere (so it lies inside it, by at most radius (1 - cos(pi / 32)))"""
    v = [(0.0, 0.0, radius)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
    v.append((0.0, 0.0, -radius))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    idx = []
    for j in range(n_lon):
        idx.append((0, ring(1, j), ring(1, j + 1)))
        idx.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            idx.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            idx.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return np.array(v, F), np.array(idx, np.int32)


def contain_points(kind, n=1536, seed=41):
    """seeded points in 1.5 x the extent, kept 1 % of the extent (0.02) or more off the analytic surface, and the analytic answer"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.5, 1.5, (3 * n, 3)).astype(F)
    signed = np.abs(p.astype(np.float64)).max(axis=1) - 1 if kind == "cube" else np.linalg.norm(p.astype(np.float64), axis=1) - 1
    keep = np.abs(signed) >= 0.02
    return p[keep][:n], (signed[keep][:n] < 0)


def parity_rays(points, direction):
    return rays_of(points, np.broadcast_to(np.array(direction, F), points.shape))


def reference_parity(v, idx, points, direction):
    return (ar.all_hits(v, idx, parity_rays(points, direction), 0)[1] & 1).astype(np.uint8)


# ---------------------------------------------------------------- CPU
def test_symbols_and_records(gx):
    lib = C.CDLL(gx.LIB_PATH)
    for name in ("gnxr_trace_all_device", "gnxr_trace_all_counted_device", "gnxr_trace_all"):
        assert hasattr(lib, name) and name in gx._abi.PROTOTYPES
    assert C.sizeof(gx._abi.RayHit) == 16 and gx._abi.RayHit not in gx._abi.ABI_STRUCTS
    assert gx.RAY_HIT_DTYPE == ar.RECORD and gx.ALL_HITS_MAX == 32
    assert gx.CONTAINS_DIRECTION == (0.8017837, 0.5345225, 0.26726124)
    for m in ("all_hits", "count_hits", "contains", "signed_distance"):
        assert callable(getattr(gx.Scene, m))


def oracle_rays(tri, rng, n=512):
    """rays for one triangle: aimed at points of it (hits), past it (misses), grazing its edges, exactly at vertices and edge midpoints,
    axis-parallel through it, a quarter with a finite tmax around the hit distance"""
    a, b, c = tri.astype(np.float64)
    size = max(np.linalg.norm(b - a), np.linalg.norm(c - a))
    w = rng.dirichlet((1, 1, 1), n)
    kind = np.arange(n) % 8
    w[kind == 1] = w[kind == 1] * 1.6 - 0.2                       # around the triangle: hits and misses
    edge = rng.integers(0, 3, n)
    s = rng.uniform(0, 1, n)
    on_edge = np.zeros((n, 3))
    on_edge[np.arange(n), edge] = s
    on_edge[np.arange(n), (edge + 1) % 3] = 1 - s
    graze = on_edge + rng.choice([0.0, 1e-7, -1e-7, 1e-5, -1e-5], (n, 1)) * rng.normal(size=(n, 3))
    w[kind == 2] = graze[kind == 2]                               # grazing an edge
    w[kind == 3] = on_edge[kind == 3]                             # exactly on an edge (as far as fp32 goes)
    corner = np.eye(3)[rng.integers(0, 3, n)]
    w[kind == 4] = corner[kind == 4]                              # at a vertex
    target = w @ np.stack([a, b, c])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    d[kind == 5] = axis[kind == 5]                                # axis-parallel: two zero direction components
    d[kind == 6, rng.integers(0, 3)] = 0.0                        # one zero component
    dist = size * rng.uniform(0.5, 3.0, (n, 1))
    o = (target - dist * d).astype(F)
    exact = (kind == 4) | (kind == 3)
    dd = np.where(exact[:, None], (target.astype(F) - o).astype(F), d.astype(F))   # aimed in fp32 at the fp32 target
    tmax = np.full(n, np.inf)
    q = rng.integers(0, 4, n) == 0
    tmax[q] = (dist[:, 0] / np.where(exact, dist[:, 0], 1.0))[q] * rng.choice([0.5, 0.999999, 1.0, 1.000001, 2.0], q.sum())
    return rays_of(o, dd, tmax)


def test_restatement_matches_the_oracle(gx):
    """64 seeded triangles, 512 rays each.  A one-triangle scene is a one-leaf tree whose box is the triangle's own: the oracle's Intersect
    tests exactly the own box, then the triangle.  Its decision, prim, t, b1 and b2 must equal the restatement's on bits.  A third of the
    triangles translated to (1000, 1000, 1000), a third scaled by 2^-20."""
    import oracle_lib as ol
    rng = np.random.default_rng(2026)
    n_hits = n_edge = 0
    for k in range(64):
        tri = rng.uniform(-1, 1, (3, 3)) * rng.choice([1.0, 0.1, 1e-3])
        if k % 8 == 7:
            tri[:, rng.integers(0, 3)] = tri[0, 0]                # axis-aligned: a flat own box
        tri = ((tri + (1000.0 if k % 3 == 1 else 0.0)) * (2.0 ** -20 if k % 3 == 2 else 1.0)).astype(F)
        rays = oracle_rays(tri, rng)
        idx = np.array([(0, 1, 2)], np.int32)
        own_box, hit_tri, t, b1, b2 = ar.pair_tables(tri, idx, rays)
        want = (own_box & hit_tri)[:, 0]
        got = ol.OracleScene(mesh_scene(gx, tri, idx)).Intersect(rays)
        assert ((got["prim"] >= 0) == want).all(), (k, np.flatnonzero((got["prim"] >= 0) != want)[:8])
        assert (got["prim"][want] == 0).all()
        for name, mine in (("t", t), ("b1", b1), ("b2", b2)):
            assert (got[name][want].view(np.uint32) == mine[want, 0].view(np.uint32)).all(), (k, name)
        n_hits += int(want.sum())
        n_edge += int((want & ((b1[:, 0] == 0) | (b2[:, 0] == 0) | (b1[:, 0] + b2[:, 0] == 1))).sum())
    assert n_hits > 64 * 100 and n_edge > 64   # the set hits, misses, and lands on edges and vertices


def sheets(n=40, copies_of=5, copies=2):
    """n parallel unit quads at z = 0.1 k (two triangles each) and `copies` exactly coincident copies of quad `copies_of` behind them"""
    v, idx = [], []
    for z in [0.1 * k for k in range(n)] + [0.1 * copies_of] * copies:
        base = len(v)
        v += [(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)]
        idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return np.array(v, F), np.array(idx, np.int32)


def sheet_rays(rng, n=256):
    """up through the stack, slightly tilted, with a tmax that ends after 0 .. 40 sheets or never"""
    o = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), np.full(n, -1.0)], axis=1)
    d = np.stack([rng.normal(0, 0.01, n), rng.normal(0, 0.01, n), np.ones(n)], axis=1)
    tmax = np.where(np.arange(n) % 4 == 0, np.inf, 1.0 + 0.1 * rng.integers(-1, 40, n) + 0.05)
    return rays_of(o, d, tmax)


def test_hand_cases():
    v, idx = sheets()
    # straight up through everything: 40 sheets + 2 copies, one triangle of each quad
    rec, cnt = ar.all_hits(v, idx, rays_of([(0.3, -0.2, -1)], [(0, 0, 1)]), 32)
    assert cnt[0] == 42
    t, prim = rec["t"][0], rec["prim"][0]
    assert (np.diff(t) >= 0).all() and t[0] == 1
    # the three coincident quads at z = 0.5: bit-equal t, ascending authoring index (quad 5, then the copies 40 and 41)
    same = np.flatnonzero(t == t[5])
    assert list(same) == [5, 6, 7] and list(prim[same] // 2) == [5, 40, 41]
    # tmax between sheets 2 and 3 (t = 1.2, 1.3): three hits; K = 1 keeps the nearest and the count stays 3
    rec, cnt = ar.all_hits(v, idx, rays_of([(0.3, -0.2, -1)], [(0, 0, 1)], 1.25), 1)
    assert cnt[0] == 3 and rec["prim"][0, 0] // 2 == 0
    rec, cnt = ar.all_hits(v, idx, rays_of([(0.3, -0.2, -1)], [(0, 0, 1)], 1.25), 4)
    assert cnt[0] == 3 and rec[0, 3].tobytes() == ar.EMPTY.tobytes() and rec["prim"][0, 2] // 2 == 2
    # every class of invalid ray, and the tmax values that fall out of the arithmetic
    o, d = (0.3, -0.2, -1.0), (0.0, 0.0, 1.0)
    bad = np.concatenate([rays_of([(np.nan, 0, -1)], [d]), rays_of([(np.inf, 0, -1)], [d]), rays_of([o], [(0, np.nan, 1)]), rays_of([o], [(0, -np.inf, 1)]),
                          rays_of([o], [d], np.nan), rays_of([o], [(0, 0, 0)]), rays_of([o], [d], 0.0), rays_of([o], [d], -3.0)])
    rec, cnt = ar.all_hits(v, idx, bad, 2)
    assert (cnt == 0).all() and all(r.tobytes() == ar.EMPTY.tobytes() for r in rec.reshape(-1))
    assert ar.all_hits(v, idx, rays_of([o], [d], np.inf), 0)[1][0] == 42
    # no triangles
    rec, cnt = ar.all_hits(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), rays_of([o], [d]), 2)
    assert cnt[0] == 0 and rec[0, 1].tobytes() == ar.EMPTY.tobytes()


def test_bad_arguments_without_a_device(gx):
    """A null scene, a null pointer with n > 0, n < 0, max_hits outside [0, 32] and a hits array that does not go with max_hits are
    refused before anything is looked at (the handle is a dummy)."""
    L = gx.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    for fn in (L.gnxr_trace_all_device, lambda s, r, n, k, h, c, st: L.gnxr_trace_all_counted_device(s, r, n, k, h, c, p, st)):
        assert fn(None, p, 1, 1, p, p, None) == ERR_INVALID
        assert fn(None, p, 0, 1, p, p, None) == ERR_INVALID
        assert fn(p, None, 4, 1, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 1, None, p, None) == ERR_INVALID      # hits missing with max_hits > 0
        assert fn(p, p, 4, 1, p, None, None) == ERR_INVALID
        assert fn(p, p, 4, 0, p, p, None) == ERR_INVALID         # hits set with max_hits == 0
        assert fn(p, p, -1, 1, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, 33, p, p, None) == ERR_INVALID
        assert fn(p, p, 4, -1, p, p, None) == ERR_INVALID
        assert fn(p, p, 0, 33, p, p, None) == ERR_INVALID        # n == 0 is a no-op only for good arguments
    assert L.gnxr_trace_all_counted_device(p, p, 4, 1, p, p, None, None) == ERR_INVALID
    R, H, I = (lambda x: C.cast(x, C.POINTER(gx._abi.Ray))), (lambda x: C.cast(x, C.POINTER(gx._abi.RayHit))), (lambda x: C.cast(x, C.POINTER(C.c_int32)))
    assert L.gnxr_trace_all(None, R(p), 1, 1, H(p), I(p)) == ERR_INVALID
    assert L.gnxr_trace_all(p, None, 1, 1, H(p), I(p)) == ERR_INVALID
    assert L.gnxr_trace_all(p, R(p), 1, 1, None, I(p)) == ERR_INVALID
    assert L.gnxr_trace_all(p, R(p), 1, 0, H(p), I(p)) == ERR_INVALID
    assert L.gnxr_trace_all(p, R(p), -1, 1, H(p), I(p)) == ERR_INVALID
    assert L.gnxr_trace_all(p, R(p), 1, 33, H(p), I(p)) == ERR_INVALID


def test_python_refuses_other_inputs_before_the_library(gx):
    """Only contiguous float32 (n, 8) rays / (n, 3) points on the scene's device pass, max_hits is an integer in [0, 32], and the launch
    keywords are `stream` and `counts`; everything else raises before a library call (the handle is empty: a call would fail differently)."""
    s = object.__new__(gx.Scene)
    s._h, s.device = None, 0
    bad = [np.zeros((4, 8), F), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 7)), torch.zeros((8, 4)).t(), torch.zeros((4, 16))[:, ::2],
           torch.zeros(32), "rays", None, torch.zeros((4, 8))]
    for b in bad:
        with pytest.raises(ValueError):
            s.all_hits(b, 4)
        with pytest.raises(ValueError):
            s.count_hits(b)
    for b in [np.zeros((4, 3), F), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 4)), torch.zeros((3, 4)).t(), "points", None, torch.zeros((4, 3))]:
        with pytest.raises(ValueError):
            s.contains(b)
        with pytest.raises(ValueError):
            s.signed_distance(b)
    for k in (33, -1):
        with pytest.raises(ValueError):
            s.all_hits(torch.zeros((4, 8)), k)
    for k in (1.5, "4", None, True):
        with pytest.raises(TypeError):
            s.all_hits(torch.zeros((4, 8)), k)
    for method, args in ((s.all_hits, (torch.zeros((4, 8)), 4)), (s.count_hits, (torch.zeros((4, 8)),)), (s.contains, (torch.zeros((4, 3)),)),
                         (s.signed_distance, (torch.zeros((4, 3)),))):
        with pytest.raises(ValueError, match="unexpected arguments"):
            method(*args, streams=None)
    with pytest.raises(ValueError, match="unexpected arguments"):
        s.signed_distance(torch.zeros((4, 3)), counts=torch.zeros(3, dtype=torch.int64))


def test_no_scratch(gx):
    """tools/kernel_regs.py: every instantiation of k_all_hits (wide / binary, list / count-only, timed / counting) runs without scratch
    and without spilled VGPRs -- the list lives in the output row, not in a private array"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    ks = [k for k in kernel_regs.kernels(gx.LIB_PATH) if "k_all_hits<" in k["name"]]
    assert len(ks) == 8, [k["name"] for k in ks]
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in ks), ks


@pytest.mark.parametrize("kind", ["cube", "sphere"])
def test_containment_reference_is_right(gx, kind):
    """The reference's parity along CONTAINS_DIRECTION agrees with the analytic answer for every point of the seeded set (kept 1 % of
    the extent off the surface; the sphere's tessellation lies inside the sphere by less than that), so the GPU test below compares the
    device with a reference known to be right."""
    v, idx = box_mesh_closed() if kind == "cube" else sphere_mesh()
    p, inside = contain_points(kind)
    assert len(p) == 1536 and 0.1 < inside.mean() < 0.9
    assert (reference_parity(v, idx, p, gx.CONTAINS_DIRECTION) == inside).all()


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 1, 4, 32])
def test_cornell(gpu, K):
    """scenes.cornell() and the 2 k mesh in its box: 2048 random rays and 512 from outside aimed through the box"""
    for name, b in (("cornell", scenes.cornell()), ("dragon", dragon())):
        c = case(name)
        want = c.want(K)
        assert len(c.rays) == 2560 and want[1].max() >= (4 if name == "dragon" else 2) and (want[1] == 0).any()
        scene = gpu.Scene(b)
        assert_same(device_lists(scene, c.rays, K), want)
        if K == 4:   # the host entry point walks the same way, and count_hits is the K = 0 form
            hits, counts = scene.AllHits(c.rays, K)
            assert_same((hits.view(ar.RECORD), counts), want)
            n = scene.count_hits(torch.from_numpy(np.array(c.rays)).cuda())
            torch.cuda.synchronize()
            assert n.dtype == torch.int32 and n.cpu().numpy().tobytes() == want[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal_counts"])
def test_split_methods(gpu, split):
    """the lists do not depend on the tree: one expected array for all four split methods"""
    c = case("dragon")
    assert_same(device_lists(gpu.Scene(dragon(split)), c.rays, 8), c.want(8))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 32])
def test_overflow_and_ties(gpu, K):
    """40 parallel quads and two exactly coincident copies of one: count > K, count == K and count < K all occur, the coincident
    triangles are both kept in authoring order, and the empty slots are (+inf, -1, 0, 0)"""
    v, idx = sheets()
    rays = sheet_rays(np.random.default_rng(12))
    want = ar.all_hits(v, idx, rays, K)
    rec, cnt = want
    assert (cnt > K).any() and (cnt == K).any() and (cnt < K).any() and cnt.max() == 42
    if K == 32:
        assert ((rec["t"][:, 1:] == rec["t"][:, :-1]) & (rec["prim"][:, 1:] > rec["prim"][:, :-1]) & (rec["prim"][:, :-1] >= 0)).any()   # a tie, in order
    short = np.flatnonzero(cnt < K)
    assert all(rec[i, cnt[i]:].tobytes() == np.full(K - cnt[i], ar.EMPTY, ar.RECORD).tobytes() for i in short)
    assert_same(device_lists(gpu.Scene(mesh_scene(gpu, v, idx)), rays, K), want)


def degenerate_rays(v, idx, rng):
    lo, hi = v.min(axis=0), v.max(axis=0)
    inside = lambda n: rng.uniform(lo, hi, (n, 3))
    parts = []
    # zero direction components with origins exactly on the planes of the walls (the bounds of the box), in and across the plane
    for axis in range(3):
        for bound in (lo, hi):
            o = inside(24)
            o[:, axis] = bound[axis]
            d = rng.normal(size=(24, 3))
            d[:12, axis] = 0.0                       # in the plane
            d[12:] = 0.0
            d[12:18, axis] = 1.0                     # along the axis, off the wall
            d[18:, axis] = -1.0
            parts.append(rays_of(o, d))
    # axis-parallel rays and rays with one zero component from inside
    o, d = inside(96), rng.normal(size=(96, 3))
    d[:48] = np.eye(3)[rng.integers(0, 3, 48)] * rng.choice([-1.0, 1.0], (48, 1))
    d[48:, 0] = 0.0
    parts.append(rays_of(o, d))
    # direction components of 1e-42: 1 / d overflows
    o, d = inside(96), rng.normal(size=(96, 3))
    d[np.arange(96), rng.integers(0, 3, 96)] = rng.choice([1e-42, -1e-42], 96)
    d[:24] = np.stack([np.full(24, 1e-42), np.full(24, -1e-42), rng.choice([-1.0, 1.0], 24)], axis=1)   # two of them (never all three: t would be a NaN)
    d[np.abs(d).max(axis=1) < 1e-30, 2] = 1.0
    parts.append(rays_of(o, d))
    # along shared edges and through shared vertices
    a, b = v[idx[:, 0]], v[idx[:, 1]]
    parts.append(rays_of(a, b - a))
    parts.append(rays_of(a - (b - a), b - a))
    o = inside(len(v) * 2)
    parts.append(rays_of(o, np.tile(v, (2, 1)).astype(F) - o.astype(F)))
    # tmax in {0, negative, +inf, NaN}, a NaN origin, a zero direction
    o, d = inside(64), rng.normal(size=(64, 3))
    r = rays_of(o, d, np.tile([0.0, -2.0, np.inf, np.nan], 16))
    r[60, 0] = np.nan
    r[61, 4:7] = 0.0
    r[62, 5] = np.inf
    parts.append(r)
    return np.concatenate(parts)


@pytest.mark.gpu
def test_degenerate_rays(gpu):
    b = scenes.cornell()
    v, idx = mesh_of(b)
    rays = degenerate_rays(v, idx, np.random.default_rng(13))
    want = ar.all_hits(v, idx, rays, 8)
    assert (want[1] > 0).mean() > 0.3 and (want[1][-64:] == 0).sum() >= 48
    scene = gpu.Scene(b)
    assert_same(device_lists(scene, rays, 8), want)
    assert_same(device_lists(scene, rays, 0), ar.all_hits(v, idx, rays, 0))
    # the same rays through the 2 k mesh: deeper trees, the flagged rays' node test at every level
    c = case("dragon")
    rays = degenerate_rays(c.v, c.idx[-12:], np.random.default_rng(14))
    assert_same(device_lists(gpu.Scene(dragon()), rays, 8), ar.all_hits(c.v, c.idx, rays, 8))


@pytest.mark.gpu
def test_translated_mesh(gpu):
    """The 2 k mesh at (1000, 1000, 1000), where an ulp is 6e-5: boxes and slab products round coarsely, and the own-box test decides"""
    v, idx = mesh_of(dragon())
    idx = idx[:len(idx) - 12]   # the mesh without the box and its light
    used = np.unique(idx)
    v = (v[used] + F(1000)).astype(F)
    idx = np.searchsorted(used, idx).astype(np.int32)
    rng = np.random.default_rng(22)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rays = np.concatenate([aimed_rays(lo, hi, 1024, rng, 1.2), rays_of(rng.uniform(lo, hi, (1024, 3)), rng.normal(size=(1024, 3)))])
    want = ar.all_hits(v, idx, rays, 8)
    assert want[1].max() >= 4
    for split in ("sah", "hlbvh"):
        assert_same(device_lists(gpu.Scene(mesh_scene(gpu, v, idx, split)), rays, 8), want)


@pytest.mark.gpu
def test_deep_tree(gpu):
    """chain_scene(36): rays along the x axis pass through all 36 triangles with a sibling on the stack per level.  Run with the default
    LDS levels, where the tree's need exceeds them (the global spill carries the rest), and forced onto 2 LDS levels through
    GNXR_ALLHITS_LDS_LEVELS, the launch's knob."""
    rays, want = deep_tree_case(gpu)
    assert (want[1][:64] == 36).all() and (want[1] > 32).sum() > 64 and len(set(want[1])) > 20
    scene = gpu.Scene(chain_scene(gpu))
    assert scene.bvh4()[2] > 16, scene.bvh4()[2]   # more than the default LDS levels
    assert_same(device_lists(scene, rays, 32), want)
    os.environ["GNXR_ALLHITS_LDS_LEVELS"] = "2"
    try:
        assert_same(device_lists(scene, rays, 32), want)
        c = case("dragon")
        assert_same(device_lists(gpu.Scene(dragon()), c.rays, 4), c.want(4))
    finally:
        del os.environ["GNXR_ALLHITS_LDS_LEVELS"]


@pytest.mark.gpu
def test_deep_binary_tree_spills(gpu):
    """test_deep_tree's chain and rays on a scene kept on the binary tree by the creation switch, with 2 LDS levels: the binary walk, its
    LDS levels and its global spill together.  chain_scene(36) creates (its depth stays inside the 64-entry limit of scene creation)."""
    rays, want = deep_tree_case(gpu)
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        scene = gpu.Scene(chain_scene(gpu))
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    assert binary_depth(scene) + 2 > 2   # the walk's bound on this tree against the LDS levels below: the spill carries the rest
    os.environ["GNXR_ALLHITS_LDS_LEVELS"] = "2"
    try:
        assert_same(device_lists(scene, rays, 32), want)
    finally:
        del os.environ["GNXR_ALLHITS_LDS_LEVELS"]


@pytest.mark.gpu
def test_off_the_wide_tree(gpu):
    rng = np.random.default_rng(9)
    v, idx = concentric_mesh(rng)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rays = np.concatenate([aimed_rays(lo, hi, 1024, rng, 1.2), rays_of(rng.uniform(-1, 1, (1024, 3)), rng.normal(size=(1024, 3)))])
    want = ar.all_hits(v, idx, rays, 32)
    assert want[1].max() > 32
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    _, meta, _ = scene.bvh()
    assert meta[:, 1].max() > 127   # a leaf the 4-wide encoding cannot hold: the scene is on the binary walk
    assert_same(device_lists(scene, rays, 32), want)
    assert_same(device_lists(scene, rays, 0), ar.all_hits(v, idx, rays, 0))
    # and a scene kept on the binary tree by the creation switch
    os.environ["GNXR_BINARY_BVH"] = "1"
    try:
        binary = gpu.Scene(dragon())
    finally:
        del os.environ["GNXR_BINARY_BVH"]
    c = case("dragon")
    assert_same(device_lists(binary, c.rays, 4), c.want(4))


@pytest.mark.gpu
def test_live_scene(gpu):
    """update_vertices (a sine deformation from a device tensor) -> the brute force over the new vertices; rebuild_bvh -> the same bytes;
    set_geometry with another triangle count -> the brute force over the new mesh"""
    c = case("dragon")
    rays = c.rays[:1024]
    b = dragon()
    v, idx = mesh_of(b)
    scene = gpu.Scene(b)
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(0.15) * np.sin(F(5) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    scene.update_vertices(torch.from_numpy(v2[:n_mesh_v].copy()).cuda())
    want2 = ar.all_hits(v2, idx, rays, 4)
    assert want2[0].tobytes() != ar.all_hits(c.v, c.idx, rays, 4, tables=tuple(t[:1024] for t in c.tables))[0].tobytes()
    assert_same(device_lists(scene, rays, 4), want2)
    scene.rebuild_bvh()
    assert_same(device_lists(scene, rays, 4), want2)
    rng = np.random.default_rng(11)
    v3 = rng.uniform(-2, 2, (900, 3)).astype(F)
    v3[1::3] = v3[0::3] + rng.uniform(-0.6, 0.6, (300, 3)).astype(F)
    v3[2::3] = v3[0::3] + rng.uniform(-0.6, 0.6, (300, 3)).astype(F)
    idx3 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    tri_light = np.full(300, -1, np.int32)
    n_lights = b.desc().n_lights
    tri_light[:n_lights] = np.arange(n_lights)   # every area light keeps exactly one triangle
    scene.set_geometry(v3, idx3, np.zeros(300, np.int32), tri_light=tri_light)
    want3 = ar.all_hits(v3, idx3, rays, 4)
    assert want3[1].max() >= 2
    assert_same(device_lists(scene, rays, 4), want3)


@pytest.mark.gpu
def test_first_hit_is_intersect(gpu):
    """Slot 0 of K = 1 is Scene.intersect's hit: prim, t, b1 and b2 on bits.  The set keeps the rays for which the reference shows that
    the own-box test never overrules an accepting triangle test (then no wider leaf box does either, the slab test being monotone in
    the box), so both calls decide on the triangle test alone."""
    c = case("dragon")
    own_box, tri = c.tables[0], c.tables[1]
    keep = ~(tri & ~own_box).any(axis=1)
    assert keep.mean() > 0.99
    rays = np.array(c.rays[keep])
    want = ar.all_hits(c.v, c.idx, rays, 1, tables=tuple(t[keep] for t in c.tables))
    scene = gpu.Scene(dragon())
    rec, cnt = device_lists(scene, rays, 1)
    assert_same((rec, cnt), want)
    hit = scene.intersect(torch.from_numpy(rays).cuda())
    torch.cuda.synchronize()
    h = hit.hits.cpu().numpy()
    prim = h.view(np.int32)[:, 0]
    assert (cnt > 0).sum() > 1500 and (cnt == 0).any()
    assert (prim == rec["prim"][:, 0]).all()
    m = cnt > 0
    for got, name in ((h[:, 1], "t"), (h[:, 3], "b1"), (h[:, 4], "b2")):
        assert (got[m].view(np.uint32) == rec[name][m, 0].view(np.uint32)).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "sphere"])
def test_contains_and_signed_distance(gpu, kind):
    v, idx = box_mesh_closed() if kind == "cube" else sphere_mesh()
    p, inside = contain_points(kind)
    scene = gpu.Scene(mesh_scene(gpu, v, idx))
    pts = torch.from_numpy(p).cuda()

    def check(v_now, analytic, where=slice(None)):
        want = reference_parity(v_now, idx, p, gpu.CONTAINS_DIRECTION)
        assert (want == analytic)[where].all()
        got = scene.contains(pts)
        sd = scene.signed_distance(pts)
        near = scene.closest_point(pts)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.tobytes()
        chain = torch.where(got != 0, -1.0, 1.0) * torch.sqrt(near.dist2)   # the chain of public calls
        assert sd.dtype == torch.float32 and chain.dtype == torch.float32 and sd.cpu().numpy().tobytes() == chain.cpu().numpy().tobytes()
        assert ((sd.cpu().numpy() < 0) == (want != 0)).all()
        # another direction answers the same question
        other = scene.contains(pts, direction=(-0.3, 0.9, 0.2))
        torch.cuda.synchronize()
        assert other.cpu().numpy().tobytes() == reference_parity(v_now, idx, p, (-0.3, 0.9, 0.2)).tobytes()
    check(v, inside)
    if kind == "cube":   # a refit that turns the cube into a sheared box
        v2 = v.copy()
        v2[:, 0] += F(0.5) * v[:, 1]
        scene.update_vertices(torch.from_numpy(v2).cuda())
        q = p.astype(np.float64)
        q[:, 0] -= 0.5 * q[:, 1]
        clear = np.abs(np.abs(q).max(axis=1) - 1) > 1e-4   # (the shear moves a few points of the set up to the surface)
        assert clear.mean() > 0.99
        check(v2, np.abs(q).max(axis=1) < 1, clear)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_batch_sizes_and_out(gpu, n):
    c = case("dragon")
    scene = gpu.Scene(dragon())
    rays = torch.from_numpy(np.array(c.rays[:n])).cuda()
    out = torch.full((n, 4, 4), 7.0, device="cuda")
    counts_out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    for _ in range(2):   # the second call reuses what the first wrote
        res = scene.all_hits(rays, 4, out=out, counts_out=counts_out)
        torch.cuda.synchronize()
        assert res.records is out and res.count is counts_out and res.t.shape == (n, 4) and res.prim.shape == (n, 4) and res.b.shape == (n, 4, 2)
        want = c.want(4)
        assert_same((out.cpu().numpy().view(ar.RECORD).reshape(n, 4), counts_out.cpu().numpy()), (want[0][:n], want[1][:n]))
    assert (res.prim.cpu().numpy() == want[0]["prim"][:n]).all() and (res.b.cpu().numpy()[:, :, 1] == want[0]["b2"][:n]).all()
    hits, counts = scene.AllHits(c.rays[:n], 4)
    assert hits.shape == (n, 4) and counts.shape == (n,)
    with pytest.raises(ValueError):
        scene.all_hits(rays, 4, out=torch.zeros((n + 1, 4, 4), device="cuda"))
    with pytest.raises(ValueError):
        scene.all_hits(rays, 4, counts_out=torch.zeros((n + 1,), dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
def test_streams(gpu):
    """Rays written by torch on a side stream, answered there and reduced there with no synchronise in between: the null stream's bytes"""
    c = case("dragon")
    scene = gpu.Scene(dragon())
    src = torch.from_numpy(np.array(c.rays)).cuda()
    null = device_lists(scene, c.rays, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rays = src * 1.0
        res = scene.all_hits(rays, 4, stream=side)
        total = res.count.to(torch.int64).sum()
        inside = scene.contains(rays[:, 0:3].contiguous(), stream=side)
    side.synchronize()
    assert int(total) == int(c.want(4)[1].astype(np.int64).sum())
    got = (res.records.cpu().numpy().view(ar.RECORD).reshape(-1, 4), res.count.cpu().numpy())
    assert_same(got, null)
    assert_same(got, c.want(4))
    assert inside.cpu().numpy()[:256].tobytes() == reference_parity(c.v, c.idx, c.rays[:256, 0:3], gpu.CONTAINS_DIRECTION).tobytes()


@pytest.mark.gpu
def test_counted(gpu):
    """the counting form: the same lists, and three counters that are not zero -- nodes visited, own-box tests, triangle tests"""
    c = case("dragon")
    scene = gpu.Scene(dragon())
    work = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert_same(device_lists(scene, c.rays, 4, counts=work), c.want(4))
    nodes, boxes, tris = (int(x) for x in work.cpu())
    n, hits = len(c.rays), int(c.want(4)[1].sum())
    assert nodes >= n and hits <= tris <= boxes < n * len(c.idx) // 4
    cnt = scene.count_hits(torch.from_numpy(np.array(c.rays)).cuda(), counts=work)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tobytes() == c.want(4)[1].tobytes() and tuple(int(x) for x in work.cpu()) == (2 * nodes, 2 * boxes, 2 * tris)


@pytest.mark.gpu
def test_refusals(gpu):
    """misaligned pointers, host memory, max_hits outside [0, 32] and an array that runs past its allocation give GNXR_ERR_INVALID with
    the front end's messages before anything is queued; wrong tensors raise; the scene still answers afterwards"""
    c = case("dragon")
    scene = gpu.Scene(dragon())
    L = gpu.lib()
    rays = torch.from_numpy(np.array(c.rays)).cuda()
    out = torch.zeros((len(rays), 4, 4), device="cuda")
    cnt = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.gnxr_last_error().decode()
    call = L.gnxr_trace_all_device
    assert call(scene._h, P(rays, 4), 100, 4, P(out), P(cnt), None) == ERR_INVALID and "d_rays is not 16-byte aligned" in err()
    assert call(scene._h, P(rays), 100, 4, P(out, 8), P(cnt), None) == ERR_INVALID and "d_hits is not 16-byte aligned" in err()
    assert call(scene._h, P(rays), 100, 4, P(out), P(cnt, 2), None) == ERR_INVALID and "d_counts is not 4-byte aligned" in err()
    assert call(scene._h, P(rays), 100, 33, P(out), P(cnt), None) == ERR_INVALID and "max_hits" in err()
    assert call(scene._h, P(rays), 100, -1, P(out), P(cnt), None) == ERR_INVALID and "max_hits" in err()
    assert call(scene._h, P(rays), 100, 0, P(out), P(cnt), None) == ERR_INVALID and "count-only" in err()
    host = np.zeros((100, 16), F)
    assert call(scene._h, C.c_void_p(host.ctypes.data), 100, 4, P(out), P(cnt), None) == ERR_INVALID and "d_rays is not device memory" in err()
    assert call(scene._h, P(rays), 100, 4, C.c_void_p(host.ctypes.data), P(cnt), None) == ERR_INVALID and "d_hits is not device memory" in err()
    lone = torch.zeros((64, 8), device="cuda")
    assert call(scene._h, P(lone), 1 << 20, 4, P(out), P(cnt), None) == ERR_INVALID and "d_rays" in err()
    # a hits array too small for n * max_hits records.  (The front end compares with the runtime's allocation, which for a tensor is the
    # block of torch's caching allocator it lives in: the shortfall has to exceed that block, as `lone` does above -- 512 MB asked of 4 KB.)
    many = torch.zeros((1 << 20, 8), device="cuda")
    many_cnt = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")
    lone_hits = torch.zeros((64, 4), device="cuda")
    assert call(scene._h, P(many), 1 << 20, 32, P(lone_hits), P(many_cnt), None) == ERR_INVALID and "d_hits" in err()
    assert call(scene._h, P(many), 1 << 20, 0, None, P(lone_hits), None) == ERR_INVALID and "d_counts" in err()
    work = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert L.gnxr_trace_all_counted_device(scene._h, P(rays), 100, 4, P(out), P(cnt), P(work, 4), None) == ERR_INVALID and "d_work" in err()
    torch.cuda.synchronize()
    assert (out == 0).all() and (cnt == 0).all() and (work == 0).all()   # nothing was queued by the refused calls
    for bad in (rays.double(), rays.cpu(), rays[:, :4].contiguous(), rays.t(), np.array(c.rays)):
        with pytest.raises(ValueError):
            scene.all_hits(bad, 4)
    for k in (33, -1):
        with pytest.raises(ValueError):
            scene.all_hits(rays, k)
    with pytest.raises(ValueError):
        scene.all_hits(rays, 4, out=torch.zeros((len(rays), 4, 3), device="cuda"))
    with pytest.raises(ValueError):
        scene.all_hits(rays, 4, out=out.double())
    with pytest.raises(ValueError):
        scene.all_hits(rays, 4, counts=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        scene.contains(rays[:, 0:3])   # a non-contiguous view
    with pytest.raises(ValueError):
        scene.contains(rays[:, 0:3].contiguous(), direction=(0, 0, 0))
    assert_same(device_lists(scene, c.rays, 4), c.want(4))
