"""The cost-driven 4-wide collapse on the device: the walk over cuts of two, three and four children (balanced and chain) gives the
reference's answers, and the device rebuild produces the host collapse's tree.

(a) ray queries on seeded soups against the oracle, bit for bit -- among them arrangements around a pair of coplanar, overlapping
    triangles that a ray hits at exactly the same t: which of the two is reported depends on the order the slots of one cut are visited in;
(b) every soup moved, rebuilt on the device and compared with a fresh scene's tables;
(c) one small PathIntegrator render of the 2 000-triangle dragon scene against the oracle.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded)

import oracle_lib as ol
import scenes
import test_ray_queries_device as trq
import test_scene_rebuild as tsr
import test_scene_update as tsu

SIZES = (1, 2, 3, 4, 5, 7, 8, 13, 64, 2049)


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.5, 1.5, (n, 1, 3))
    s = 0.05 + 0.6 * rng.uniform(0, 1, (n, 1, 1)) ** 2
    v = (c + s * rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def growing(n=12):
    """triangle i sits at 1.6^i * 0.01 on the x axis and is that large: the SAH splits peel the small ones off one end (chain cuts)"""
    v = []
    for i in range(n):
        x = 0.01 * 1.6 ** i
        v += [(x - 2, 0, 0), (x * 1.5 - 2, x * 0.5, 0), (x - 2, 0, x * 0.5)]
    return np.array(v, np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


# Two triangles in the plane z = 0 that overlap on the small one.  For a ray from z = +-1 with direction z = -+1 (the largest component)
# the watertight test's scaled distance is the sum of the three edge functions times 1, summed as the determinant is, so t = det * (1 / det):
# exactly 1 for most determinants, for both triangles at once for most rays -- and then the one visited first is the hit.  Their
# centroids differ: they are leaves of their own, and with at most four triangles in the scene the tree is ONE DNode4 -- the pair sits
# in two slots of one cut.
PAIR = [(-0.2, -0.2, 0), (0.5, -0.2, 0), (-0.2, 0.5, 0), (-1.0, -1.0, 0), (1.5, -1.0, 0), (-1.0, 1.5, 0)]
OTHERS = {"pair": [],
          "pair+1": [(1.8, 1.8, 0.5), (2.0, 1.8, 0.5), (1.8, 2.0, 0.6)],
          "pair+2": [(1.8, 1.8, 0.5), (2.0, 1.8, 0.5), (1.8, 2.0, 0.6), (-2.2, 0, -1.0), (-2.0, 0.3, -1.0), (-2.2, 0.3, -1.4)],
          "pair+2near": [(0.0, 0.0, 0.3), (0.1, 0.0, 0.3), (0.0, 0.1, 0.3), (0.02, 0.02, -0.2), (0.07, 0.02, -0.2), (0.02, 0.07, -0.2)]}


def pair_case(name):
    v = np.array(PAIR + OTHERS[name], np.float32)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


CASES = {**{f"soup{n}": (lambda n=n: soup(n, 1000 + n)) for n in SIZES}, "growing12": growing, **{k: (lambda k=k: pair_case(k)) for k in OTHERS}}


def builder(gx, v, idx):
    return tsr.soup_builder(gx, v, idx, "sah")


def case_rays(gx, name):
    """~20 000 seeded random rays, rays with exactly zero direction components in all 8 octants' faces, and (pair cases) exact ties"""
    rng = np.random.default_rng(7)
    n = 4000
    o = rng.uniform(-2.4, 2.4, (n, 3)).astype(np.float32)
    zd = np.array([[sx * a, sy * b, sz * c] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1) for a, b, c in ((0.6, 0.8, 0), (0, 0.6, 0.8), (0.8, 0, 0.6), (1, 0, 0), (0, 1, 0), (0, 0, 1))],
                  np.float32)
    sets = [scenes.random_rays(20000, seed=5), scenes.random_rays(2000, seed=6, tmax=1.7), gx.make_rays(o, zd[rng.integers(0, len(zd), n)])]
    if name.startswith("pair"):
        m = 512   # all 8 octants: sign of z by the side the ray starts on, signs of x and y by the slant
        uv = rng.uniform(0, 1, (m, 2))
        uv = np.where(uv.sum(axis=1, keepdims=True) > 1, 1 - uv, uv)
        xy = (-0.15 + 0.5 * uv).astype(np.float32)                    # points of the overlap: x, y > -0.2, x + y < 0.3
        slant = (rng.uniform(0.05, 0.9, (m, 2)) * rng.choice([-1.0, 1.0], (m, 2))).astype(np.float32)
        side = rng.choice([-1.0, 1.0], m).astype(np.float32)
        d = np.concatenate([slant, -side[:, None]], axis=1).astype(np.float32)
        o2 = np.concatenate([xy - slant, side[:, None]], axis=1).astype(np.float32)
        sets.append(gx.make_rays(o2, d))
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_queries_equal_oracle(gpu, name):
    v, idx = CASES[name]()
    b = builder(gpu, v, idx)
    scene, osc = gpu.Scene(b), ol.OracleScene(b)
    if name.startswith("pair"):
        nodes4, root4, _ = scene.bvh4()
        kids = nodes4.view(np.int32)[:, 24:28]
        assert root4 == 0 and len(nodes4) == 1 and (kids != 0x7ffffffe).sum() == len(idx)
    sets = case_rays(gpu, name)
    for rays in sets:
        h, o = trq.dquery(scene, rays)
        trq.check_oracle(h, o, osc, rays)
    if name.startswith("pair") and name != "pair+2near":
        h, _ = trq.dquery(scene, sets[-1])
        assert set(np.unique(h["prim"])) <= {0, 1} and (np.abs(h["t"] - 1.0) <= 2.0 ** -22).all() and (h["t"] == 1.0).any()   # the overlap, ties among them


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in CASES if not k.startswith("pair")])
def test_rebuilt_soup_equals_fresh_scene(gpu, name):
    v, idx = CASES[name]()
    v0 = tsu.deform(v, len(v), seed=31, amount=0.05)
    s, fresh = tsr.rebuilt_and_fresh(gpu, builder(gpu, v0, idx), v)
    tsr.same_scene_tables(s, fresh)


@pytest.mark.gpu
def test_dragon_render_equals_oracle(gpu):
    b = scenes.dragon_cornell(2000, "glass+metal", mesh_path=tsu.MESH2K)
    integ = gpu.PathIntegrator(8, 1.0, "spatial")
    img, st = integ.Render(gpu.Scene(b), 96, 96, 6)
    oimg, ost = ol.OracleScene(b).render(integ, 96, 96, 6)
    assert (st["rays_closest"], st["rays_any"]) == (ost["rays_closest"], ost["rays_any"])
    assert trq.biteq(img[..., :3], oimg[..., :3])
