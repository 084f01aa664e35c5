"""Boxes and hand-made cases that tests/test_overlap_box.py and tests/dev_overlap_time.py share.  A plain module: nothing here is collected."""
import numpy as np

import overlap_reference as orf
from query_cases import bound_of, dragon, mesh_of, surface_samples, uniform_in

F = np.float32
INF = F(np.inf)


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


# Triangles of small integer coordinates and boxes against them: (name, triangle, lo, hi, overlaps).  Every value below survives the
# definition's fp32 steps exactly, or rounds in the direction the comment says, so the expectation is geometry's.
RIGHT = ((0, 0, 0), (4, 0, 0), (0, 4, 0))      # in z = 0, hypotenuse x + y = 4
HALF = ((0, 0, 0), (2, 0, 0), (0, 2, 0))       # hypotenuse x + y = 2 through (1, 1)
TILTED = ((2, 2, -1), (-2, 2, 3), (2, -2, 3))  # in x + y + z = 3, n = (16, 16, 16), (1, 1, 1) = a / 2 + b / 4 + c / 4 inside
WIDE = ((0, 0, 0), (8, 0, 0), (0, 8, 0))
SKEW = ((4, 0, 0), (0, 4, 0), (0, 0, 4))       # in x + y + z = 4, bounds [0, 4]^3
ODD = ((1, 2, 3), (4, 0, 0), (0, 4, -1))
HAND_MADE = [
    # a box-axis contact: the box's corner on vertex a, decided by step 2's comparisons alone
    ("box axis, touching", RIGHT, (-1, -1, -1), (0, 0, 1), 1),
    ("box axis, one ulp short", RIGHT, (-1, -1, -1), (down(0), 0, 1), 0),
    ("box axis, one ulp past", RIGHT, (-1, -1, -1), (up(0), up(0), 1), 1),
    # an edge-axis contact: the box's edge x = y = 1 on the hypotenuse's midpoint, from outside; no box axis and no plane separates.
    # ctr rounds to 2 in all three; h = 1, 1 - 2^-24 (exact), 1 (rounded from 1 + 2^-25): r = 4 h against min(p) = 4
    ("edge axis, touching", HALF, (1, 1, -1), (3, 3, 1), 1),
    ("edge axis, one ulp short", HALF, (up(1), up(1), -1), (3, 3, 1), 0),
    ("edge axis, one ulp past", HALF, (down(1), down(1), -1), (3, 3, 1), 1),
    # a plane contact: the box's corner (1, 1, 1) on the triangle's interior, the box on the far side.  ua = (0, 0, -3), so
    # vmin = (-h.x, -h.y, 2) is exact and dot(n, vmin) = 16 (2 - 2 h.x) = 0, 2^-19, 0
    ("plane, touching", TILTED, (1, 1, 1), (3, 3, 3), 1),
    ("plane, one ulp short", TILTED, (up(1), up(1), 1), (3, 3, 3), 0),
    ("plane, one ulp past", TILTED, (down(1), down(1), 1), (3, 3, 3), 1),
    ("a box in the triangle's interior, no vertex in it", WIDE, (1, 1, -1), (2, 2, 1), 1),
    ("a box inside the triangle's bounds, below its plane", SKEW, (0.25, 0.25, 0.25), (0.5, 0.5, 0.5), 0),
    ("a box inside the triangle's bounds, above its plane", SKEW, (3, 3, 3), (3.5, 3.5, 3.5), 0),
    ("a point box on vertex a", ODD, ODD[0], ODD[0], 1),
    ("a point box on vertex b", ODD, ODD[1], ODD[1], 1),
    ("a point box on vertex c", ODD, ODD[2], ODD[2], 1),
    ("an inverted box", RIGHT, (1, 1, 0), (0, 2, 0), 0),
    ("a NaN bound", RIGHT, (np.nan, 0, 0), (1, 1, 1), 0),
    ("a NaN upper bound", RIGHT, (0, 0, 0), (1, np.nan, 1), 0),
    ("an infinite lower bound", RIGHT, (-np.inf, -1, -1), (1, 1, 1), 0),
    ("an infinite upper bound", RIGHT, (-1, -1, -1), (np.inf, 1, 1), 0),
]
ONE = np.array([(0, 1, 2)], np.int32)


def hand_made_by_triangle():
    """{triangle: (boxes (m, 8), expected counts (m,), names)}: the cases grouped into one-triangle scenes"""
    out = {}
    for name, tri, lo, hi, want in HAND_MADE:
        out.setdefault(tri, []).append((name, lo, hi, want))
    return {tri: (orf.box_records(np.array([c[1] for c in cs], F), np.array([c[2] for c in cs], F)), np.array([c[3] for c in cs], np.int32), [c[0] for c in cs])
            for tri, cs in out.items()}


def mixed_boxes(v, idx, n, rng):
    """n boxes of mixed size around the mesh (v, idx): half centred uniformly in its bounds, half on surface-near points; half extents
    from a thousandth of the scene's extent -- below a triangle's edge -- to the whole of it, squeezed per axis by up to 8 so that thin
    slabs and rods occur, and a few degenerate ones (a point, a flat box)"""
    lo, hi = bound_of(v)
    extent = float((hi - lo).max())
    ctr = np.concatenate([uniform_in(lo, hi, n // 2, rng, 1.1), surface_samples(v, idx, n - n // 2, rng, 1e-3 * extent)])
    half = (extent * rng.choice([0.001, 0.004, 0.02, 0.08, 0.3, 1.0], (n, 1)) * rng.choice([1.0, 0.5, 0.125], (n, 3))).astype(F)
    half[0:8] = 0
    half[8:16, 1] = 0
    ctr = ctr[rng.permutation(n)]
    return orf.box_records((ctr - half).astype(F), (ctr + half).astype(F))


_dragon_cache = {}


def dragon_case():
    """the 2 k mesh in its Cornell box, 1024 mixed boxes and the restatement's matrix over them: computed once, shared, never written"""
    if not _dragon_cache:
        v, idx = mesh_of(dragon())
        boxes = mixed_boxes(v, idx, 1024, np.random.default_rng(77))
        m = orf.overlap_matrix(v, idx, boxes)
        for x in (v, idx, boxes, m):
            x.setflags(write=False)
        _dragon_cache.update(v=v, idx=idx, boxes=boxes, m=m, count=orf.counts_of(m))
    return _dragon_cache
