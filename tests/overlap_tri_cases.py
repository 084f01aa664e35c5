"""Query triangles and hand-made cases that tests/test_overlap_triangles.py and tests/dev_overlap_tri_time.py share.  A plain module:
nothing here is collected."""
import numpy as np

import overlap_tri_reference as otr
from overlap_cases import down, up
from query_cases import bound_of, dragon, mesh_of, surface_samples, uniform_in

F = np.float32

# Pairs of triangles of small integer coordinates: (name, query, scene triangle, overlaps).  Every product below is exact in fp32, or
# rounds in the direction the comment says, so the expectation is geometry's.
RIGHT = ((0, 0, 0), (4, 0, 0), (0, 4, 0))      # in z = 0, hypotenuse x + y = 4
TILTED = ((3, 0, 0), (0, 3, 0), (0, 0, 3))     # in x + y + z = 3, nt = (9, 9, 9); (1, 1, 1) is its centroid
E2 = F(2.0) ** F(-22)                          # one ulp at 2
HAND_MADE = [
    # a vertex on a face
    ("vertex on a face", ((1, 1, 0), (1, 1, 3), (2, 1, 3)), RIGHT, 1),
    # ... lifted by the smallest float: qlo.z > thi.z = 0, decided by step 2's comparisons alone
    ("vertex on a face, one ulp short (the bounds test)", ((1, 1, up(0)), (1, 1, 3), (2, 1, 3)), RIGHT, 0),
    # the same contact where the arithmetic carries the ulp: qa on the centroid of TILTED, the rest of the query beyond its plane.
    # With eps = 2^-23 and qa = (1 + eps, 1 + eps, 1): t = (2 - eps, -1 - eps, -1) and its rotations, all exact; e0 = (-3, 3, 0),
    # e1 = (0, -3, 3), nt = (9, 9, 9); dot(nt, ta) = ((18 - 16 eps) + (-9 - 8 eps)) - 9 = -24 eps, likewise tb, and tc gives -16 eps:
    # tmax = -16 eps < 0 = qmin (the query's other two vertices project to about 27 and 27), so nt separates.
    ("vertex on a tilted face", ((1, 1, 1), (3, 2, 2), (2, 3, 2)), TILTED, 1),
    ("vertex on a tilted face, one ulp short", ((up(1), up(1), 1), (3, 2, 2), (2, 3, 2)), TILTED, 0),
    ("vertex on a tilted face, one ulp past", ((down(1), down(1), 1), (3, 2, 2), (2, 3, 2)), TILTED, 1),
    # an edge through a face: the query's edge (1, 1, -1) - (1, 1, 1) crosses z = 0 inside RIGHT.  (Not a contact: there is no
    # one-ulp version of it.)
    ("edge piercing a face", ((1, 1, -1), (1, 1, 1), (5, 5, 1)), RIGHT, 1),
    # coplanar, the query's vertex (2, 2, 0) on the hypotenuse: decided by cross(nt, e1) = (-64, -64, 0)
    ("coplanar, sharing one edge point", ((2, 2, 0), (5, 2, 0), (2, 5, 0)), RIGHT, 1),
    # ... moved off by one ulp of 2 (E2): t = (-2 - E2, -2 - E2, 0), (2 - E2, -2 - E2, 0), (-2 - E2, 2 - E2, 0), exact; on
    # L = (-64, -64, 0) they project to 256 + 128 E2, 128 E2, 128 E2 (powers of two scale exactly): tmin = 2^-15 > 0 = qmax
    ("coplanar, one ulp off the edge", ((2 + E2, 2 + E2, 0), (5, 2 + E2, 0), (2 + E2, 5, 0)), RIGHT, 0),
    ("coplanar, one ulp over the edge", ((2 - E2 / 2, 2 - E2 / 2, 0), (5, 2, 0), (2, 5, 0)), RIGHT, 1),
    ("coplanar, one inside the other", ((1, 1, 0), (2, 1, 0), (1, 2, 0)), RIGHT, 1),
    ("coplanar, the other inside the one", ((-1, -1, 0), (9, -1, 0), (-1, 9, 0)), RIGHT, 1),
    # coplanar and disjoint inside each other's bounds: x + y >= 6 against x + y <= 4
    ("coplanar and disjoint", ((3, 3, 0), (4, 3, 0), (3, 4, 0)), RIGHT, 0),
    ("parallel planes one unit apart (the bounds test)", ((1, 1, 1), (2, 1, 1), (1, 2, 1)), RIGHT, 0),
    ("parallel tilted planes, the bounds overlapping", ((4, 0, 0), (0, 4, 0), (0, 0, 4)), TILTED, 0),
    ("a point query on a vertex", ((4, 0, 0),) * 3, RIGHT, 1),
    ("a point query on a face", ((1, 1, 1),) * 3, TILTED, 1),
    ("a point query beside the plane, inside the bounds", ((1, 1, 2),) * 3, TILTED, 0),
    ("a segment query through a face", ((0, 0, 0), (2, 2, 2), (2, 2, 2)), TILTED, 1),
    ("a segment query short of the face", ((0, 0, 0), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), TILTED, 0),
    ("a NaN coordinate", ((1, 1, 0), (1, np.nan, 3), (2, 1, 3)), RIGHT, 0),
    ("an infinite coordinate", ((1, 1, 0), (1, 1, np.inf), (2, 1, 3)), RIGHT, 0),
    ("a negative infinite coordinate", ((-np.inf, 1, 0), (1, 1, 3), (2, 1, 3)), RIGHT, 0),
]
# Pairs that exactly one of the five axis groups separates (otr.GROUPS), inside each other's bounds: dropping the group reports them.
# Found by a search over integer coordinates in [-4, 4]; (group, query, scene triangle).
LONE_SEPARATOR = [
    ("nq", ((0, 0, -1), (2, -3, -1), (2, 4, -4)), ((3, 2, -2), (4, -4, 3), (2, 1, -2))),
    ("nt", ((-4, -1, 0), (1, 1, 0), (-3, 1, 0)), ((3, 2, 2), (1, -1, -2), (0, 1, -1))),
    ("edge x edge", ((-2, 2, -1), (3, 4, -2), (0, -3, 2)), ((1, 3, 3), (4, 4, 4), (-3, -4, 0))),
    # an in-plane axis of the query is alone only against a triangle without a normal of its own: a zero-area one
    ("cross(nq, f)", ((-2, 2, 2), (1, -2, -3), (-3, 3, 4)), ((-1, -1, 2), (2, -4, -4), (2, -4, -4))),
    ("cross(nt, e)", ((-1, -1, 2), (2, -4, -4), (2, -4, -4)), ((-2, 2, 2), (1, -2, -3), (-3, 3, 4))),
]
ALL_PAIRS = HAND_MADE + [(f"{g} alone", q, t, 0) for g, q, t in LONE_SEPARATOR]
ONE = np.array([(0, 1, 2)], np.int32)


def pairs_by_triangle():
    """{scene triangle: (queries (m, 12), expected counts (m,), names)}: the pairs grouped into one-triangle scenes"""
    out = {}
    for name, q, t, want in ALL_PAIRS:
        out.setdefault(t, []).append((name, q, want))
    return {t: (otr.tri_records(np.array([c[1] for c in cs], F)), np.array([c[2] for c in cs], np.int32), [c[0] for c in cs]) for t, cs in out.items()}


def mixed_triangles(v, idx, n, rng):
    """n query triangles of mixed size around the mesh (v, idx): half centred on its surface, half uniformly in its grown bounds; the
    extent is 2^U(-7, 1) of the scene's diagonal, the corners uniform in a cube of that edge round the centre; a few segments (two
    corners equal) and points (all three)."""
    lo, hi = bound_of(v)
    diag = float(np.linalg.norm(hi - lo))
    ctr = np.concatenate([surface_samples(v, idx, n // 2, rng, 0.0), uniform_in(lo, hi, n - n // 2, rng, 1.1)])
    ctr = ctr[rng.permutation(n)]
    extent = diag * 2.0 ** rng.uniform(-7, 1, (n, 1, 1))
    corners = (ctr[:, None, :] + extent * rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(F)
    corners[0:12, 2] = corners[0:12, 1]          # segments
    corners[12:20, 1] = corners[12:20, 0]        # points
    corners[12:20, 2] = corners[12:20, 0]
    corners[20:24] = ctr[20:24, None, :]         # points on the surface (or in the air)
    return otr.tri_records(corners)


def sine_deformed(v, idx, amplitude=0.25, frequency=8.0):
    """the mesh's own vertices (all but the Cornell box's and the light's last twelve triangles) under a sine displacement strong enough
    to fold the 2 k mesh through itself (by the restatement 1762 directed pairs, 37 % of the triangles involved; 0.15 / 8 folds 1.5 %,
    0.3 / 8 56 %); returns (the scene's new vertex array, the number of leading vertices that moved)"""
    n_mesh_v = int(idx[:len(idx) - 12].max()) + 1
    v2 = v.copy()
    v2[:n_mesh_v] += (F(amplitude) * np.sin(F(frequency) * v[:n_mesh_v, [1, 2, 0]])).astype(F)
    return v2, n_mesh_v


_cache = {}


def tri_case():
    """the 2 k mesh in its Cornell box, 1024 mixed query triangles and the restatement's matrix over them: computed once, shared, never
    written"""
    if "tri" not in _cache:
        v, idx = mesh_of(dragon())
        queries = mixed_triangles(v, idx, 1024, np.random.default_rng(78))
        m = otr.overlap_matrix(v, idx, queries)
        for x in (v, idx, queries, m):
            x.setflags(write=False)
        _cache["tri"] = dict(v=v, idx=idx, queries=queries, m=m, count=m.sum(axis=1).astype(np.int32))
    return _cache["tri"]


def check_mix(count):
    """the conditions on the query set: enough misses, enough long lists, enough short ones"""
    assert (count == 0).mean() > 0.2 and (count > 32).mean() > 0.03 and ((count > 0) & (count < 8)).mean() > 0.1, \
        ((count == 0).mean(), (count > 32).mean(), ((count > 0) & (count < 8)).mean())


def self_case():
    """the 2 k scene at rest and under the sine deformation, with the restatement's self matrices: computed once, shared, never written"""
    if "self" not in _cache:
        c = tri_case()
        v2, n_mesh_v = sine_deformed(c["v"], c["idx"])
        rest, bent = otr.self_matrix(c["v"], c["idx"]), otr.self_matrix(v2, c["idx"])
        for x in (v2, rest, bent):
            x.setflags(write=False)
        _cache["self"] = dict(v2=v2, n_mesh_v=n_mesh_v, rest=rest, bent=bent)
    return _cache["self"]
