"""include/gnxr.h, "Triangle overlap queries", restated in numpy float32: a brute force over all triangles, one rounded fp32 operation per
step and in the header's order.  Rows, CSR lists and counts of the device are compared with what this module gives on bytes (the rows /
CSR / counts helpers are overlap_reference.py's).  A plain module: nothing here is collected."""
import numpy as np

F = np.float32
SKIP_SHARED, SELF = 1, 2
GROUPS = ("nq", "nt", "edge x edge", "cross(nq, f)", "cross(nt, e)")   # the five groups of step 5's seventeen axes


def _sel_min(x, y):
    return np.where(y < x, y, x)


def _sel_max(x, y):
    return np.where(y > x, y, x)


def _min3(x, y, z):
    return _sel_min(_sel_min(x, y), z)


def _max3(x, y, z):
    return _sel_max(_sel_max(x, y), z)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub(u, v):
    return [u[k] - v[k] for k in range(3)]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def tri_records(corners):
    """(n, 3, 3) or (n, 9) corners -> (n, 12) float32 gnxr_tri_query records, pads 0"""
    corners = np.asarray(corners, F).reshape(-1, 3, 3)
    q = np.zeros((len(corners), 12), F)
    for m in range(3):
        q[:, 4 * m:4 * m + 3] = corners[:, m]
    return q


def corners_of(queries):
    """(n, 12) records -> (n, 3, 3)"""
    return np.asarray(queries, F).reshape(-1, 3, 4)[:, :, 0:3]


def tri_valid(queries):
    """step 1: (n,) bool"""
    return np.isfinite(corners_of(queries)).all(axis=(1, 2))


def query_bounds(queries):
    """qlo, qhi (n, 3) by selection -- and so the gnxr_box_query records the walk of a query equals"""
    c = corners_of(queries)
    with np.errstate(invalid="ignore"):
        return _min3(c[:, 0], c[:, 1], c[:, 2]), _max3(c[:, 0], c[:, 1], c[:, 2])


def axes_separate(qa, qb, qc, a, b, c):
    """steps 4 and 5 for arrays of pairs; every argument a list of three (pairs,) float32 arrays.  Returns the seventeen `separates`
    arrays in the header's order: nq, nt, nine cross(f_i, e_j), three cross(nq, f_i), three cross(nt, e_j)."""
    ub, uc = _sub(qb, qa), _sub(qc, qa)
    f = [ub, _sub(uc, ub), uc]
    nq = _cross(ub, uc)
    ta, tb, tc = _sub(a, qa), _sub(b, qa), _sub(c, qa)
    e = [_sub(tb, ta), _sub(tc, tb), _sub(ta, tc)]
    nt = _cross(e[0], e[1])
    axes = [nq, nt] + [_cross(f[i], e[j]) for i in range(3) for j in range(3)] + [_cross(nq, f[i]) for i in range(3)] + [_cross(nt, e[j]) for j in range(3)]
    zero = np.zeros_like(ub[0])
    out = []
    for L in axes:
        d1, d2 = _dot(L, ub), _dot(L, uc)
        qmin, qmax = _min3(zero, d1, d2), _max3(zero, d1, d2)
        da, db, dc = _dot(L, ta), _dot(L, tb), _dot(L, tc)
        tmin, tmax = _min3(da, db, dc), _max3(da, db, dc)
        out.append((tmin > qmax) | (tmax < qmin))
    return out


def groups_separate(q, t):
    """one pair of (3, 3) triangles: which of the five axis GROUPS holds an axis that separates -- a tuple of five bools"""
    q, t = np.asarray(q, F).reshape(3, 3), np.asarray(t, F).reshape(3, 3)
    col = lambda p: [np.array([p[k]], F) for k in range(3)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = [bool(x[0]) for x in axes_separate(col(q[0]), col(q[1]), col(q[2]), col(t[0]), col(t[1]), col(t[2]))]
    return (s[0], s[1], any(s[2:11]), any(s[11:14]), any(s[14:17]))


def overlap_matrix(v, idx, queries, skip_shared=False):
    """(n queries, n triangles) bool: triangle t of (v, idx), in authoring order, overlaps query i -- steps 1 to 5.  Steps 1 to 3
    (comparisons) run over all pairs; steps 4 and 5 over the pairs that pass them, one array element per pair."""
    v, queries = np.asarray(v, F), np.asarray(queries, F).reshape(-1, 12)
    idx = np.asarray(idx).reshape(-1, 3)
    n = len(queries)
    corners = [v[idx[:, m]] for m in range(3)]
    qc = corners_of(queries)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ok = np.broadcast_to(tri_valid(queries)[:, None], (n, len(idx))).copy()
        qlo, qhi = query_bounds(queries)
        # 2. the bounds test on the triangle's own box: selections and comparisons
        for k in range(3):
            ak, bk, ck = (p[:, k] for p in corners)
            tlo, thi = _min3(ak, bk, ck), _max3(ak, bk, ck)
            ok &= (tlo[None, :] <= qhi[:, k][:, None]) & (thi[None, :] >= qlo[:, k][:, None])
        # 3. shared vertices
        if skip_shared:
            for m in range(3):
                for p in corners:
                    ok &= ~(qc[:, m][:, None, :] == p[None, :, :]).all(axis=2)
        qi, ti = np.nonzero(ok)
        q3 = [[qc[qi, m, k] for k in range(3)] for m in range(3)]
        a, b, c = ([p[ti, k] for k in range(3)] for p in corners)
        keep = np.ones(len(qi), bool)
        for sep in axes_separate(q3[0], q3[1], q3[2], a, b, c):
            keep &= ~sep
    ok[qi, ti] = keep
    return ok


def self_matrix(v, idx):
    """GNXR_OVERLAP_TRI_SELF: the scene's own triangles in authoring order as the queries, with the skip rule"""
    return overlap_matrix(v, idx, tri_records(np.asarray(v, F)[np.asarray(idx).reshape(-1, 3)]), skip_shared=True)


def pairs_of(m):
    """the unique (i, j), i < j, of a self matrix reported in either direction, sorted lexicographically: (m, 2) int32"""
    i, j = np.nonzero(np.triu(m | m.T, 1))
    return np.stack([i, j], axis=1).astype(np.int32)


# ---------------------------------------------------------------- an independent check in float64, geometry only
def sat_gap64(v, idx, queries, qi, ti):
    """float64, per pair (query qi[k], triangle ti[k]): the largest separation of the two triangles over the axes of the separating-axis
    theorem for two triangles (the two normals, the nine edge x edge products and, for coplanar pairs, each normal crossed with its own
    three edges), each normalised, so the figure is a length.  Positive: they are apart by at least that much along some axis;
    negative: on every axis they overlap by at least that much.  Degenerate axes are skipped.  Works on the vertices as they stand --
    no translation -- and knows nothing of the fp32 definition's order of operations."""
    v = np.asarray(v, np.float64)
    idx = np.asarray(idx).reshape(-1, 3)
    qc = corners_of(queries).astype(np.float64)[qi]          # (pairs, 3, 3)
    q = [qc[:, m] for m in range(3)]
    t = [v[idx[ti, m]] for m in range(3)]
    fq = [q[1] - q[0], q[2] - q[1], q[0] - q[2]]
    et = [t[1] - t[0], t[2] - t[1], t[0] - t[2]]
    nq, nt = np.cross(fq[0], fq[1]), np.cross(et[0], et[1])
    axes = [nq, nt] + [np.cross(f, e) for f in fq for e in et] + [np.cross(nq, f) for f in fq] + [np.cross(nt, e) for e in et]
    scale = np.maximum(np.abs(qc).max(axis=(1, 2)), 1e-300)
    gap = np.full(len(qi), -np.inf)
    for ax in axes:
        length = np.linalg.norm(ax, axis=1)
        good = length > 1e-12 * scale * scale   # a product of two edges: far below any axis two distinct directions give
        ax = ax / np.where(good, length, 1.0)[:, None]
        pq = np.stack([(p * ax).sum(axis=1) for p in q])
        pt = np.stack([(p * ax).sum(axis=1) for p in t])
        g = np.maximum(pt.min(axis=0) - pq.max(axis=0), pq.min(axis=0) - pt.max(axis=0))
        gap = np.where(good, np.maximum(gap, g), gap)
    return gap
