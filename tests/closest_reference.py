"""Closest-point queries (include/gnxr.h, "Closest-point queries") restated in numpy float32: every triangle against every query, no tree.
Each `*`, `+`, `-`, `/` below is one rounded fp32 operation on arrays of float32, in the association the header states, so the records
equal the device's bit for bit whatever tree the scene has."""
import numpy as np

F = np.float32
RECORD = np.dtype([("prim", np.int32), ("dist2", np.float32), ("p", np.float32, 3), ("b1", np.float32), ("b2", np.float32), ("feature", np.int32)])
assert RECORD.itemsize == 32


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


def triangle_bounds(a, b, c):
    """lo = min(min(a, b), c), hi = max(max(a, b), c) per axis"""
    return _min(_min(a, b), c), _max(_max(a, b), c)


def box_dist2(lo, hi, q):
    """bd2 of the walk: per axis e = max(max(lo - q, q - hi), 0), then (e.x e.x + e.y e.y) + e.z e.z"""
    e = _max(_max(lo - q, q - hi), F(0))
    return _dot(e, e)


def closest_on_triangle(a, b, c, q):
    """(dist2, p, b1, b2, feature) of query points q against triangles (a, b, c); the arrays are float32 (..., 3) and broadcast."""
    a, b, c, q = (np.asarray(x, F) for x in (a, b, c, q))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, q - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = q - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = q - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        v3 = d1 / (d1 - d3)
        w5 = d2 / (d2 - d6)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = F(1) / ((va + vb) + vc)
        v7, w7 = vb * denom, vc * denom
        shape = np.broadcast(d1, d3, d5).shape
        zero, one = np.zeros(shape, F), np.ones(shape, F)
        full = lambda x: np.broadcast_to(x, shape + (3,))
        points = [full(a), full(b), a + v3[..., None] * ab, full(c), a + w5[..., None] * ac, b + w6[..., None] * (c - b)]
        face = (a + v7[..., None] * ab) + w7[..., None] * ac
        p = np.select([m[..., None] for m in conds], points, face)
        b1 = np.select(conds, [zero, one, v3, zero, zero, one - w6], v7)
        b2 = np.select(conds, [zero, zero, zero, one, w5, w6], w7)
        feature = np.select(conds, [4, 5, 1, 6, 2, 3], 0).astype(np.int32)
        lo, hi = triangle_bounds(a, b, c)
        p = np.where(p < lo, lo, np.where(p > hi, hi, p))
        d = q - p
        return _dot(d, d), p, b1, b2, feature


def closest_points(vertices, indices, queries, chunk=128, ties=False):
    """The gnxr_closest_point records (RECORD) of `queries` (n, 4) = x, y, z, max_distance against the triangles `indices` (authoring
    order) of `vertices`.  ties=True: also the number of triangles that share the winning dist2, per query."""
    vertices, queries = np.asarray(vertices, F), np.asarray(queries, F).reshape(-1, 4)
    indices = np.asarray(indices).reshape(-1, 3)
    a, b, c = (vertices[indices[:, k]][None] for k in range(3))
    out = np.zeros(len(queries), RECORD)
    out["prim"] = -1
    tied = np.zeros(len(queries), np.int64)
    for s in range(0, len(queries), chunk):
        rec = queries[s:s + chunk]
        q, md = rec[:, None, 0:3], rec[:, 3]
        with np.errstate(all="ignore"):
            r2 = md * md
            ok = ~(np.isnan(rec[:, 0:3]).any(axis=1) | np.isnan(md) | (md < 0))
            if len(indices) == 0:
                continue
            dist2, p, b1, b2, feature = closest_on_triangle(a, b, c, q)
            counts = (dist2 <= r2[:, None]) & ok[:, None]   # a NaN dist2 fails
        key = np.where(counts, dist2, F(np.inf))
        least = key.min(axis=1)
        winners = counts & (key == least[:, None])
        win = winners.argmax(axis=1)   # the smallest authoring index among the bit-equal least
        has = counts.any(axis=1)
        rows = np.arange(len(rec))
        o = out[s:s + chunk]
        o["prim"] = np.where(has, win, -1)
        o["dist2"] = np.where(has, dist2[rows, win], 0)
        o["p"] = np.where(has[:, None], p[rows, win], 0)
        o["b1"] = np.where(has, b1[rows, win], 0)
        o["b2"] = np.where(has, b2[rows, win], 0)
        o["feature"] = np.where(has, feature[rows, win], 0)
        tied[s:s + chunk] = winners.sum(axis=1)
    return (out, tied) if ties else out
