"""Neighbour queries (include/gnxr.h, "Neighbour queries") restated in numpy float32: every triangle against every query, no tree.  The
per-triangle arithmetic is closest_reference.closest_on_triangle, so records and counts equal the device's byte for byte whatever tree the
scene has, in both modes and for every K."""
import numpy as np

import closest_reference as cr

F = np.float32
RECORD = cr.RECORD
NEAR_MAX = 32


def empty_slots(shape):
    """slots nothing was found for: prim -1, dist2 +inf, every other field 0"""
    out = np.zeros(shape, RECORD)
    out["prim"] = -1
    out["dist2"] = np.inf
    return out


def near_lists(vertices, indices, queries, K, chunk=128):
    """(records (n, K) of RECORD, count_all (n,) int32, count_nearest (n,) int32) of `queries` (n, 4) = x, y, z, max_distance against the
    triangles `indices` (authoring order) of `vertices`: per query dist2 against every triangle; the mask dist2 <= r2 under the
    valid-query rule; a stable sort by (dist2, prim); the cut to K.  The records are those of both modes; count_all is GNXR_NEAR_ALL's
    count, count_nearest = min(count_all, K) is GNXR_NEAR_NEAREST's."""
    vertices, queries = np.asarray(vertices, F), np.asarray(queries, F).reshape(-1, 4)
    indices = np.asarray(indices).reshape(-1, 3)
    n, T = len(queries), len(indices)
    out = empty_slots((n, K))
    count = np.zeros(n, np.int32)
    if T:
        a, b, c = (vertices[indices[:, k]][None] for k in range(3))
    for s in range(0, n if T else 0, chunk):
        rec = queries[s:s + chunk]
        q, md = rec[:, None, 0:3], rec[:, 3]
        with np.errstate(all="ignore"):
            r2 = md * md
            ok = ~(np.isnan(rec[:, 0:3]).any(axis=1) | np.isnan(md) | (md < 0))
            dist2, p, b1, b2, feature = cr.closest_on_triangle(a, b, c, q)
            near = (dist2 <= r2[:, None]) & ok[:, None]   # a NaN dist2 fails
        count[s:s + chunk] = near.sum(axis=1)
        if K == 0:
            continue
        key = np.where(near, dist2, F(np.inf))
        rows = np.arange(len(rec))[:, None]
        by_dist = np.argsort(key, axis=1, kind="stable")   # stable: bit-equal dist2 stay in authoring order
        # the near ones first, in that order (a near triangle at dist2 = +inf must not stand behind one that is not near)
        first = np.take_along_axis(by_dist, np.argsort(~near[rows, by_dist], axis=1, kind="stable"), axis=1)[:, :K]
        k = first.shape[1]
        held = np.arange(k)[None, :] < np.minimum(count[s:s + chunk], K)[:, None]
        o = out[s:s + chunk, :k]
        o["prim"] = np.where(held, first, -1)
        o["dist2"] = np.where(held, dist2[rows, first], F(np.inf))
        o["p"] = np.where(held[..., None], p[rows, first], 0)
        o["b1"] = np.where(held, b1[rows, first], 0)
        o["b2"] = np.where(held, b2[rows, first], 0)
        o["feature"] = np.where(held, feature[rows, first], 0)
    return out, count, np.minimum(count, K).astype(np.int32)
