"""All-hits ray queries (include/gnxr.h, "All-hits ray queries") restated in numpy float32: every triangle against every ray, no tree.
Each `*`, `+`, `-`, `/` below is one rounded fp32 operation on arrays of float32, in the association of csrc/device_geom.h (slab_test,
ray_shear, tri_test_sheared -- the reference's Bounds3::IntersectP and the ray-space part of Triangle::Intersect), the fp64 fallback of
the edge functions included, so the records equal the device's byte for byte whatever tree the scene has."""
import numpy as np

F = np.float32
RECORD = np.dtype([("t", np.float32), ("prim", np.int32), ("b1", np.float32), ("b2", np.float32)])
assert RECORD.itemsize == 16
EMPTY = np.array([(np.inf, -1, 0, 0)], RECORD)[0]
EPS = F(2.0 ** -24)


def gamma(n):
    """gamma(n) = (n * MachineEpsilon) / (1 - n * MachineEpsilon) in fp32"""
    return (F(n) * EPS) / (F(1) - F(n) * EPS)


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


def triangle_bounds(p0, p1, p2):
    """lo = min(min(p0, p1), p2), hi = max(max(p0, p1), p2) per axis, by selection"""
    return _min(_min(p0, p1), p2), _max(_max(p0, p1), p2)


def slab_test(lo, hi, o, d, tmax):
    """Bounds3::IntersectP(ray, invDir, dirIsNeg) on [lo, hi] in the reference's comparison sequence.  lo, hi, o, d: (..., 3); tmax (...)."""
    with np.errstate(all="ignore"):
        inv = F(1) / d
        neg = inv < 0
        near, far = np.where(neg, hi, lo), np.where(neg, lo, hi)
        k = F(1) + F(2) * gamma(3)
        tn = (near - o) * inv
        tf = ((far - o) * inv) * k
        t_min, t_max = tn[..., 0], tf[..., 0]
        ok = ~((t_min > tf[..., 1]) | (tn[..., 1] > t_max))
        t_min = np.where(tn[..., 1] > t_min, tn[..., 1], t_min)
        t_max = np.where(tf[..., 1] < t_max, tf[..., 1], t_max)
        ok &= ~((t_min > tf[..., 2]) | (tn[..., 2] > t_max))
        t_min = np.where(tn[..., 2] > t_min, tn[..., 2], t_min)
        t_max = np.where(tf[..., 2] < t_max, tf[..., 2], t_max)
        return ok & (t_min < tmax) & (t_max > 0)


def _permute(v, order):
    """(v[kx], v[ky], v[kz]) per ray: v (R, T, 3) or (R, 1, 3), order (R, 3)"""
    return np.take_along_axis(v, np.broadcast_to(order[:, None, :], v.shape[:2] + (3,)), axis=2)


def tri_test(p0, p1, p2, o, d, tmax):
    """The ray-space part of Triangle::Intersect.  p0, p1, p2: (1 or R, T, 3); o, d: (R, 1, 3); tmax: (R, 1).  Returns (hit, t, b1, b2),
    each (R, T); t, b1, b2 mean something where hit."""
    with np.errstate(all="ignore"):
        ad = np.abs(d[:, 0, :])
        kz = np.where(ad[:, 0] > ad[:, 1], np.where(ad[:, 0] > ad[:, 2], 0, 2), np.where(ad[:, 1] > ad[:, 2], 1, 2))
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        order = np.stack([kx, ky, kz], axis=1)
        dp = _permute(d, order)
        sx, sy, sz = -dp[..., 0] / dp[..., 2], -dp[..., 1] / dp[..., 2], F(1) / dp[..., 2]
        q = [_permute(np.broadcast_to(p - o, np.broadcast(p, o).shape), order) for p in (p0, p1, p2)]
        x = [v[..., 0] + sx * v[..., 2] for v in q]
        y = [v[..., 1] + sy * v[..., 2] for v in q]
        z = [v[..., 2] for v in q]
        e0 = x[1] * y[2] - y[1] * x[2]
        e1 = x[2] * y[0] - y[2] * x[0]
        e2 = x[0] * y[1] - y[0] * x[1]
        again = (e0 == 0) | (e1 == 0) | (e2 == 0)
        if again.any():
            X, Y = [v.astype(np.float64) for v in x], [v.astype(np.float64) for v in y]
            e0 = np.where(again, (Y[2] * X[1] - X[2] * Y[1]).astype(F), e0)
            e1 = np.where(again, (Y[0] * X[2] - X[0] * Y[2]).astype(F), e1)
            e2 = np.where(again, (Y[1] * X[0] - X[1] * Y[0]).astype(F), e2)
        hit = ~(((e0 < 0) | (e1 < 0) | (e2 < 0)) & ((e0 > 0) | (e1 > 0) | (e2 > 0)))
        det = (e0 + e1) + e2
        hit &= ~(det == 0)
        z = [v * sz for v in z]
        t_scaled = (e0 * z[0] + e1 * z[1]) + e2 * z[2]
        bound = tmax * det
        hit &= ~((det < 0) & ((t_scaled >= 0) | (t_scaled < bound)))
        hit &= ~((det > 0) & ((t_scaled <= 0) | (t_scaled > bound)))
        inv_det = F(1) / det
        b1, b2 = e1 * inv_det, e2 * inv_det
        t = t_scaled * inv_det
        mx = lambda a, b, c: np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(c))
        max_zt, max_xt, max_yt, max_e = mx(*z), mx(*x), mx(*y), mx(e0, e1, e2)
        delta_z = gamma(3) * max_zt
        delta_x = gamma(5) * (max_xt + max_zt)
        delta_y = gamma(5) * (max_yt + max_zt)
        delta_e = F(2) * (((gamma(2) * max_xt) * max_yt + delta_y * max_xt) + delta_x * max_yt)
        delta_t = (F(3) * (((gamma(3) * max_e) * max_zt + delta_e * max_zt) + delta_z * max_e)) * np.abs(inv_det)
        hit &= ~(t <= delta_t)
        return hit, t.astype(F), b1.astype(F), b2.astype(F)


def valid_rays(rays):
    """finite o and d, tmax not a NaN, d not (0, 0, 0)"""
    o, d, tmax = rays[:, 0:3], rays[:, 4:7], rays[:, 3]
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & ~np.isnan(tmax) & (d != 0).any(axis=1)


def pair_tables(vertices, indices, rays, chunk_pairs=1 << 20):
    """Per (ray, triangle): own_box (the own-box test accepts), tri (the triangle test accepts), t, b1, b2 -- each (n, T); invalid rays
    accept nothing.  A HIT is own_box & tri."""
    vertices, rays = np.asarray(vertices, F), np.asarray(rays, F).reshape(-1, 8)
    indices = np.asarray(indices).reshape(-1, 3)
    n, T = len(rays), len(indices)
    own_box, tri = np.zeros((n, T), bool), np.zeros((n, T), bool)
    t, b1, b2 = np.zeros((n, T), F), np.zeros((n, T), F), np.zeros((n, T), F)
    if T == 0 or n == 0:
        return own_box, tri, t, b1, b2
    p0, p1, p2 = (vertices[indices[:, k]][None] for k in range(3))
    lo, hi = triangle_bounds(p0, p1, p2)
    ok = valid_rays(rays)
    step = max(1, chunk_pairs // T)
    for s in range(0, n, step):
        r = rays[s:s + step]
        o, d, tmax = r[:, None, 0:3], r[:, None, 4:7], r[:, None, 3]
        own_box[s:s + step] = slab_test(lo, hi, o, d, tmax) & ok[s:s + step, None]
        h, t[s:s + step], b1[s:s + step], b2[s:s + step] = tri_test(p0, p1, p2, o, d, tmax)
        tri[s:s + step] = h & ok[s:s + step, None]
    return own_box, tri, t, b1, b2


def all_hits(vertices, indices, rays, max_hits, tables=None):
    """(records, counts): the (n, max_hits) gnxr_ray_hit records (RECORD) and the int32 (n,) counts of `rays` (n, 8) = o, tmax, d, pad
    against the triangles `indices` (authoring order) of `vertices`.  `tables`: pair_tables of the same arguments, to share them."""
    own_box, tri, t, b1, b2 = tables if tables is not None else pair_tables(vertices, indices, rays)
    hit = own_box & tri
    n, T = hit.shape
    counts = hit.sum(axis=1).astype(np.int32)
    out = np.full((n, max_hits), EMPTY, RECORD)
    if max_hits == 0 or T == 0:
        return out, counts
    for i in np.flatnonzero(counts):
        prim = np.flatnonzero(hit[i])
        order = np.lexsort((prim, t[i, prim]))[:max_hits]   # ascending t, then ascending authoring index
        p = prim[order]
        o = out[i, :len(p)]
        o["t"], o["prim"], o["b1"], o["b2"] = t[i, p], p, b1[i, p], b2[i, p]
    return out, counts
