"""Sphere casts (include/gnxr.h, "Sphere casts") restated in numpy float32: every triangle against every cast, no tree.  Each `*`, `+`,
`-`, `/` and sqrt below is one rounded fp32 operation on arrays of float32, in the association the header states, and the point-triangle
arithmetic is closest_reference.closest_on_triangle, so the records equal the device's bit for bit whatever tree the scene has."""
import numpy as np

import closest_reference as cr

F = np.float32
RECORD = cr.RECORD   # the dist2 slot holds t
INF = F(np.inf)
_dot, _min, _max = cr._dot, cr._min, cr._max


def empty_records(n):
    """no hit: prim -1, t +inf, every other field 0"""
    out = np.zeros(n, RECORD)
    out["prim"] = -1
    out["dist2"] = np.inf
    return out


def casts_of(origins, directions, radius, tmax=np.inf):
    c = np.zeros((len(origins), 8), F)
    c[:, 0:3], c[:, 3], c[:, 4:7], c[:, 7] = origins, radius, directions, tmax
    return c


def valid_casts(casts):
    """step 0: no NaN anywhere, r >= 0, tmax >= 0, o and d finite"""
    o, r, d, tmax = casts[:, 0:3], casts[:, 3], casts[:, 4:7], casts[:, 7]
    with np.errstate(all="ignore"):
        return (r >= 0) & (tmax >= 0) & np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)


def grown_box(lo, hi, o, r, inv, bound):
    """step 1 on boxes [lo, hi] (..., 3) for casts that broadcast against them: (passes, tb).  `bound`: the cast's tmax."""
    glo, ghi = lo - r[..., None], hi + r[..., None]
    moving = np.isfinite(inv)
    neg = inv < 0
    entry = (np.where(neg, ghi, glo) - o) * np.where(moving, inv, F(1))
    leave = (np.where(neg, glo, ghi) - o) * np.where(moving, inv, F(1))
    shape = np.broadcast(entry, moving).shape
    entry, leave, moving = np.broadcast_to(entry, shape), np.broadcast_to(leave, shape), np.broadcast_to(moving, shape)
    static_ok = (moving | ((glo <= o) & (o <= ghi))).all(axis=-1)
    tb = np.zeros(shape[:-1], F)
    tx = np.full(shape[:-1], INF)
    for k in range(3):
        tb = np.where(moving[..., k], _max(tb, entry[..., k]), tb)
        tx = np.where(moving[..., k], _min(tx, leave[..., k]), tx)
    return static_ok & (tb <= tx) & (tb <= bound), tb


def _take(ta, t, ok):
    """a candidate counts iff 0 <= t < +inf (a NaN fails); ta keeps the smallest"""
    ok = ok & (t >= 0) & (t < INF)
    return np.where(ok, _min(ta, t), ta)


def analytic_time(a, b, c, o, d, r):
    """step 2: ta (+inf: none) of casts (o, d, r) against triangles (a, b, c); float32 arrays (..., 3) / (...) that broadcast"""
    r2 = r * r
    dd = _dot(d, d)
    start = cr.closest_on_triangle(a, b, c, o)[0] <= r2
    ta = np.full(start.shape, INF)
    # the face
    ab, ac = b - a, c - a
    n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                  ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], axis=-1)
    nn = _dot(n, n)
    length = np.sqrt(nn)
    sd, dn = _dot(n, o - a), _dot(n, d)
    h = r * length
    tf = (np.where(sd < 0, -h, h) - sd) / dn
    ok = (nn > 0) & (tf >= 0) & (tf < INF)
    centre = o + np.where(ok, tf, F(0))[..., None] * d
    ok = ok & (cr.closest_on_triangle(a, b, c, centre)[4] == 0)
    ta = _take(ta, tf, ok)
    # the edges
    for p0, p1 in ((a, b), (a, c), (b, c)):
        e, m = p1 - p0, o - p0
        me, de, ee, md, mm = _dot(m, e), _dot(d, e), _dot(e, e), _dot(m, d), _dot(m, m)
        A = ee * dd - de * de
        C = ee * (mm - r2) - me * me
        B = ee * md - de * me
        disc = B * B - A * C
        t = (-B - np.sqrt(disc)) / A
        w = me + t * de
        ta = _take(ta, t, (A > 0) & (disc >= 0) & (w >= 0) & (w <= ee))
    # the vertices
    for v in (a, b, c):
        m = o - v
        bq, cq = _dot(m, d), _dot(m, m) - r2
        disc = bq * bq - dd * cq
        t = (-bq - np.sqrt(disc)) / dd
        ta = _take(ta, t, (dd > 0) & (disc >= 0))
    return np.where(start, F(0), ta)


def hit_times(vertices, indices, casts):
    """(hits (n, T) bool, t (n, T) float32) of steps 0-3 for every cast against every triangle"""
    a, b, c = (vertices[indices[:, k]][None] for k in range(3))
    o, r, d, tmax = casts[:, None, 0:3], casts[:, None, 3], casts[:, None, 4:7], casts[:, None, 7]
    with np.errstate(all="ignore"):
        inv = F(1) / d
        lo, hi = cr.triangle_bounds(a, b, c)
        passes, tb = grown_box(lo, hi, o, r, inv, tmax)
        ta = analytic_time(a, b, c, o, d, r)
        t = np.where(ta > tb, ta, tb)
        hits = valid_casts(casts)[:, None] & passes & (ta < INF) & (t <= tmax)
    return hits, t


def sphere_casts(vertices, indices, casts, chunk=64):
    """The records (RECORD, t in the dist2 slot) of `casts` (n, 8) = o.xyz, radius, d.xyz, tmax against the triangles `indices` (authoring
    order) of `vertices`: the smallest (t, prim) over all triangles that hit, then closest_on_triangle at the centre of that time."""
    vertices, casts = np.asarray(vertices, F), np.ascontiguousarray(casts, F).reshape(-1, 8)
    indices = np.asarray(indices).reshape(-1, 3)
    out = empty_records(len(casts))
    for s in range(0, len(casts) if len(indices) else 0, chunk):
        rec = casts[s:s + chunk]
        hits, t = hit_times(vertices, indices, rec)
        key = np.where(hits, t, INF)
        least = key.min(axis=1)
        win = (hits & (key == least[:, None])).argmax(axis=1)   # the smallest authoring index among the bit-equal least
        has = hits.any(axis=1)
        tw = least
        with np.errstate(all="ignore"):
            centre = rec[:, 0:3] + np.where(has, tw, F(0))[:, None] * rec[:, 4:7]
            _, p, b1, b2, feature = cr.closest_on_triangle(*(vertices[indices[win, k]] for k in range(3)), centre)
        o = out[s:s + chunk]
        o["prim"] = np.where(has, win, -1)
        o["dist2"] = np.where(has, tw, INF)
        o["p"] = np.where(has[:, None], p, 0)
        o["b1"] = np.where(has, b1, 0)
        o["b2"] = np.where(has, b2, 0)
        o["feature"] = np.where(has, feature, 0)
    return out
