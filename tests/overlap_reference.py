"""include/gnxr.h, "Overlap queries", restated in numpy float32: a brute force over all triangles, one rounded fp32 operation per step and
in the header's order.  Rows, CSR lists and counts of the device are compared with what this module gives on bytes.  A plain module:
nothing here is collected."""
import numpy as np

F = np.float32
OVERLAP_MAX = 32


def _sel_min(x, y):
    return np.where(y < x, y, x)


def _sel_max(x, y):
    return np.where(y > x, y, x)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def box_valid(boxes):
    """step 1: (n,) bool"""
    lo, hi = boxes[:, 0:3], boxes[:, 4:7]
    with np.errstate(invalid="ignore"):
        return (lo <= hi).all(axis=1) & np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1)


def overlap_matrix(v, idx, boxes):
    """(n boxes, n triangles) bool: triangle t of (v, idx), in authoring order, overlaps box i -- steps 1 to 5.  Steps 1 and 2 (comparisons)
    run over all pairs; steps 3 to 5 over the pairs that pass them, one array element per pair."""
    v, boxes = np.asarray(v, F), np.asarray(boxes, F).reshape(-1, 8)
    idx = np.asarray(idx).reshape(-1, 3)
    n = len(boxes)
    corners = [v[idx[:, m]] for m in range(3)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ok = np.broadcast_to(box_valid(boxes)[:, None], (n, len(idx))).copy()
        # 2. the bounds test on the triangle's own box: selections and comparisons
        for k in range(3):
            ak, bk, ck = (p[:, k] for p in corners)
            tlo, thi = _sel_min(_sel_min(ak, bk), ck), _sel_max(_sel_max(ak, bk), ck)
            ok &= (tlo[None, :] <= boxes[:, 4 + k][:, None]) & (thi[None, :] >= boxes[:, k][:, None])
        bi, ti = np.nonzero(ok)
        lo, hi = [boxes[bi, k] for k in range(3)], [boxes[bi, 4 + k] for k in range(3)]
        a, b, c = ([p[ti, k] for k in range(3)] for p in corners)
        # 3. centre, half extents, the vertices relative to the centre, the edges
        ctr = [F(0.5) * lo[k] + F(0.5) * hi[k] for k in range(3)]
        h = [F(0.5) * hi[k] - F(0.5) * lo[k] for k in range(3)]
        ua, ub, uc = ([p[k] - ctr[k] for k in range(3)] for p in (a, b, c))
        e0, e1, e2 = [ub[k] - ua[k] for k in range(3)], [uc[k] - ub[k] for k in range(3)], [ua[k] - uc[k] for k in range(3)]
        keep = np.ones(len(bi), bool)
        # 4. nine edge axes
        for e, p, q in ((e0, ua, uc), (e1, ub, ua), (e2, uc, ub)):
            for i, j in ((1, 2), (2, 0), (0, 1)):
                p0 = e[i] * p[j] - e[j] * p[i]
                p1 = e[i] * q[j] - e[j] * q[i]
                r = h[i] * np.abs(e[j]) + h[j] * np.abs(e[i])
                keep &= ~((_sel_min(p0, p1) > r) | (_sel_max(p0, p1) < -r))
        # 5. the plane
        nrm = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
        below, above = [(-h[k]) - ua[k] for k in range(3)], [h[k] - ua[k] for k in range(3)]
        vmin = [np.where(nrm[k] > 0, below[k], above[k]) for k in range(3)]
        vmax = [np.where(nrm[k] > 0, above[k], below[k]) for k in range(3)]
        keep &= ~((_dot(nrm, vmin) > 0) | ~(_dot(nrm, vmax) >= 0))
    ok[bi, ti] = keep
    return ok


def counts_of(m):
    return m.sum(axis=1).astype(np.int32)


def rows_of(m, K):
    """rows mode: (n, K) int32 -- per box the smallest min(count, K) authoring indices, ascending, then -1"""
    rows = np.full((len(m), K), -1, np.int32)
    for i, row in enumerate(m):
        prims = np.flatnonzero(row)[:K]
        rows[i, :len(prims)] = prims
    return rows


def csr_of(m, offsets=None, prims=None):
    """CSR mode: (offsets, prims).  offsets None: the exclusive prefix sum of the counts, so every row is complete.  Given offsets (and
    the array `prims` the rows are written into, which keeps whatever lies outside them): row i holds the smallest offsets[i + 1] -
    offsets[i] indices, then -1; a pair out of order is an empty row."""
    if offsets is None:
        offsets = np.zeros(len(m) + 1, np.int64)
        np.cumsum(counts_of(m), dtype=np.int64, out=offsets[1:])
    offsets = np.asarray(offsets, np.int64)
    prims = np.full(int(offsets[-1]), -1, np.int32) if prims is None else prims.copy()
    for i, row in enumerate(m):
        cap = max(int(offsets[i + 1] - offsets[i]), 0)
        mine = np.flatnonzero(row)[:cap]
        prims[offsets[i]:offsets[i] + cap] = -1
        prims[offsets[i]:offsets[i] + len(mine)] = mine
    return offsets, prims


def box_records(lo, hi):
    boxes = np.zeros((len(lo), 8), F)
    boxes[:, 0:3] = lo
    boxes[:, 4:7] = hi
    return boxes


def voxel_records(origin, cell, dims):
    """gx.voxel_boxes, restated: x fastest, lo = float32(i) * cell + origin, hi = float32(i + 1) * cell + origin"""
    o = np.array(origin, F)
    c = np.array([cell] * 3 if np.isscalar(cell) else cell, F)
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    boxes = np.zeros((nx * ny * nz, 8), F)
    for k, i in enumerate((ix, iy, iz)):
        i = i.reshape(-1)
        boxes[:, k] = i.astype(F) * c[k] + o[k]
        boxes[:, 4 + k] = (i + 1).astype(F) * c[k] + o[k]
    return boxes


# ---------------------------------------------------------------- an independent check in float64, geometry only
def sat_gap64(v, idx, boxes, bi, ti):
    """float64, per pair (box bi[k], triangle ti[k]): the largest separation of triangle and box over the 13 axes of the separating-axis
    theorem (three box axes, the triangle's normal, nine edge x axis products), each normalised, so the figure is a length.  Positive:
    they are apart by at least that much along some axis; negative: on every axis they overlap by at least that much.  Degenerate
    axes are skipped.  Knows nothing of the fp32 definition's order of operations."""
    v = np.asarray(v, np.float64)
    idx = np.asarray(idx).reshape(-1, 3)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 8)
    ctr = 0.5 * (boxes[bi, 0:3] + boxes[bi, 4:7])
    h = 0.5 * (boxes[bi, 4:7] - boxes[bi, 0:3])
    tri = [v[idx[ti, m]] - ctr for m in range(3)]           # (pairs, 3) each
    edges = [tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]]
    axes = [np.broadcast_to(np.eye(3)[k], tri[0].shape) for k in range(3)]
    axes.append(np.cross(edges[0], edges[1]))
    axes += [np.cross(np.eye(3)[k], e) for e in edges for k in range(3)]
    gap = np.full(len(ctr), -np.inf)
    for ax in axes:
        length = np.linalg.norm(ax, axis=1)
        good = length > 1e-30
        ax = ax / np.where(good, length, 1.0)[:, None]
        p = np.stack([(t * ax).sum(axis=1) for t in tri])
        r = (h * np.abs(ax)).sum(axis=1)
        g = np.maximum(p.min(axis=0) - r, -r - p.max(axis=0))
        gap = np.where(good, np.maximum(gap, g), gap)
    return gap
