"""BVHAccel::HLBVHBuild (accelerator/BVHAccel.cpp:369-626) with maxPrimsInNode = 1, restated in numpy float32.

TEST INFRASTRUCTURE: the plain reference tests/test_hlbvh_build.py compares the device build (csrc/hlbvh_build.hip.h) with.  It is
sequential on purpose -- a stable argsort where the device has its own radix sort, a top-down walk with binary searches where the
device has the closed form per Karras node, a recursion (kept on an explicit stack) where the device runs one launch per level -- and
it is itself pinned to three dumps of the compiled reference by the CPU tests of that module.

    bounds, meta, order = hlbvh_reference(vertices, indices)

takes the world-space arrays of SceneBuilder.desc() and returns what Scene.bvh() returns: the flattened pre-order tree (LinearBVHNode[]:
child 0 follows its parent, child 1 sits at `offset`), meta = offset / nPrimitives / axis, and the primitive order.  All arithmetic is
np.float32, one rounding per operation (the reference is built without fused multiply-adds).  Where the reference's CHECKs would fire
(no centroid extent among the treelet roots of a range, an empty side after the split) or a leaf would not fit LinearBVHNode's 16-bit
count, it raises ValueError.
"""
from bisect import bisect_left

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
N_BUCKETS = 12
TREELET_SHIFT = 18            # a treelet = a run of equal top 12 of the 30 code bits


def primitive_boxes(vertices, indices):
    """(lo [n,3], hi [n,3], centroid [n,3]): Triangle::WorldBound and BVHPrimitiveInfo::centroid = .5f * pMin + .5f * pMax."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    p0, p1, p2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    lo = np.minimum(np.minimum(p0, p1), p2)
    hi = np.maximum(np.maximum(p0, p1), p2)
    return lo, hi, F(.5) * lo + F(.5) * hi


def _left_shift3(x):
    x = np.where(x == 1 << 10, x - 1, x).astype(np.uint32)
    x = (x | (x << 16)) & 0x30000ff
    x = (x | (x << 8)) & 0x300f00f
    x = (x | (x << 4)) & 0x30c30c3
    x = (x | (x << 2)) & 0x9249249
    return x


def morton_codes(cen):
    """EncodeMorton3(bounds.Offset(centroid) * 1024) for every centroid; Bounds3::Offset divides only on axes with hi > lo."""
    clo, chi = cen.min(axis=0), cen.max(axis=0)
    o = cen - clo
    for a in range(3):
        if chi[a] > clo[a]:
            o[:, a] = o[:, a] / (chi[a] - clo[a])
    q = (o * F(1 << 10)).astype(np.uint32)      # truncation; the values lie in [0, 1024]
    return (_left_shift3(q[:, 2]) << 2) | (_left_shift3(q[:, 1]) << 1) | _left_shift3(q[:, 0])


def code_runs(sorted_codes):
    """(distinct codes, start of each run of equal codes in the sorted array): the LBVH leaves"""
    head = np.ones(len(sorted_codes), bool)
    head[1:] = sorted_codes[1:] != sorted_codes[:-1]
    start = np.flatnonzero(head)
    return sorted_codes[start], start


def _area(lo, hi):
    x, y, z = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return F(2) * ((x * y + x * z) + y * z)


def _split_upper(blo, bhi):
    """One step of buildUpperSAH over the treelet roots with boxes (blo, bhi), in their current order: (dim, goes_left [k] bool)."""
    c = (blo + bhi) * F(.5)
    clo, chi = c.min(axis=0), c.max(axis=0)
    d = chi - clo
    dim = 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)      # Bounds3::MaximumExtent
    if not chi[dim] != clo[dim]:
        raise ValueError("HLBVH: treelet roots without centroid extent (CHECK_NE in buildUpperSAH)")
    bucket = (F(N_BUCKETS) * ((c[:, dim] - clo[dim]) / (chi[dim] - clo[dim]))).astype(np.int32)
    bucket[bucket == N_BUCKETS] = N_BUCKETS - 1
    if bucket.min() < 0 or bucket.max() >= N_BUCKETS:
        raise ValueError("HLBVH: SAH bucket out of range (CHECK_GE / CHECK_LT in buildUpperSAH)")
    count = np.zeros(N_BUCKETS, np.int64)
    lo = np.full((N_BUCKETS, 3), FLT_MAX, np.float32)        # an empty Bounds3 is (FLT_MAX, -FLT_MAX)
    hi = np.full((N_BUCKETS, 3), -FLT_MAX, np.float32)
    for b in range(N_BUCKETS):
        m = bucket == b
        if m.any():
            count[b] = m.sum()
            lo[b], hi[b] = blo[m].min(axis=0), bhi[m].max(axis=0)
    total = _area(blo.min(axis=0), bhi.max(axis=0))
    cost = np.zeros(N_BUCKETS - 1, np.float32)
    for i in range(N_BUCKETS - 1):
        a0 = _area(lo[:i + 1].min(axis=0), hi[:i + 1].max(axis=0))
        a1 = _area(lo[i + 1:].min(axis=0), hi[i + 1:].max(axis=0))
        cost[i] = F(.125) + (F(count[:i + 1].sum()) * a0 + F(count[i + 1:].sum()) * a1) / total     # an empty side: 0 * inf = NaN
    split = 0
    for i in range(1, N_BUCKETS - 1):
        if cost[i] < cost[split]:       # a NaN never wins, the first minimum does
            split = i
    left = bucket <= split
    if not left.any() or left.all():
        raise ValueError("HLBVH: an empty side after the SAH split (CHECK_GT / CHECK_LT in buildUpperSAH)")
    return dim, left


def hlbvh_reference(vertices, indices):
    plo, phi, cen = primitive_boxes(vertices, indices)
    n = len(plo)
    if n == 0:
        raise ValueError("HLBVH: no primitives")
    codes = morton_codes(cen)
    order = np.argsort(codes, kind="stable").astype(np.int32)
    ukey, ustart = code_runs(codes[order])
    U = len(ukey)
    if np.diff(np.append(ustart, n)).max() > 0xffff:
        raise ValueError("HLBVH: a leaf exceeds 65535 primitives (CHECK_LT in flattenBVHTree)")

    # ---- build nodes: [0, U) are the leaves (run u of equal codes, in sorted order), interior nodes are appended
    c0, c1, axis, depth = [-1] * U, [-1] * U, [0] * U, [0] * U
    keys = [int(k) for k in ukey]

    def new_interior(ax, dep):
        c0.append(-1); c1.append(-1); axis.append(ax); depth.append(dep)
        return len(c0) - 1

    # one LBVH per treelet (emitLBVH): a range of runs splits at the highest bit in which its first and last code differ, at the first
    # run that has the bit set; a range of one run is a leaf (the bits run out without a split)
    thead = np.ones(U, bool)
    thead[1:] = (ukey[1:] >> TREELET_SHIFT) != (ukey[:-1] >> TREELET_SHIFT)
    tstart = np.flatnonzero(thead).tolist() + [U]
    roots = []
    for t in range(len(tstart) - 1):
        stack = [(tstart[t], tstart[t + 1], -1, 0, 0)]          # runs [a, b), parent node, which child, depth
        while stack:
            a, b, parent, which, dep = stack.pop()
            if b - a == 1:
                me = a
                depth[me] = dep
            else:
                bit = (keys[a] ^ keys[b - 1]).bit_length() - 1
                first_set = ((keys[a] >> bit) | 1) << bit        # the smallest code of this range's prefix with the bit set
                mid = bisect_left(keys, first_set, a, b)
                me = new_interior(bit % 3, dep)
                stack.append((mid, b, me, 1, dep + 1))
                stack.append((a, mid, me, 0, dep + 1))
            if parent < 0:
                roots.append(me)
            elif which == 0:
                c0[parent] = me
            else:
                c1[parent] = me
    n_lbvh = len(c0)
    blo = np.zeros((n_lbvh, 3), np.float32)
    bhi = np.zeros((n_lbvh, 3), np.float32)
    blo[:U] = np.minimum.reduceat(plo[order], ustart, axis=0)
    bhi[:U] = np.maximum.reduceat(phi[order], ustart, axis=0)
    # interior boxes = union of the children, deepest level first
    c0a, c1a, dpa = np.array(c0), np.array(c1), np.array(depth)
    interior = np.arange(U, n_lbvh)
    for dep in range(int(dpa[U:].max()) if n_lbvh > U else -1, -1, -1):
        ids = interior[dpa[U:] == dep]
        blo[ids] = np.minimum(blo[c0a[ids]], blo[c1a[ids]])
        bhi[ids] = np.maximum(bhi[c0a[ids]], bhi[c1a[ids]])

    # ---- buildUpperSAH over the treelet roots
    up_lo, up_hi = [], []          # boxes of the upper nodes, numbered from n_lbvh
    roots = np.array(roots)
    root = roots[0]
    if len(roots) > 1:
        with np.errstate(over="ignore", invalid="ignore"):
            stack = [(0, len(roots), -1, 0)]
            while stack:
                s, e, parent, which = stack.pop()
                if e - s == 1:
                    me = int(roots[s])
                else:
                    r = roots[s:e]
                    dim, left = _split_upper(blo[r], bhi[r])
                    roots[s:e] = np.concatenate([r[left], r[~left]])
                    mid = s + int(left.sum())
                    me = new_interior(dim, 0)
                    up_lo.append(blo[r].min(axis=0)); up_hi.append(bhi[r].max(axis=0))     # == Union(child 0, child 1)
                    stack.append((mid, e, me, 1))
                    stack.append((s, mid, me, 0))
                if parent < 0:
                    root = me
                elif which == 0:
                    c0[parent] = me
                else:
                    c1[parent] = me
        blo = np.concatenate([blo, np.array(up_lo, np.float32).reshape(-1, 3)])
        bhi = np.concatenate([bhi, np.array(up_hi, np.float32).reshape(-1, 3)])

    # ---- flattenBVHTree: pre-order, child 0 next, child 1 at `offset`
    total = len(c0)
    src = np.zeros(total, np.int64)            # build node of each flattened node
    meta = np.zeros((total, 3), np.int32)
    run_len = np.diff(np.append(ustart, n))
    k = 0
    stack = [(int(root), -1)]
    while stack:
        node, parent = stack.pop()
        src[k] = node
        if parent >= 0:
            meta[parent, 0] = k
        if node < U:
            meta[k, 0], meta[k, 1] = ustart[node], run_len[node]
        else:
            meta[k, 2] = axis[node]
            stack.append((c1[node], k))
            stack.append((c0[node], -1))
        k += 1
    assert k == total
    bounds = np.concatenate([blo[src], bhi[src]], axis=1)
    return np.ascontiguousarray(bounds, np.float32), meta, order
