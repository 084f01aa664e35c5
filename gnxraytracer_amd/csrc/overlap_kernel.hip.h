// overlap_kernel.hip.h -- box overlap queries on caller-supplied device memory (gnxr_overlap_box_device): EVERY triangle that touches an
// axis-aligned box, counted, and the smallest authoring indices among them, ascending, in the lane's own output row.  The definition,
// operation by operation, is in include/gnxr.h ("Overlap queries"); why the walk below finds exactly those triangles is in DESIGN.md.
//
// One box per lane, grid-stride, in caller order: a fifth client of bvh_walk.hip.h.  A triangle overlaps iff the closed bounds test on
// the box of its own three vertices passes AND neither the nine edge axes nor the plane separate it (overlap_tri).  A node's box is the
// min / max of the vertices under it, so the bounds test with its exact comparisons passes on every node that encloses a triangle whose
// own box passes: the bounds test alone is applied inside the tree, it prunes with no epsilon, and the result does not depend on the
// tree.  The order of visits does not matter: the first child that stays is entered and the others are pushed as 4-byte references
// (walk_enter_all); nothing shrinks, so every deferred child is walked.
//
// The list (LIST): the lane's own row of int32 authoring indices IS the list -- a lane re-reads only what it wrote itself --, kept
// ascending by insertion; the number held and the largest index of a full row stay in registers, so a triangle that does not beat a
// full row costs one comparison and no memory.  The row is prims[i K .. i K + K) (rows mode) or prims[offsets[i] .. offsets[i + 1])
// (CSR mode); nothing outside it is written.  An insertion moves the entries above the new one, so a row of length L costs O(L^2)
// dword moves in the worst case (DESIGN.md has the measurement).  No dynamically indexed private array (it would live in scratch).
#pragma once
#include "bvh_walk.hip.h"

namespace gnxr {

struct OverlapArrays {
    const float4 *boxes;          // gnxr_box_query i = boxes[2 i] (lo.xyz, pad), boxes[2 i + 1] (hi.xyz, pad)
    const long long *offsets;     // CSR mode: n + 1 row starts into prims; nullptr in rows mode
    int *prims;                   // the rows; nullptr in the count-only form
    int *counts;                  // per box
    int K;                        // rows mode: the length of every row
};

// the box as the tests see it: the bounds for the comparisons, centre and half extents for the separating axes
struct OverlapBox {
    V3 lo, hi, ctr, h;
};

// closed overlap of [lo, hi] with the query's bounds: comparisons only
GX_DEV bool overlap_bounds(const OverlapBox &q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    return lox <= q.hi.x && hix >= q.lo.x && loy <= q.hi.y && hiy >= q.lo.y && loz <= q.hi.z && hiz >= q.lo.z;
}

// One edge axis (box axis k crossed with the edge e; i, j the two other axes in cyclic order): ei = e[i], ej = e[j]; (pi, pj) and
// (qi, qj) the same components of the two vertices with distinct projections; hi_, hj the half extents.  true: the axis separates.
GX_DEV bool overlap_axis_separates(float ei, float ej, float pi, float pj, float qi, float qj, float hi_, float hj) {
    const float p0 = ei * pj - ej * pi;
    const float p1 = ei * qj - ej * qi;
    const float r = hi_ * fabsf(ej) + hj * fabsf(ei);
    return sel_min(p0, p1) > r || sel_max(p0, p1) < -r;
}

// the three box axes crossed with edge e; p, q: the edge's first vertex and the vertex off the edge
GX_DEV bool overlap_edge_separates(V3 e, V3 p, V3 q, V3 h) {
    return overlap_axis_separates(e.y, e.z, p.y, p.z, q.y, q.z, h.y, h.z) ||   // x: i = y, j = z
           overlap_axis_separates(e.z, e.x, p.z, p.x, q.z, q.x, h.z, h.x) ||   // y: i = z, j = x
           overlap_axis_separates(e.x, e.y, p.x, p.y, q.x, q.y, h.x, h.y);     // z: i = x, j = y
}

// steps 2 - 5 of the definition
GX_DEV bool overlap_tri(const OverlapBox &q, V3 a, V3 b, V3 c) {
    V3 tlo, thi;
    tri_own_box(a, b, c, &tlo, &thi);
    if (!overlap_bounds(q, tlo.x, tlo.y, tlo.z, thi.x, thi.y, thi.z)) return false;
    const V3 ua(a.x - q.ctr.x, a.y - q.ctr.y, a.z - q.ctr.z), ub(b.x - q.ctr.x, b.y - q.ctr.y, b.z - q.ctr.z), uc(c.x - q.ctr.x, c.y - q.ctr.y, c.z - q.ctr.z);
    const V3 e0(ub.x - ua.x, ub.y - ua.y, ub.z - ua.z), e1(uc.x - ub.x, uc.y - ub.y, uc.z - ub.z), e2(ua.x - uc.x, ua.y - uc.y, ua.z - uc.z);
    if (overlap_edge_separates(e0, ua, uc, q.h) || overlap_edge_separates(e1, ub, ua, q.h) || overlap_edge_separates(e2, uc, ub, q.h)) return false;
    const V3 n(e0.y * e1.z - e0.z * e1.y, e0.z * e1.x - e0.x * e1.z, e0.x * e1.y - e0.y * e1.x);
    const V3 below(-q.h.x - ua.x, -q.h.y - ua.y, -q.h.z - ua.z), above(q.h.x - ua.x, q.h.y - ua.y, q.h.z - ua.z);
    const V3 vmin(n.x > 0.f ? below.x : above.x, n.y > 0.f ? below.y : above.y, n.z > 0.f ? below.z : above.z);
    const V3 vmax(n.x > 0.f ? above.x : below.x, n.y > 0.f ? above.y : below.y, n.z > 0.f ? above.z : below.z);
    const float dmin = (n.x * vmin.x + n.y * vmin.y) + n.z * vmin.z;
    const float dmax = (n.x * vmax.x + n.y * vmax.y) + n.z * vmax.z;
    return !(dmin > 0.f || !(dmax >= 0.f));
}

// The list of one box: its output row, ascending; `held` entries, and the largest of them once the row is full.
struct OverlapList {
    int *row;
    int cap, held;
    int top;   // a full row's last entry: a prim at or above it does not enter.  -1 for a row without slots: no prim is below it
    GX_DEV void insert(int prim) {
        if (held == cap && prim >= top) return;
        const int last = held < cap ? held : cap - 1;   // the slot the row grows into; a full row drops its entry there
        int lp = prim;                                  // what ends up in `last`: the new entry, or the first entry moved
        int j = last;
        while (j > 0) {
            const int e = row[j - 1];
            if (e < prim) break;
            if (j == last) lp = e;
            row[j] = e;
            --j;
        }
        row[j] = prim;
        if (held < cap) ++held;
        if (held == cap) top = lp;   // `last` is slot cap - 1 then: the largest entry without reading it back
    }
};

// WIDE: the 4-wide tree from sc.root4; else the binary tree from node 0.  LIST: rows are kept (else the count alone; no list memory is
// touched).  COUNT: nodes visited and triangles tested of the whole launch are added to work[0], work[1] (the measurement's
// instantiation; never the timed path).
template <bool WIDE, bool LIST, bool COUNT>
static __global__ void __launch_bounds__(kBlock) k_overlap_box(DScene sc, OverlapArrays qa, long long n, int lds_entries, int entries, int *spill, unsigned long long *work) {
    extern __shared__ int ov_stack_lds[];
    WalkStack<int> stack;   // of child references
    stack.init(ov_stack_lds, spill, lds_entries, entries);
    unsigned long long cntNodes = 0, cntTris = 0;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += stack.threads) {
        const float4 b0 = qa.boxes[2 * i], b1 = qa.boxes[2 * i + 1];
        OverlapBox q;
        q.lo = V3(b0.x, b0.y, b0.z); q.hi = V3(b1.x, b1.y, b1.z);
        q.ctr = V3(0.5f * q.lo.x + 0.5f * q.hi.x, 0.5f * q.lo.y + 0.5f * q.hi.y, 0.5f * q.lo.z + 0.5f * q.hi.z);
        q.h = V3(0.5f * q.hi.x - 0.5f * q.lo.x, 0.5f * q.hi.y - 0.5f * q.lo.y, 0.5f * q.hi.z - 0.5f * q.lo.z);
        int count = 0;
        OverlapList list;
        list.row = nullptr; list.cap = 0; list.held = 0;
        if (LIST) {
            if (qa.offsets) {   // CSR: the row is what the two offsets span, and nothing when they are out of order
                const long long first = qa.offsets[i], len = qa.offsets[i + 1] - first;
                list.row = qa.prims + first;
                list.cap = len <= 0 ? 0 : len > 0x7fffffffll ? 0x7fffffff : (int)len;
            } else {
                list.row = qa.prims + i * (long long)qa.K;
                list.cap = qa.K;
            }
        }
        list.top = list.cap > 0 ? 0x7fffffff : -1;
        // nothing overlaps an inverted box, a NaN bound (the comparison fails) or an infinite one
        const bool valid = q.lo.x <= q.hi.x && q.lo.y <= q.hi.y && q.lo.z <= q.hi.z && gx_finite(q.lo.x) && gx_finite(q.lo.y) && gx_finite(q.lo.z) &&
                           gx_finite(q.hi.x) && gx_finite(q.hi.y) && gx_finite(q.hi.z);
        if (valid) {
            int sp = 0;
            int cur = WIDE ? sc.root4 : 0;
            while (true) {
                const WalkNode node = walk_decode<WIDE>(sc, cur);
                if (COUNT) cntNodes++;
                int next = kNode4Empty;   // the child to enter, or none
                if (node.leaf) {
                    if (COUNT) cntTris += (unsigned)node.count;
                    for (int j = 0; j < node.count; ++j) {
                        V3 a, b, c;
                        load_tri(sc.tris, node.first + j, &a, &b, &c);
                        if (!overlap_tri(q, a, b, c)) continue;
                        ++count;
                        if (LIST) list.insert(sc.tris[node.first + j].prim);
                    }
                } else {
                    int r[4]; bool e[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int s, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        r[s] = ref;
                        e[s] = !(WIDE && ref == kNode4Empty) && overlap_bounds(q, lox, loy, loz, hix, hiy, hiz);
                    });
                    next = walk_enter_all<WIDE>(r, e, [&](int ref) __attribute__((always_inline)) { stack.put_child(sp, ref, 0u); });
                }
                if (next == kNode4Empty) {   // nothing shrinks, so every deferred child is walked: no walk_pop and its test
                    if (sp == 0) break;
                    next = stack.get(--sp);
                }
                cur = next;
            }
        }
        qa.counts[i] = count;
        if (LIST)
            for (int j = list.held; j < list.cap; ++j) list.row[j] = -1;
    }
    if (COUNT) {
        atomicAdd(&work[0], cntNodes);
        atomicAdd(&work[1], cntTris);
    }
}

}  // namespace gnxr
