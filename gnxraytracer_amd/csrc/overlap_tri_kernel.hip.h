// overlap_tri_kernel.hip.h -- triangle overlap queries on caller-supplied device memory (gnxr_overlap_tri_device): EVERY triangle of the
// scene that touches a query triangle, counted, and the smallest authoring indices among them, ascending, in the lane's own output row.
// The definition, operation by operation, is in include/gnxr.h ("Triangle overlap queries"); DESIGN.md has why the walk finds exactly
// those triangles and what the seventeen axes cost.
//
// One query triangle per lane, grid-stride: the sixth client of bvh_walk.hip.h, built like k_overlap_box (overlap_kernel.hip.h), whose
// closed bounds test (overlap_bounds), list (OverlapList) and row layouts it uses as they are.  Inside the tree the ONLY test is the
// bounds test of the query's own box [qlo, qhi] against a node's box, so the walk visits the nodes the box query of [qlo, qhi] visits,
// prunes with no epsilon, and the result does not depend on the tree.  At a leaf a triangle overlaps iff its own box passes that test,
// it is not skipped for sharing a vertex with the query (skip_shared), and none of the seventeen axes separates the two
// (overlap_tri_tri).  The axes are independent: what depends on the query alone (nq, the three cross(nq, f_i) and the query's
// intervals on those four) is computed once per query, the axes are tested cheapest first and the test stops at the first that
// separates.  The bits are those of the definition's order.
//
// SELF: lane i's query is the scene's own triangle sc.tris[i] -- leaf order, so neighbouring lanes hold neighbouring triangles and walk
// nearly the same path -- and its row, offsets and count are those of that triangle's authoring index.
// No dynamically indexed private array (it would live in scratch).
#pragma once
#include "overlap_kernel.hip.h"

namespace gnxr {

struct OverlapTriArrays {
    const float4 *tris;           // gnxr_tri_query i = tris[3 i] (a.xyz, pad), tris[3 i + 1] (b.xyz, pad), tris[3 i + 2] (c.xyz, pad); nullptr: SELF
    const long long *offsets;     // CSR mode: n + 1 row starts into prims; nullptr in rows mode
    int *prims;                   // the rows; nullptr in the count-only form
    int *counts;                  // per query
    int K;                        // rows mode: the length of every row
    unsigned skip_shared;         // step 3 of the definition applies (always in SELF)
    long long base;               // SELF: the launch's first triangle in leaf order (rows and counts are indexed by authoring index)
};

// two products and a difference per component
GX_DEV V3 tt_cross(V3 u, V3 v) { return V3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }
GX_DEV float tt_dot(V3 u, V3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
GX_DEV bool tt_same(V3 p, V3 q) { return p.x == q.x && p.y == q.y && p.z == q.z; }

// [lo, hi] of {x, y, z} by selection, in the definition's order
struct TriInterval { float lo, hi; };
GX_DEV TriInterval tt_interval(float x, float y, float z) { return {sel_min(sel_min(x, y), z), sel_max(sel_max(x, y), z)}; }
// the query's interval on L: its vertices are 0, ub, uc after the translation
GX_DEV TriInterval tt_query_interval(V3 L, V3 ub, V3 uc) { return tt_interval(0.f, tt_dot(L, ub), tt_dot(L, uc)); }
// does L separate the translated triangle (ta, tb, tc) from the query's interval qi on L?  Closed: touching does not separate
GX_DEV bool tt_separates(V3 L, TriInterval qi, V3 ta, V3 tb, V3 tc) {
    const TriInterval ti = tt_interval(tt_dot(L, ta), tt_dot(L, tb), tt_dot(L, tc));
    return ti.lo > qi.hi || ti.hi < qi.lo;
}
GX_DEV bool tt_axis_separates(V3 L, V3 ub, V3 uc, V3 ta, V3 tb, V3 tc) { return tt_separates(L, tt_query_interval(L, ub, uc), ta, tb, tc); }

// What a query keeps over its walk: the vertices, and step 1's quantities that depend on it alone
struct TriQuery {
    OverlapBox box;               // lo, hi = qlo, qhi (ctr and h are not used)
    V3 a, b, c;
    V3 nq, g0, g1, g2;            // cross(ub, uc) and cross(nq, f_i)
    TriInterval inq, ig0, ig1, ig2;   // the query's intervals on those four
    GX_DEV void set(V3 qa, V3 qb, V3 qc) {
        a = qa; b = qb; c = qc;
        tri_own_box(qa, qb, qc, &box.lo, &box.hi);
        const V3 ub = qb - qa, uc = qc - qa, f1 = uc - ub;
        nq = tt_cross(ub, uc);
        g0 = tt_cross(nq, ub); g1 = tt_cross(nq, f1); g2 = tt_cross(nq, uc);
        inq = tt_query_interval(nq, ub, uc);
        ig0 = tt_query_interval(g0, ub, uc); ig1 = tt_query_interval(g1, ub, uc); ig2 = tt_query_interval(g2, ub, uc);
    }
    GX_DEV bool valid() const {
        return gx_finite(a.x) && gx_finite(a.y) && gx_finite(a.z) && gx_finite(b.x) && gx_finite(b.y) && gx_finite(b.z) && gx_finite(c.x) && gx_finite(c.y) &&
               gx_finite(c.z);
    }
};

// steps 2 - 5 of the definition, the axes in the order nq, nt, cross(nq, f_i), cross(nt, e_j), cross(f_i, e_j)
GX_DEV bool overlap_tri_tri(const TriQuery &q, bool skip_shared, V3 a, V3 b, V3 c) {
    V3 tlo, thi;
    tri_own_box(a, b, c, &tlo, &thi);
    if (!overlap_bounds(q.box, tlo.x, tlo.y, tlo.z, thi.x, thi.y, thi.z)) return false;
    if (skip_shared && (tt_same(q.a, a) || tt_same(q.a, b) || tt_same(q.a, c) || tt_same(q.b, a) || tt_same(q.b, b) || tt_same(q.b, c) || tt_same(q.c, a) ||
                        tt_same(q.c, b) || tt_same(q.c, c)))
        return false;
    const V3 ta = a - q.a, tb = b - q.a, tc = c - q.a;
    if (tt_separates(q.nq, q.inq, ta, tb, tc)) return false;
    const V3 ub = q.b - q.a, uc = q.c - q.a;
    const V3 e0 = tb - ta, e1 = tc - tb, e2 = ta - tc;
    const V3 nt = tt_cross(e0, e1);
    if (tt_axis_separates(nt, ub, uc, ta, tb, tc)) return false;
    if (tt_separates(q.g0, q.ig0, ta, tb, tc) || tt_separates(q.g1, q.ig1, ta, tb, tc) || tt_separates(q.g2, q.ig2, ta, tb, tc)) return false;
    if (tt_axis_separates(tt_cross(nt, e0), ub, uc, ta, tb, tc) || tt_axis_separates(tt_cross(nt, e1), ub, uc, ta, tb, tc) ||
        tt_axis_separates(tt_cross(nt, e2), ub, uc, ta, tb, tc))
        return false;
    const V3 f1 = uc - ub;
    if (tt_axis_separates(tt_cross(ub, e0), ub, uc, ta, tb, tc) || tt_axis_separates(tt_cross(ub, e1), ub, uc, ta, tb, tc) ||
        tt_axis_separates(tt_cross(ub, e2), ub, uc, ta, tb, tc))
        return false;
    if (tt_axis_separates(tt_cross(f1, e0), ub, uc, ta, tb, tc) || tt_axis_separates(tt_cross(f1, e1), ub, uc, ta, tb, tc) ||
        tt_axis_separates(tt_cross(f1, e2), ub, uc, ta, tb, tc))
        return false;
    return !(tt_axis_separates(tt_cross(uc, e0), ub, uc, ta, tb, tc) || tt_axis_separates(tt_cross(uc, e1), ub, uc, ta, tb, tc) ||
             tt_axis_separates(tt_cross(uc, e2), ub, uc, ta, tb, tc));
}

// WIDE, LIST, COUNT: as k_overlap_box.  SELF: the queries are the scene's own triangles (above).
template <bool WIDE, bool LIST, bool COUNT, bool SELF>
static __global__ void __launch_bounds__(kBlock) k_overlap_tri(DScene sc, OverlapTriArrays qa, long long n, int lds_entries, int entries, int *spill, unsigned long long *work) {
    extern __shared__ int ot_stack_lds[];
    WalkStack<int> stack;   // of child references
    stack.init(ot_stack_lds, spill, lds_entries, entries);
    const bool skip_shared = SELF || qa.skip_shared != 0u;
    unsigned long long cntNodes = 0, cntTris = 0;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += stack.threads) {
        TriQuery q;
        long long out = i;   // the query's row, offsets and count
        if (SELF) {
            V3 a, b, c;
            load_tri(sc.tris, (int)(qa.base + i), &a, &b, &c);
            q.set(a, b, c);
            out = sc.tris[qa.base + i].prim;
        } else {
            const float4 t0 = qa.tris[3 * i], t1 = qa.tris[3 * i + 1], t2 = qa.tris[3 * i + 2];
            q.set(V3(t0.x, t0.y, t0.z), V3(t1.x, t1.y, t1.z), V3(t2.x, t2.y, t2.z));
        }
        int count = 0;
        OverlapList list;
        list.row = nullptr; list.cap = 0; list.held = 0;
        if (LIST) {
            if (qa.offsets) {   // CSR: the row is what the two offsets span, and nothing when they are out of order
                const long long first = qa.offsets[out], len = qa.offsets[out + 1] - first;
                list.row = qa.prims + first;
                list.cap = len <= 0 ? 0 : len > 0x7fffffffll ? 0x7fffffff : (int)len;
            } else {
                list.row = qa.prims + out * (long long)qa.K;
                list.cap = qa.K;
            }
        }
        list.top = list.cap > 0 ? 0x7fffffff : -1;
        if (q.valid()) {   // nothing overlaps a triangle with a coordinate that is not finite
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
                        if (!overlap_tri_tri(q, skip_shared, a, b, c)) continue;
                        ++count;
                        if (LIST) list.insert(sc.tris[node.first + j].prim);
                    }
                } else {
                    int r[4]; bool e[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int s, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        r[s] = ref;
                        e[s] = !(WIDE && ref == kNode4Empty) && overlap_bounds(q.box, lox, loy, loz, hix, hiy, hiz);
                    });
                    next = walk_enter_all<WIDE>(r, e, [&](int ref) __attribute__((always_inline)) { stack.put_child(sp, ref, 0u); });
                }
                if (next == kNode4Empty) {   // nothing shrinks, so every deferred child is walked
                    if (sp == 0) break;
                    next = stack.get(--sp);
                }
                cur = next;
            }
        }
        qa.counts[out] = count;
        if (LIST)
            for (int j = list.held; j < list.cap; ++j) list.row[j] = -1;
    }
    if (COUNT) {
        atomicAdd(&work[0], cntNodes);
        atomicAdd(&work[1], cntTris);
    }
}

}  // namespace gnxr
