// closest_kernel.hip.h -- closest-point queries on caller-supplied device memory (gnxr_closest_point_device): which triangle is nearest to
// a point, where on it, and how far.  The definition, operation by operation, is in include/gnxr.h ("Closest-point queries"); the proof
// that the walk below prunes exactly is in DESIGN.md.
//
// One query per lane.  The walk is nearest-first by box distance over the 4-wide tree (DScene::nodes4) or, for scenes that are off it, over
// the binary tree (DScene::nodes): at a node the squared distance bd2 from the query to each child's box is computed in the same fp32
// operations as a triangle's dist2, children with bd2 > best are dropped, the nearest survivor is entered and the others go onto the stack,
// farthest first, as (child reference, bd2) pairs; a popped entry is tested against the current best again before its memory is touched.
// bd2 is a lower bound IN FP32 of the dist2 of every triangle under the box (the closest point is clamped into the triangle's own bounds,
// every box encloses those, and subtraction, squaring and addition round monotonically), so `bd2 > best` never drops the winner and
// `bd2 == best` is entered because a smaller authoring index may tie.  No epsilon anywhere.
//
// The stack (8-byte entries), the node decode, the children's boxes, the sort with its keys and the pop are bvh_walk.hip.h's.
//
// Queries arrive in caller order, and neighbouring lanes that walk to different corners of the tree share neither node loads nor control
// flow.  From kClosestBinMin queries on, the call therefore bins them first: an 18-bit Morton key of p over the root's box (64 cells per
// axis; k_closest_keys), three passes of the HLBVH stage's radix sort over (key, index), and the walk takes its queries through the sorted
// indices -- it gathers the record and scatters the result itself, so nothing else moves.  The key orders the work and nothing more: the
// records are the same bytes with and without it (DESIGN.md has both timings).
#pragma once
#include "bvh_walk.hip.h"
#include "hlbvh_build.hip.h"

namespace gnxr {

// gnxr_point_query / gnxr_closest_point as the kernel moves them: one and two dwordx4
struct ClosestArrays {
    const float4 *queries;   // (p.xyz, max_distance)
    float4 *out;             // 2 per query: (prim, dist2, p.x, p.y), (p.z, b1, b2, feature)
};

GX_DEV float cp_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
GX_DEV float cp_clamp(float p, float lo, float hi) { return p < lo ? lo : (p > hi ? hi : p); }

struct ClosestOnTri {
    V3 p;
    float b1, b2;
    int feature;
};

// Ericson, Real-Time Collision Detection 5.1.5 (ClosestPtPointTriangle) in its order of tests, then the clamp into the triangle's bounds.
// Returns dist2.  Callers that only compare distances ignore `r`; its barycentrics and feature then cost nothing.
GX_DEV float closest_on_triangle(V3 a, V3 b, V3 c, V3 q, ClosestOnTri *r) {
    const V3 ab = b - a, ac = c - a, ap = q - a;
    const float d1 = cp_dot(ab, ap), d2 = cp_dot(ac, ap);
    V3 p;
    float b1, b2;
    int feature;
    do {
        if (d1 <= 0.f && d2 <= 0.f) { p = a; b1 = 0.f; b2 = 0.f; feature = 4; break; }
        const V3 bp = q - b;
        const float d3 = cp_dot(ab, bp), d4 = cp_dot(ac, bp);
        if (d3 >= 0.f && d4 <= d3) { p = b; b1 = 1.f; b2 = 0.f; feature = 5; break; }
        const float vc = d1 * d4 - d3 * d2;
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
            const float v = d1 / (d1 - d3);
            p = a + v * ab; b1 = v; b2 = 0.f; feature = 1;
            break;
        }
        const V3 cp = q - c;
        const float d5 = cp_dot(ab, cp), d6 = cp_dot(ac, cp);
        if (d6 >= 0.f && d5 <= d6) { p = c; b1 = 0.f; b2 = 1.f; feature = 6; break; }
        const float vb = d5 * d2 - d1 * d6;
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
            const float w = d2 / (d2 - d6);
            p = a + w * ac; b1 = 0.f; b2 = w; feature = 2;
            break;
        }
        const float va = d3 * d6 - d5 * d4;
        if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
            const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            p = b + w * (c - b); b1 = 1.f - w; b2 = w; feature = 3;
            break;
        }
        const float denom = 1.f / ((va + vb) + vc);
        const float v = vb * denom, w = vc * denom;
        p = (a + v * ab) + w * ac; b1 = v; b2 = w; feature = 0;
    } while (false);
    V3 lo, hi;
    tri_own_box(a, b, c, &lo, &hi);
    p = V3(cp_clamp(p.x, lo.x, hi.x), cp_clamp(p.y, lo.y, hi.y), cp_clamp(p.z, lo.z, hi.z));
    const V3 d = q - p;
    r->p = p; r->b1 = b1; r->b2 = b2; r->feature = feature;
    return cp_dot(d, d);
}

// squared distance from q to the box [lo, hi], per axis e = max(max(lo - q, q - hi), 0): the shape of a triangle's dist2
GX_DEV float box_dist2(float lox, float loy, float loz, float hix, float hiy, float hiz, V3 q) {
    const float ex = sel_max(sel_max(lox - q.x, q.x - hix), 0.f);
    const float ey = sel_max(sel_max(loy - q.y, q.y - hiy), 0.f);
    const float ez = sel_max(sel_max(loz - q.z, q.z - hiz), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}

// best = (dist2, authoring index) in lexicographic order; it starts at (r2, INT_MAX), which makes `dist2 <= r2` and the tie rule one test
struct ClosestBest {
    float d2;
    int prim;
    int leaf;   // the winner's leaf-order index (-1: none yet)
};
GX_DEV void closest_leaf(const DTri *__restrict__ tris, int first, int n, V3 q, ClosestBest *best) {
    for (int i = 0; i < n; ++i) {
        V3 a, b, c;
        load_tri(tris, first + i, &a, &b, &c);
        const int prim = tris[first + i].prim;
        ClosestOnTri unused;
        const float d2 = closest_on_triangle(a, b, c, q, &unused);
        if (d2 < best->d2 || (d2 == best->d2 && prim < best->prim)) { best->d2 = d2; best->prim = prim; best->leaf = first + i; }   // a NaN fails both
    }
}

// WIDE: the 4-wide tree from sc.root4; else the binary tree from node 0.  COUNT: nodes visited and triangles tested of the whole launch are
// added to counts[0], counts[1] (the measurement's instantiation; never the timed path).  A stack entry is (child reference, key).
template <bool WIDE, bool COUNT>
static __global__ void __launch_bounds__(kBlock) k_closest_point(DScene sc, ClosestArrays qa, const uint32_t *__restrict__ order, long long n, int lds_entries, int entries,
                                                                 uint2 *spill, unsigned long long *counts) {
    extern __shared__ uint2 cp_stack_lds[];
    WalkStack<uint2> stack;
    stack.init(cp_stack_lds, spill, lds_entries, entries);
    unsigned long long cntNodes = 0, cntTris = 0;
    for (long long slot = blockIdx.x * (long long)kBlock + threadIdx.x; slot < n; slot += stack.threads) {
        const long long i = order ? (long long)order[slot] : slot;   // binned: the slot-th query in Morton order
        const float4 rec = qa.queries[i];
        const V3 q(rec.x, rec.y, rec.z);
        const float r2 = rec.w * rec.w;
        ClosestBest best = {r2, 0x7fffffff, -1};
        const bool valid = rec.w >= 0.f && q.x == q.x && q.y == q.y && q.z == q.z;   // a NaN max_distance fails the first test
        if (valid) {
            int sp = 0;
            int cur = WIDE ? sc.root4 : 0;
            while (true) {
                const WalkNode node = walk_decode<WIDE>(sc, cur);
                if (COUNT) cntNodes++;
                int next = kNode4Empty;   // the child to enter, or none
                if (node.leaf) {
                    if (COUNT) cntTris += (unsigned)node.count;
                    closest_leaf(sc.tris, node.first, node.count, q, &best);
                } else {
                    int r[4]; unsigned k[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int s, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        r[s] = ref;
                        k[s] = walk_key<WIDE>(ref, box_dist2(lox, loy, loz, hix, hiy, hiz, q), best.d2);
                    });
                    next = walk_enter_nearest<WIDE>(r, k, [&](int ref, unsigned key) __attribute__((always_inline)) { stack.put_child(sp, ref, key); });
                }
                next = walk_pop(stack, sp, next, [&](uint2 e) __attribute__((always_inline)) { return walk_within(e, best.d2); });   // the best may have shrunk since the push
                if (next == kNode4Empty) break;
                cur = next;
            }
        }
        float4 o0 = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f), o1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (best.leaf >= 0) {
            V3 a, b, c;
            load_tri(sc.tris, best.leaf, &a, &b, &c);
            ClosestOnTri r;
            const float d2 = closest_on_triangle(a, b, c, q, &r);
            o0 = make_float4(__int_as_float(best.prim), d2, r.p.x, r.p.y);
            o1 = make_float4(r.p.z, r.b1, r.b2, __int_as_float(r.feature));
        }
        qa.out[2 * i] = o0;
        qa.out[2 * i + 1] = o1;
    }
    if (COUNT) {
        atomicAdd(&counts[0], cntNodes);
        atomicAdd(&counts[1], cntTris);
    }
}

// The binning key of each query and its index: the cell of p in a 64^3 grid over the root's box (node 0 of the binary tree, which every
// scene has), interleaved.  Points outside land in the border cells; a NaN lands in cell 0 (fmaxf drops it).
static __global__ void __launch_bounds__(kBlock) k_closest_keys(const float4 *__restrict__ nodes, const float4 *__restrict__ queries, int n, uint32_t *__restrict__ keys,
                                                                uint32_t *__restrict__ vals) {
    const float4 n0 = nodes[0], n1 = nodes[1];   // (lo.xyz, hi.x), (hi.y, hi.z, ..)
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 q = queries[i];
        const uint32_t cx = (uint32_t)fminf(fmaxf((q.x - n0.x) / (n0.w - n0.x) * 64.f, 0.f), 63.f);
        const uint32_t cy = (uint32_t)fminf(fmaxf((q.y - n0.y) / (n1.x - n0.y) * 64.f, 0.f), 63.f);
        const uint32_t cz = (uint32_t)fminf(fmaxf((q.z - n0.z) / (n1.y - n0.z) * 64.f, 0.f), 63.f);
        keys[i] = (hlbvh::left_shift3(cz) << 2) | (hlbvh::left_shift3(cy) << 1) | hlbvh::left_shift3(cx);
        vals[i] = (uint32_t)i;
    }
}

}  // namespace gnxr
