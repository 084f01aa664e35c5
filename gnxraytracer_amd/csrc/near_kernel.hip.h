// near_kernel.hip.h -- neighbour queries on caller-supplied device memory (gnxr_near_device): EVERY triangle within max_distance of a
// point, counted, and the first K of them in ascending (dist2, authoring index) -- or, in the NEAREST mode, the K nearest and no more of
// the tree than they need.  The definition, operation by operation, is in include/gnxr.h ("Neighbour queries"); the proof that the
// NEAREST walk prunes exactly is in DESIGN.md.
//
// One query per lane, grid-stride, a third client of bvh_walk.hip.h beside k_closest_point and k_all_hits.  A triangle's dist2 is
// closest_on_triangle's and a box's bd2 is box_dist2's (closest_kernel.hip.h: called, not copied), so bd2 is a lower bound IN FP32 of the
// dist2 of every triangle under the box.
//   ALL      a box is dropped iff bd2 > r2, a fixed bound; the order of visits does not matter: the first child that stays is entered and
//            the others are pushed as 4-byte references (walk_enter_all, as in k_all_hits).  count = every near triangle, never clamped to K.
//   NEAREST  the bound is r2 until the list is full and the K-th key's dist2 from then on, which only shrinks; children are sorted by bd2
//            and walked nearest-first with (reference, bd2) stack entries, and a popped entry is tested against the bound again
//            (walk_enter_nearest and walk_pop, as in k_closest_point).  A box with bd2 == the K-th dist2 is entered: a smaller authoring index may tie.  count = slots filled.
// No epsilon anywhere.
//
// The list (LIST): the lane's own output row out[i K .. i K + K) IS the list -- a lane re-reads only what it wrote itself --, kept sorted
// by insertion; the number held and the K-th key stay in registers, so a candidate that does not beat a full list costs one comparison
// and no memory.  While the walk runs a slot holds the compact entry (prim, dist2, leaf-order index, 0) in the first dwordx4 of its 32
// bytes, where prim and dist2 already are in their final place; when the query retires every held slot is recomputed from its leaf-order
// index by closest_on_triangle, as k_closest_point does for its winner (the same bits), and the empty slots are filled.  No dynamically
// indexed private array (it would live in scratch).
#pragma once
#include "closest_kernel.hip.h"

namespace gnxr {

struct NearArrays {
    const float4 *queries;   // (p.xyz, max_distance)
    float4 *out;             // 2 K per query: (prim, dist2, p.x, p.y), (p.z, b1, b2, feature); nullptr when K == 0
    int *counts;             // per query
    int K;
};

// The list of one query: its output row, sorted by (dist2, prim); `held` entries, and the K-th key once it is full.
struct NearList {
    float4 *row;   // slot j's compact entry is row[2 j]
    int K, held;
    float kd;
    int kp;
    GX_DEV void insert(float d2, int prim, int leaf) {
        if (held == K && !(d2 < kd || (d2 == kd && prim < kp))) return;
        const int last = held < K ? held : K - 1;   // the slot the list grows into; a full list drops its entry there
        float ld = d2;                              // the key that ends up in `last`: the new entry's, or that of the first entry moved
        int lp = prim;
        int j = last;
        while (j > 0) {
            const float4 e = row[2 * (j - 1)];
            if (e.y < d2 || (e.y == d2 && __float_as_int(e.x) < prim)) break;
            if (j == last) { ld = e.y; lp = __float_as_int(e.x); }
            row[2 * j] = e;
            --j;
        }
        row[2 * j] = make_float4(__int_as_float(prim), d2, __int_as_float(leaf), 0.f);
        if (held < K) ++held;
        if (held == K) { kd = ld; kp = lp; }   // `last` is slot K - 1 then: the K-th key without reading it back
    }
};

GX_DEV void near_empty_slot(float4 *slot) {
    slot[0] = make_float4(__int_as_float(-1), GX_INF, 0.f, 0.f);
    slot[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// a stack entry: NEAREST (child reference, bd2 bits), ALL the child reference alone
template <bool NEAREST> struct NearEntry { typedef int type; };
template <> struct NearEntry<true> { typedef uint2 type; };

// WIDE: the 4-wide tree from sc.root4; else the binary tree from node 0.  NEAREST: the mode (it implies LIST).  LIST: K > 0 (else the
// count alone; no list memory is touched).  COUNT: nodes visited and triangles tested of the whole launch are added to work[0], work[1]
// (the measurement's instantiation; never the timed path).
template <bool WIDE, bool NEAREST, bool LIST, bool COUNT>
static __global__ void __launch_bounds__(kBlock) k_near(DScene sc, NearArrays qa, const uint32_t *__restrict__ order, long long n, int lds_entries, int entries, void *spill,
                                                        unsigned long long *work) {
    static_assert(LIST || !NEAREST, "the NEAREST mode keeps a list");
    typedef typename NearEntry<NEAREST>::type Entry;
    extern __shared__ uint2 near_stack_lds[];
    WalkStack<Entry> stack;
    stack.init(reinterpret_cast<Entry *>(near_stack_lds), reinterpret_cast<Entry *>(spill), lds_entries, entries);
    unsigned long long cntNodes = 0, cntTris = 0;
    for (long long slot = blockIdx.x * (long long)kBlock + threadIdx.x; slot < n; slot += stack.threads) {
        const long long i = order ? (long long)order[slot] : slot;   // binned: the slot-th query in Morton order
        const float4 rec = qa.queries[i];
        const V3 q(rec.x, rec.y, rec.z);
        const float r2 = rec.w * rec.w;
        int count = 0;
        NearList list;
        list.row = LIST ? qa.out + 2 * (i * (long long)qa.K) : nullptr;
        list.K = qa.K; list.held = 0; list.kd = r2; list.kp = 0x7fffffff;
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
                    for (int j = 0; j < node.count; ++j) {
                        V3 a, b, c;
                        load_tri(sc.tris, node.first + j, &a, &b, &c);
                        ClosestOnTri unused;
                        const float d2 = closest_on_triangle(a, b, c, q, &unused);
                        if (!(d2 <= r2)) continue;   // a NaN fails
                        ++count;
                        if (LIST) list.insert(d2, sc.tris[node.first + j].prim, node.first + j);
                    }
                } else {
                    const float bound = NEAREST ? list.kd : r2;   // kd is r2 until the list is full
                    int r[4]; unsigned k[4]; bool e[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int s, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        r[s] = ref;
                        k[s] = walk_key<WIDE>(ref, box_dist2(lox, loy, loz, hix, hiy, hiz, q), bound);
                        e[s] = k[s] != kWalkDropped;
                    });
                    if (NEAREST) next = walk_enter_nearest<WIDE>(r, k, [&](int ref, unsigned key) __attribute__((always_inline)) { stack.put_child(sp, ref, key); });
                    else next = walk_enter_all<WIDE>(r, e, [&](int ref) __attribute__((always_inline)) { stack.put_child(sp, ref, 0u); });
                }
                next = walk_pop(stack, sp, next, [&](Entry e) __attribute__((always_inline)) { return walk_within(e, list.kd); });   // NEAREST: the K-th key may have shrunk since the push
                if (next == kNode4Empty) break;
                cur = next;
            }
        }
        qa.counts[i] = NEAREST ? list.held : count;
        if (LIST) {
            for (int j = 0; j < list.held; ++j) {
                const float4 e = list.row[2 * j];
                V3 a, b, c;
                load_tri(sc.tris, __float_as_int(e.z), &a, &b, &c);
                ClosestOnTri r;
                const float d2 = closest_on_triangle(a, b, c, q, &r);
                list.row[2 * j] = make_float4(e.x, d2, r.p.x, r.p.y);
                list.row[2 * j + 1] = make_float4(r.p.z, r.b1, r.b2, __int_as_float(r.feature));
            }
            for (int j = list.held; j < list.K; ++j) near_empty_slot(list.row + 2 * j);
        }
    }
    if (COUNT) {
        atomicAdd(&work[0], cntNodes);
        atomicAdd(&work[1], cntTris);
    }
}

}  // namespace gnxr
