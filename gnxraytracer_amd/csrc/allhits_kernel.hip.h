// allhits_kernel.hip.h -- all-hits ray queries on caller-supplied device memory (gnxr_trace_all_device): EVERY triangle a ray passes
// through within its tmax, counted, and the first K of them in ascending (t, authoring index).  The definition, operation by operation,
// is in include/gnxr.h ("All-hits ray queries"); the argument that the walk below finds exactly those triangles is in DESIGN.md.
//
// One ray per lane, grid-stride, a kernel of its own beside k_trace4 (which it does not touch).  A triangle is a hit iff the exact
// Bounds3::IntersectP (slab_test) accepts the box of its own three vertices AND the watertight test (tri_test_sheared) accepts it, both
// with the ray's own tmax: nothing shrinks, nothing is pruned by distance.  Because the slab arithmetic is monotone in the box, a triangle
// whose own box passes has every enclosing node box passing, so the tests at interior nodes only choose the subtrees to walk and may be
// any superset of the exact test:
//   finite 1 / d        k_trace4's max3 / min3 form (equal to Bounds3::IntersectP there);
//   any 1 / d not finite (a zero or tiny direction component: 0 * inf = NaN in the exact sequence)
//                       the same form over the axes with a finite 1 / d; an axis without one only asks that the origin is not
//                       strictly outside the slab, !(lo - o > 0) && !(hi - o < 0), which is what every accepting run of the exact
//                       sequence implies (an entry of +inf or an exit of -inf always rejects) and is monotone in the box as well.
// The order of visits does not matter: at a node the first accepted child is entered and the others are pushed as 4-byte references.
//
// The stack (4-byte entries), the node decode and the children's boxes are bvh_walk.hip.h's; the step that enters every accepted child
// is its walk_enter_all, written out here.
//
// The list (LIST): the lane's own output row hits[i K .. i K + K) IS the list -- a lane re-reads only what it wrote itself --, kept sorted
// by insertion; the number held and the K-th key stay in registers, so a hit that does not beat a full list costs one comparison and no
// memory.  No dynamically indexed private array (it would live in scratch).  The empty slots are filled when the ray retires.
#pragma once
#include "bvh_walk.hip.h"

namespace gnxr {

struct AllHitsArrays {
    const float4 *rays;   // gnxr_ray i = rays[2 i] (o.xyz, tmax), rays[2 i + 1] (d.xyz, pad)
    float4 *hits;         // K per ray: (t, prim, b1, b2); nullptr when K == 0
    int *counts;          // per ray
    int K;
};

// the ray as the node tests see it
struct AllHitsRay {
    V3 ro, inv;
    float tmax;
    int neg[3];
    bool flagged;       // some 1 / d is not finite
    bool fin[3];        // per axis: 1 / d is finite
};

// May anything under the box [lo, hi] be a hit?  A superset of slab_test (see the head of the file); never the deciding test.
GX_DEV bool ah_enter(const AllHitsRay &r, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const float k = 1 + 2 * GX_GAMMA(3);
    const float nx = r.neg[0] ? hix : lox, fx = r.neg[0] ? lox : hix;
    const float ny = r.neg[1] ? hiy : loy, fy = r.neg[1] ? loy : hiy;
    const float nz = r.neg[2] ? hiz : loz, fz = r.neg[2] ? loz : hiz;
    float ex = (nx - r.ro.x) * r.inv.x, ey = (ny - r.ro.y) * r.inv.y, ez = (nz - r.ro.z) * r.inv.z;
    float xx = (fx - r.ro.x) * r.inv.x, xy = (fy - r.ro.y) * r.inv.y, xz = (fz - r.ro.z) * r.inv.z;
    bool inside = true;
    if (r.flagged) {
        if (!r.fin[0]) { ex = -GX_INF; xx = GX_INF; inside = inside && !(lox - r.ro.x > 0.f) && !(hix - r.ro.x < 0.f); }
        if (!r.fin[1]) { ey = -GX_INF; xy = GX_INF; inside = inside && !(loy - r.ro.y > 0.f) && !(hiy - r.ro.y < 0.f); }
        if (!r.fin[2]) { ez = -GX_INF; xz = GX_INF; inside = inside && !(loz - r.ro.z > 0.f) && !(hiz - r.ro.z < 0.f); }
    }
    const float e = fmaxf(fmaxf(ex, ey), ez);
    const float x = fminf(fminf(xx, xy), xz) * k;
    return inside && e <= x && e < r.tmax && x > 0.f;
}

// The list of one ray: its output row, sorted by (t, prim); `held` entries, and the K-th key once it is full.
struct AllHitsList {
    float4 *row;
    int K, held;
    float kt;
    int kp;
    GX_DEV void insert(float t, int prim, float b1, float b2) {
        if (held == K && !(t < kt || (t == kt && prim < kp))) return;
        int j = held < K ? held : K - 1;   // a full list drops its last entry
        while (j > 0) {
            const float4 e = row[j - 1];
            if (e.x < t || (e.x == t && __float_as_int(e.y) < prim)) break;
            row[j] = e;
            --j;
        }
        row[j] = make_float4(t, __int_as_float(prim), b1, b2);
        if (held < K) ++held;
        if (held == K) { const float4 l = row[K - 1]; kt = l.x; kp = __float_as_int(l.y); }
    }
};

// WIDE: the 4-wide tree from sc.root4; else the binary tree from node 0.  LIST: K > 0 (else the count alone; no list memory is touched).
// COUNT: nodes visited, own-box tests and triangle tests of the whole launch are added to work[0 .. 3) (the measurement's instantiation;
// never the timed path).
template <bool WIDE, bool LIST, bool COUNT>
static __global__ void __launch_bounds__(kBlock) k_all_hits(DScene sc, AllHitsArrays qa, long long n, int lds_entries, int entries, int *spill, unsigned long long *work) {
    extern __shared__ int ah_stack_lds[];
    WalkStack<int> stack;   // of child references
    stack.init(ah_stack_lds, spill, lds_entries, entries);
    unsigned long long cntNodes = 0, cntBoxes = 0, cntTris = 0;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += stack.threads) {
        const float4 r0 = qa.rays[2 * i], r1 = qa.rays[2 * i + 1];
        const V3 ro(r0.x, r0.y, r0.z), rd(r1.x, r1.y, r1.z);
        const float tmax = r0.w;
        int count = 0;
        AllHitsList list;
        list.row = LIST ? qa.hits + i * (long long)qa.K : nullptr;
        list.K = qa.K; list.held = 0; list.kt = GX_INF; list.kp = 0x7fffffff;
        // no hits for a non-finite origin or direction, a NaN tmax or a zero direction: tri_test would say "hit" with a NaN t
        const bool valid = gx_finite(ro.x) && gx_finite(ro.y) && gx_finite(ro.z) && gx_finite(rd.x) && gx_finite(rd.y) && gx_finite(rd.z) && tmax == tmax &&
                           !(rd.x == 0.f && rd.y == 0.f && rd.z == 0.f);
        if (valid) {
            AllHitsRay ray;
            ray.ro = ro; ray.tmax = tmax;
            ray.inv = V3(1.f / rd.x, 1.f / rd.y, 1.f / rd.z);
            ray.neg[0] = ray.inv.x < 0; ray.neg[1] = ray.inv.y < 0; ray.neg[2] = ray.inv.z < 0;
            ray.fin[0] = gx_finite(ray.inv.x); ray.fin[1] = gx_finite(ray.inv.y); ray.fin[2] = gx_finite(ray.inv.z);
            ray.flagged = !(ray.fin[0] && ray.fin[1] && ray.fin[2]);
            const RayShear shear = ray_shear(rd);
            int sp = 0;
            int cur = WIDE ? sc.root4 : 0;
            while (true) {
                const WalkNode node = walk_decode<WIDE>(sc, cur);
                if (COUNT) cntNodes++;
                int next = kNode4Empty;   // the child to enter, or none
                if (node.leaf) {
                    for (int j = 0; j < node.count; ++j) {
                        V3 p0, p1, p2, lo, hi;
                        load_tri(sc.tris, node.first + j, &p0, &p1, &p2);
                        tri_own_box(p0, p1, p2, &lo, &hi);   // then the exact Bounds3::IntersectP on it
                        if (COUNT) cntBoxes++;
                        if (!slab_test(make_float4(lo.x, lo.y, lo.z, hi.x), make_float4(hi.y, hi.z, 0.f, 0.f), ro, ray.inv, ray.neg, tmax)) continue;
                        if (COUNT) cntTris++;
                        TriHit h;
                        if (!tri_test_sheared(p0, p1, p2, ro, shear, tmax, &h)) continue;
                        ++count;
                        if (LIST) list.insert(h.t, sc.tris[node.first + j].prim, h.b1, h.b2);
                    }
                } else {
                    int c[4]; bool e[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int s, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        c[s] = ref;
                        e[s] = !(WIDE && ref == kNode4Empty) && ah_enter(ray, lox, loy, loz, hix, hiy, hiz);
                    });
                    // walk_enter_all's ladder, written out: through the helper this kernel timed outside the parent's spread
                    if (WIDE) {
                        if (e[3]) { if (e[0] || e[1] || e[2]) stack.put(sp, c[3]); else next = c[3]; }
                        if (e[2]) { if (e[0] || e[1]) stack.put(sp, c[2]); else next = c[2]; }
                    }
                    if (e[1]) { if (e[0]) stack.put(sp, c[1]); else next = c[1]; }
                    if (e[0]) next = c[0];
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
            for (int j = list.held; j < list.K; ++j) list.row[j] = make_float4(GX_INF, __int_as_float(-1), 0.f, 0.f);
    }
    if (COUNT) {
        atomicAdd(&work[0], cntNodes);
        atomicAdd(&work[1], cntBoxes);
        atomicAdd(&work[2], cntTris);
    }
}

}  // namespace gnxr
