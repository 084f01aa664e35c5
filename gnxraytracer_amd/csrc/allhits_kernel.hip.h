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
// The stack holds at most (children - 1) entries per node of the path from the root: CompiledScene::stack4_need - 1 on the 4-wide tree,
// the depth on the binary one.  Its first lds_entries levels live in LDS as stack[level][lane] (bank == lane: conflict-free whatever level
// each lane is at), the levels above in a global spill, [level][thread] as well; put() refuses to write past the bound.
//
// The list (LIST): the lane's own output row hits[i K .. i K + K) IS the list -- a lane re-reads only what it wrote itself --, kept sorted
// by insertion; the number held and the K-th key stay in registers, so a hit that does not beat a full list costs one comparison and no
// memory.  No dynamically indexed private array (it would live in scratch).  The empty slots are filled when the ray retires.
#pragma once
#include "closest_kernel.hip.h"
#include "kernels.hip.h"

namespace gnxr {

struct AllHitsArrays {
    const float4 *rays;   // gnxr_ray i = rays[2 i] (o.xyz, tmax), rays[2 i + 1] (d.xyz, pad)
    float4 *hits;         // K per ray: (t, prim, b1, b2); nullptr when K == 0
    int *counts;          // per ray
    int K;
};

GX_DEV bool ah_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// One block's stack of child references: entry `level` of this lane.  Levels below lds_entries in LDS, the others in the global spill.
struct AllHitsStack {
    int *lds;          // this lane's column of the block's LDS stack (stride kBlock)
    int *spill;        // this thread's column of the global spill (stride `threads`)
    int lds_entries, entries;   // entries: LDS and spill levels together, the bound of the walk (never reached past: put() refuses)
    long long threads;
    GX_DEV void put(int &sp, int ref) {
        if (sp >= entries) return;
        if (sp < lds_entries) lds[sp * kBlock] = ref;
        else spill[(long long)(sp - lds_entries) * threads] = ref;
        ++sp;
    }
    GX_DEV int get(int level) const { return level < lds_entries ? lds[level * kBlock] : spill[(long long)(level - lds_entries) * threads]; }
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
    AllHitsStack stack;
    stack.lds = ah_stack_lds + threadIdx.x;
    stack.threads = (long long)gridDim.x * kBlock;
    stack.spill = spill + (blockIdx.x * (long long)kBlock + threadIdx.x);
    stack.lds_entries = lds_entries;
    stack.entries = entries;
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
        const bool valid = ah_finite(ro.x) && ah_finite(ro.y) && ah_finite(ro.z) && ah_finite(rd.x) && ah_finite(rd.y) && ah_finite(rd.z) && tmax == tmax &&
                           !(rd.x == 0.f && rd.y == 0.f && rd.z == 0.f);
        if (valid) {
            AllHitsRay ray;
            ray.ro = ro; ray.tmax = tmax;
            ray.inv = V3(1.f / rd.x, 1.f / rd.y, 1.f / rd.z);
            ray.neg[0] = ray.inv.x < 0; ray.neg[1] = ray.inv.y < 0; ray.neg[2] = ray.inv.z < 0;
            ray.fin[0] = ah_finite(ray.inv.x); ray.fin[1] = ah_finite(ray.inv.y); ray.fin[2] = ah_finite(ray.inv.z);
            ray.flagged = !(ray.fin[0] && ray.fin[1] && ray.fin[2]);
            const RayShear shear = ray_shear(rd);
            int sp = 0;
            int cur = WIDE ? sc.root4 : 0;
            while (true) {
                bool leaf;
                int first = 0, nprims = 0;
                if (WIDE) {
                    leaf = cur < 0;
                    if (leaf) { const unsigned code = (unsigned)~cur; first = (int)(code & 0xffffffu); nprims = (int)(code >> 24); }
                } else {
                    const float4 n1 = sc.nodes[2 * cur + 1];
                    const unsigned meta = __float_as_uint(n1.w);
                    nprims = (int)(meta & 0xffffu);
                    leaf = nprims > 0;
                    first = __float_as_int(n1.z);   // a leaf's first triangle, an interior node's second child
                }
                if (COUNT) cntNodes++;
                int next = kNode4Empty;   // the child to enter, or none
                if (leaf) {
                    for (int j = 0; j < nprims; ++j) {
                        V3 p0, p1, p2;
                        load_tri(sc.tris, first + j, &p0, &p1, &p2);
                        // the triangle's own box: min / max of its vertices by selection, then the exact Bounds3::IntersectP
                        const float4 b0 = make_float4(cp_min(cp_min(p0.x, p1.x), p2.x), cp_min(cp_min(p0.y, p1.y), p2.y), cp_min(cp_min(p0.z, p1.z), p2.z),
                                                      cp_max(cp_max(p0.x, p1.x), p2.x));
                        const float4 b1 = make_float4(cp_max(cp_max(p0.y, p1.y), p2.y), cp_max(cp_max(p0.z, p1.z), p2.z), 0.f, 0.f);
                        if (COUNT) cntBoxes++;
                        if (!slab_test(b0, b1, ro, ray.inv, ray.neg, tmax)) continue;
                        if (COUNT) cntTris++;
                        TriHit h;
                        if (!tri_test_sheared(p0, p1, p2, ro, shear, tmax, &h)) continue;
                        ++count;
                        if (LIST) list.insert(h.t, sc.tris[first + j].prim, h.b1, h.b2);
                    }
                } else if (WIDE) {
                    const float4 *nd = sc.nodes4 + 8 * (long long)cur;
                    const float4 lox = nd[0], loy = nd[1], loz = nd[2], hix = nd[3], hiy = nd[4], hiz = nd[5];
                    const float4 ch = nd[6];
                    const int c0 = __float_as_int(ch.x), c1 = __float_as_int(ch.y), c2 = __float_as_int(ch.z), c3 = __float_as_int(ch.w);
                    const bool e0 = c0 != kNode4Empty && ah_enter(ray, lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x);
                    const bool e1 = c1 != kNode4Empty && ah_enter(ray, lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y);
                    const bool e2 = c2 != kNode4Empty && ah_enter(ray, lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z);
                    const bool e3 = c3 != kNode4Empty && ah_enter(ray, lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w);
                    if (e3) { if (e0 || e1 || e2) stack.put(sp, c3); else next = c3; }
                    if (e2) { if (e0 || e1) stack.put(sp, c2); else next = c2; }
                    if (e1) { if (e0) stack.put(sp, c1); else next = c1; }
                    if (e0) next = c0;
                } else {
                    const int c0 = cur + 1, c1 = first;
                    const float4 a0 = sc.nodes[2 * c0], a1 = sc.nodes[2 * c0 + 1], d0 = sc.nodes[2 * c1], d1 = sc.nodes[2 * c1 + 1];
                    const bool e0 = ah_enter(ray, a0.x, a0.y, a0.z, a0.w, a1.x, a1.y), e1 = ah_enter(ray, d0.x, d0.y, d0.z, d0.w, d1.x, d1.y);
                    if (e1) { if (e0) stack.put(sp, c1); else next = c1; }
                    if (e0) next = c0;
                }
                if (next == kNode4Empty) {
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

// a scene without triangles: counts of 0 and empty slots
static __global__ void __launch_bounds__(kBlock) k_all_hits_none(float4 *hits, int *counts, long long n, int K) {
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        counts[i] = 0;
        for (int j = 0; j < K; ++j) hits[i * (long long)K + j] = make_float4(GX_INF, __int_as_float(-1), 0.f, 0.f);
    }
}

}  // namespace gnxr
