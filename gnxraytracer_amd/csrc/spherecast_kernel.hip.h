// spherecast_kernel.hip.h -- sphere casts on caller-supplied device memory (gnxr_sphere_cast_device): a ball of radius r whose centre
// moves from o along d; when does it first touch the mesh, and on which triangle.  The definition, operation by operation, is in
// include/gnxr.h ("Sphere casts"); the proof that the walk below prunes exactly is in DESIGN.md.
//
// One cast per lane, grid-stride, nearest-first like k_closest_point, but the bound is a TIME.  At a node the grown-box test (the monotone
// slab test on the child's box grown by r) gives each child an entry time tb; a child is dropped iff a static axis is outside, tb > tx or
// tb > best; the nearest survivor is entered and the others go onto the stack, farthest first, as (child reference, tb) pairs; a popped
// entry is tested against the current best again before its memory is touched.  A triangle's time is t = max(ta, tb(its own box)) with ta
// the analytic first contact, so tb of every enclosing box is a lower bound IN FP32 of t (growing by r, subtracting o and multiplying
// by a fixed 1 / d round monotonically), `tb > best` never drops the winner and `tb == best` is entered because a smaller authoring index
// may tie.  No epsilon anywhere.
//
// The stack (8-byte entries), the node decode, the children's boxes, the child sort with its keys (tb >= 0, so its bits order as the
// float does) and the pop are bvh_walk.hip.h's; closest_on_triangle is closest_kernel.hip.h's.  Casts run in caller order: QueryBinning takes
// 16-byte records.
#pragma once
#include "closest_kernel.hip.h"

namespace gnxr {

// gnxr_sphere_cast / gnxr_closest_point as the kernel moves them: two dwordx4 each
struct SphereCastArrays {
    const float4 *casts;   // cast i = casts[2 i] (o.xyz, radius), casts[2 i + 1] (d.xyz, tmax)
    float4 *out;           // 2 per cast: (prim, t, p.x, p.y), (p.z, b1, b2, feature)
};

// the cast as the box tests see it
struct SphereCast {
    V3 o, d, inv;
    float r, r2, dd;
    bool fin[3];   // per axis: 1 / d is finite (the axis moves)
};

// Step 1 on the box [lo, hi]: false = nothing under it can hit before `bound`; else *tb = the entry time, >= 0.
GX_DEV bool sc_box(const SphereCast &s, float lox, float loy, float loz, float hix, float hiy, float hiz, float bound, float *tb) {
    const float glx = lox - s.r, gly = loy - s.r, glz = loz - s.r, ghx = hix + s.r, ghy = hiy + s.r, ghz = hiz + s.r;
    float e = 0.f, x = GX_INF;
    bool in = true;
    if (s.fin[0]) {
        const bool neg = s.inv.x < 0.f;
        e = sel_max(e, ((neg ? ghx : glx) - s.o.x) * s.inv.x);
        x = sel_min(x, ((neg ? glx : ghx) - s.o.x) * s.inv.x);
    } else {
        in = in && glx <= s.o.x && s.o.x <= ghx;
    }
    if (s.fin[1]) {
        const bool neg = s.inv.y < 0.f;
        e = sel_max(e, ((neg ? ghy : gly) - s.o.y) * s.inv.y);
        x = sel_min(x, ((neg ? gly : ghy) - s.o.y) * s.inv.y);
    } else {
        in = in && gly <= s.o.y && s.o.y <= ghy;
    }
    if (s.fin[2]) {
        const bool neg = s.inv.z < 0.f;
        e = sel_max(e, ((neg ? ghz : glz) - s.o.z) * s.inv.z);
        x = sel_min(x, ((neg ? glz : ghz) - s.o.z) * s.inv.z);
    } else {
        in = in && glz <= s.o.z && s.o.z <= ghz;
    }
    *tb = e;
    return in && e <= x && e <= bound;
}

// a root of step 2 counts iff 0 <= t < +inf (a NaN fails); ta keeps the smallest
GX_DEV void sc_take(float t, float *ta) {
    if (t >= 0.f && t < GX_INF) *ta = sel_min(*ta, t);
}

// the ray o + t d against the cylinder of radius r around the line p0 + s (p1 - p0), accepted iff the axial parameter is within [0, 1]
GX_DEV void sc_edge(const SphereCast &s, V3 p0, V3 p1, float *ta) {
    const V3 e = p1 - p0, m = s.o - p0;
    const float me = cp_dot(m, e), de = cp_dot(s.d, e), ee = cp_dot(e, e), md = cp_dot(m, s.d), mm = cp_dot(m, m);
    const float A = ee * s.dd - de * de;
    if (!(A > 0.f)) return;
    const float C = ee * (mm - s.r2) - me * me;
    const float B = ee * md - de * me;
    const float disc = B * B - A * C;
    if (!(disc >= 0.f)) return;
    const float t = (-B - gx_sqrt(disc)) / A;
    const float w = me + t * de;
    if (w >= 0.f && w <= ee) sc_take(t, ta);
}

// the ray against the sphere of radius r around v
GX_DEV void sc_vertex(const SphereCast &s, V3 v, float *ta) {
    const V3 m = s.o - v;
    const float b = cp_dot(m, s.d), c = cp_dot(m, m) - s.r2;
    const float disc = b * b - s.dd * c;
    if (!(s.dd > 0.f) || !(disc >= 0.f)) return;
    sc_take((-b - gx_sqrt(disc)) / s.dd, ta);
}

// Step 2: the analytic time of first contact with triangle (a, b, c); +inf: none
GX_DEV float sc_analytic(const SphereCast &s, V3 a, V3 b, V3 c) {
    ClosestOnTri unused;
    if (closest_on_triangle(a, b, c, s.o, &unused) <= s.r2) return 0.f;   // the ball starts in contact
    float ta = GX_INF;
    const V3 ab = b - a, ac = c - a;
    const V3 n(ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x);
    const float nn = cp_dot(n, n);
    if (nn > 0.f) {   // the face: the plane offset by r towards o
        const float len = gx_sqrt(nn), sd = cp_dot(n, s.o - a), dn = cp_dot(n, s.d);
        const float h = s.r * len;
        const float tf = ((sd < 0.f ? -h : h) - sd) / dn;
        if (tf >= 0.f && tf < GX_INF) {
            ClosestOnTri at;
            closest_on_triangle(a, b, c, s.o + tf * s.d, &at);
            if (at.feature == 0) ta = tf;
        }
    }
    sc_edge(s, a, b, &ta);
    sc_edge(s, a, c, &ta);
    sc_edge(s, b, c, &ta);
    sc_vertex(s, a, &ta);
    sc_vertex(s, b, &ta);
    sc_vertex(s, c, &ta);
    return ta;
}

// best = (t, authoring index) in lexicographic order; it starts at (tmax, INT_MAX), which makes `t <= tmax` and the tie rule one test
struct SphereCastBest {
    float t;
    int prim;
    int leaf;   // the winner's leaf-order index (-1: none yet)
};

// WIDE: the 4-wide tree from sc.root4; else the binary tree from node 0.  COUNT: nodes visited and triangles tested (step 2 reached) of
// the whole launch are added to work[0], work[1] (the measurement's instantiation; never the timed path).  A stack entry is (child
// reference, bits of tb).
template <bool WIDE, bool COUNT>
static __global__ void __launch_bounds__(kBlock) k_sphere_cast(DScene sc, SphereCastArrays qa, long long n, int lds_entries, int entries, uint2 *spill,
                                                               unsigned long long *work) {
    extern __shared__ uint2 sc_stack_lds[];
    WalkStack<uint2> stack;
    stack.init(sc_stack_lds, spill, lds_entries, entries);
    unsigned long long cntNodes = 0, cntTris = 0;
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += stack.threads) {
        const float4 c0 = qa.casts[2 * i], c1 = qa.casts[2 * i + 1];
        SphereCast s;
        s.o = V3(c0.x, c0.y, c0.z); s.d = V3(c1.x, c1.y, c1.z);
        s.r = c0.w; s.r2 = c0.w * c0.w;
        const float tmax = c1.w;
        SphereCastBest best = {tmax, 0x7fffffff, -1};
        // a NaN radius or tmax fails its test; an infinite o or d hits nothing (gnxr.h, step 0)
        const bool valid = s.r >= 0.f && tmax >= 0.f && gx_finite(s.o.x) && gx_finite(s.o.y) && gx_finite(s.o.z) && gx_finite(s.d.x) && gx_finite(s.d.y) && gx_finite(s.d.z);
        if (valid) {
            s.inv = V3(1.f / s.d.x, 1.f / s.d.y, 1.f / s.d.z);
            s.fin[0] = gx_finite(s.inv.x); s.fin[1] = gx_finite(s.inv.y); s.fin[2] = gx_finite(s.inv.z);
            s.dd = cp_dot(s.d, s.d);
            int sp = 0;
            int cur = WIDE ? sc.root4 : 0;
            while (true) {
                const WalkNode node = walk_decode<WIDE>(sc, cur);
                if (COUNT) cntNodes++;
                int next = kNode4Empty;   // the child to enter, or none
                if (node.leaf) {
                    for (int j = 0; j < node.count; ++j) {
                        V3 a, b, c, lo, hi;
                        load_tri(sc.tris, node.first + j, &a, &b, &c);
                        tri_own_box(a, b, c, &lo, &hi);
                        float tb;
                        // step 1 with the cast's tmax; a triangle with tb > best cannot win (t >= tb), so step 2 is not run for it
                        if (!sc_box(s, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, tmax, &tb) || tb > best.t) continue;
                        if (COUNT) cntTris++;
                        const float ta = sc_analytic(s, a, b, c);
                        if (!(ta < GX_INF)) continue;
                        const float t = sel_max(tb, ta);
                        const int prim = sc.tris[node.first + j].prim;
                        if (t < best.t || (t == best.t && prim < best.prim)) { best.t = t; best.prim = prim; best.leaf = node.first + j; }
                    }
                } else {
                    int r[4]; unsigned k[4];   // slots 2 and 3 exist on the 4-wide tree only
                    walk_children<WIDE>(sc, cur, node.first, [&](int slot, int ref, float lox, float loy, float loz, float hix, float hiy, float hiz) __attribute__((always_inline)) {
                        float tb;
                        const bool in = sc_box(s, lox, loy, loz, hix, hiy, hiz, best.t, &tb);
                        r[slot] = ref;
                        k[slot] = in ? walk_key<WIDE>(ref, tb, best.t) : kWalkDropped;
                    });
                    next = walk_enter_nearest<WIDE>(r, k, [&](int ref, unsigned key) __attribute__((always_inline)) { stack.put_child(sp, ref, key); });
                }
                next = walk_pop(stack, sp, next, [&](uint2 e) __attribute__((always_inline)) { return walk_within(e, best.t); });   // the best may have shrunk since the push
                if (next == kNode4Empty) break;
                cur = next;
            }
        }
        float4 o0 = make_float4(__int_as_float(-1), GX_INF, 0.f, 0.f), o1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (best.leaf >= 0) {
            V3 a, b, c;
            load_tri(sc.tris, best.leaf, &a, &b, &c);
            ClosestOnTri r;
            closest_on_triangle(a, b, c, s.o + best.t * s.d, &r);
            o0 = make_float4(__int_as_float(best.prim), best.t, r.p.x, r.p.y);
            o1 = make_float4(r.p.z, r.b1, r.b2, __int_as_float(r.feature));
        }
        qa.out[2 * i] = o0;
        qa.out[2 * i + 1] = o1;
    }
    if (COUNT) {
        atomicAdd(&work[0], cntNodes);
        atomicAdd(&work[1], cntTris);
    }
}

}  // namespace gnxr
