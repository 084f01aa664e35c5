// wide_collapse.h -- which binary nodes become the children of a DNode4: the arithmetic and the decisions that the host collapse
// (scene_compile.cpp) and the device rebuild (rebuild_kernel.hip.h) must make identically, as host-and-device inline functions.
//
// A DNode4 rooted at the binary interior node N has as children a CUT of the subtree under N: 2 to 4 binary nodes that together cover
// N's leaves exactly once.  The cuts minimise the summed surface area of all DNode4 roots (the expected number of 4-wide node steps of a
// random ray, up to a constant), by a bottom-up dynamic programme over the binary tree:
//     C(X)    = area(X) + min over k in 2..4 of T(X, k)          X interior: the cost of the 4-wide subtree rooted at X
//     T(X, 1) = 0 for a leaf, C(X) otherwise                     X is one child slot
//     T(X, k) = min over i + j = k of T(A, i) + T(B, j)          X's children A, B share k slots (k >= 2: X interior)
// Ties go to the smallest k, then the smallest i (every comparison is a strict <, candidates in ascending order).  The sums are single
// fp32 additions of two stored values, so host and device agree bit for bit as long as neither contracts a * b + c (both builds use
// -ffp-contract=off).
//
// Slots.  A cut of four is balanced, ((s0 s1)(s2 s3)), or a chain, (s0 (s1 (s2 s3))); mirror images are the same shape with other
// slots, and a cut of three or two is the balanced shape with slots 1 and / or 3 empty.  The order in which BVHAccel::Intersect reaches
// the members of a cut is then fixed per ray octant by three binary decisions -- together with the shape a 4-bit code:
//     balanced  0 | h << 2 | a << 1 | b    h: the half (s2 s3) comes first; a / b: the half visited first / second is swapped
//     chain     8 | l << 2 | m << 1 | p    l: s0 comes last; m: s1 comes after (s2 s3); p: s3 comes before s2
#pragma once
#include <stdint.h>

#include "gnxr_device_types.h"

#if defined(__HIPCC__)
#define GX_WIDE_HD __host__ __device__ inline
#else
#define GX_WIDE_HD inline
#endif

namespace gnxr {

// T(X, 1..4) of a binary node
struct WideCost { float t[4]; };
static_assert(sizeof(WideCost) == 16, "WideCost is read as one dwordx4");

GX_WIDE_HD bool wide_is_leaf(const DNode &n) { return (n.meta & 0xffffu) != 0; }
GX_WIDE_HD int wide_axis(const DNode &n) { return (int)(n.meta >> 16) & 3; }

// the decisions of an interior node: the k of C(X) and, for k = 3 and k = 4, the slots its first child gets (k = 2: always 1)
GX_WIDE_HD int wide_best_k(uint8_t choice) { return 2 + (choice & 3); }
GX_WIDE_HD int wide_split(uint8_t choice, int k) { return k == 2 ? 1 : (k == 3 ? 1 + ((choice >> 2) & 1) : 1 + ((choice >> 3) & 3)); }

GX_WIDE_HD float wide_area(const DNode &n) {
    const float dx = n.hi0 - n.lo[0], dy = n.hi1 - n.lo[1], dz = n.hi2 - n.lo[2];
    return 2.f * ((dx * dy + dy * dz) + dz * dx);
}

GX_WIDE_HD WideCost wide_cost_leaf() {
    WideCost c;
    c.t[0] = 0.f; c.t[1] = c.t[2] = c.t[3] = __builtin_inff();
    return c;
}
// X interior with children A, B: T(X, .) into *out, returns X's decisions
GX_WIDE_HD uint8_t wide_cost_interior(const DNode &X, const WideCost &a, const WideCost &b, WideCost *out) {
    const float t2 = a.t[0] + b.t[0];
    float t3 = a.t[0] + b.t[1];
    int i3 = 1;
    { const float c = a.t[1] + b.t[0]; if (c < t3) { t3 = c; i3 = 2; } }
    float t4 = a.t[0] + b.t[2];
    int i4 = 1;
    { const float c = a.t[1] + b.t[1]; if (c < t4) { t4 = c; i4 = 2; } }
    { const float c = a.t[2] + b.t[0]; if (c < t4) { t4 = c; i4 = 3; } }
    float m = t2;
    int k = 2;
    if (t3 < m) { m = t3; k = 3; }
    if (t4 < m) { m = t4; k = 4; }
    out->t[0] = wide_area(X) + m; out->t[1] = t2; out->t[2] = t3; out->t[3] = t4;
    return (uint8_t)((k - 2) | ((i3 - 1) << 2) | ((i4 - 1) << 3));
}

// the four slots of a code, nearest first, 2 bits each from bit 0
GX_WIDE_HD unsigned wide_order_byte(unsigned code) {
    unsigned o0, o1, o2, o3;
    if (!(code & 8u)) {
        const unsigned base0 = (code & 4u) ? 2u : 0u, base1 = 2u - base0, sw0 = (code >> 1) & 1u, sw1 = code & 1u;
        o0 = base0 + sw0; o1 = base0 + 1u - sw0; o2 = base1 + sw1; o3 = base1 + 1u - sw1;
    } else {
        const unsigned p0 = (code & 1u) ? 3u : 2u, p1 = 5u - p0;
        const unsigned r0 = (code & 2u) ? p0 : 1u, r1 = (code & 2u) ? p1 : p0, r2 = (code & 2u) ? 1u : p1;
        if (code & 4u) { o0 = r0; o1 = r1; o2 = r2; o3 = 0u; }
        else { o0 = 0u; o1 = r0; o2 = r1; o3 = r2; }
    }
    return o0 | (o1 << 2) | (o2 << 4) | (o3 << 6);
}

// The cut of the DNode4 rooted at interior binary node `bi` (bn: the tree in pre-order, first child at bi + 1; choice: per node, of
// wide_cost_interior): the binary node behind each slot (-1: empty), the per-octant codes and the order table they stand for.
struct WideCut {
    int slot[4];
    int n;                        // slots used
    uint32_t codes;               // 4 bits per octant
    uint32_t order_lo, order_hi;  // wide_order_byte(code) per octant
};
GX_WIDE_HD WideCut wide_cut(const DNode *bn, const uint8_t *choice, int bi) {
    WideCut c;
    c.slot[0] = c.slot[1] = c.slot[2] = c.slot[3] = -1;
    const DNode N = bn[bi];
    const int A = bi + 1, B = N.offset;
    const int k = wide_best_k(choice[bi]), i = wide_split(choice[bi], k), j = k - i;
    c.n = k;
    // per decision: the axis whose direction sign decides it, and whether a POSITIVE direction already sets the bit
    int ax0 = wide_axis(N), ax1 = 0, ax2 = 0, flip0 = 0, flip1 = 0;
    unsigned shape = 0u;
    if (i <= 2 && j <= 2) {
        if (i == 1) c.slot[0] = A; else { c.slot[0] = A + 1; c.slot[1] = bn[A].offset; ax1 = wide_axis(bn[A]); }
        if (j == 1) c.slot[2] = B; else { c.slot[2] = B + 1; c.slot[3] = bn[B].offset; ax2 = wide_axis(bn[B]); }
    } else {
        shape = 8u;
        const int M = i == 1 ? B : A;              // the child that takes three slots
        c.slot[0] = i == 1 ? A : B; flip0 = i == 1 ? 0 : 1;
        const DNode m = bn[M];
        const int i2 = wide_split(choice[M], 3);
        const int P = i2 == 1 ? m.offset : M + 1;  // the child of M that takes two
        c.slot[1] = i2 == 1 ? M + 1 : m.offset; flip1 = i2 == 1 ? 0 : 1;
        ax1 = wide_axis(m);
        c.slot[2] = P + 1; c.slot[3] = bn[P].offset; ax2 = wide_axis(bn[P]);
    }
    c.codes = 0u; c.order_lo = 0u; c.order_hi = 0u;
    for (int oct = 0; oct < 8; ++oct) {
        const int n0 = (oct >> ax0) & 1, n1 = (oct >> ax1) & 1, n2 = (oct >> ax2) & 1;
        unsigned code;
        if (!shape) {
            // the near child of N first (dirIsNeg[axis of N]); inside each half the near grandchild first
            const int h = n0, a = h ? n2 : n1, b = h ? n1 : n2;
            code = (unsigned)((h << 2) | (a << 1) | b);
        } else code = 8u | (unsigned)(((n0 ^ flip0) << 2) | ((n1 ^ flip1) << 1) | n2);
        c.codes |= code << (4 * oct);
        const uint32_t byte = wide_order_byte(code);
        if (oct < 4) c.order_lo |= byte << (8 * oct); else c.order_hi |= byte << (8 * (oct - 4));
    }
    return c;
}

}  // namespace gnxr
