// bvh_walk.hip.h -- the mechanics the per-lane query walks share (k_closest_point, k_all_hits, k_near, k_sphere_cast, k_overlap_box, k_overlap_tri): the stack, the
// node decode, the children of an interior node with their boxes, and the descent step in its two orders (walk_enter_nearest,
// walk_enter_all) with the pop that follows it (walk_pop).  Nothing here decides a result: the callers supply the keys and the bounds --
// what a box is worth to a kernel, which children stay and what is tested at a leaf is that kernel's own.  DESIGN.md, "The walk the
// queries share", has the bound of the stack and why.
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// min / max by selection (the result is one of the arguments, never arithmetic), and a triangle's own box made of them
GX_DEV float sel_min(float x, float y) { return y < x ? y : x; }
GX_DEV float sel_max(float x, float y) { return y > x ? y : x; }
GX_DEV void tri_own_box(V3 a, V3 b, V3 c, V3 *lo, V3 *hi) {
    *lo = V3(sel_min(sel_min(a.x, b.x), c.x), sel_min(sel_min(a.y, b.y), c.y), sel_min(sel_min(a.z, b.z), c.z));
    *hi = V3(sel_max(sel_max(a.x, b.x), c.x), sel_max(sel_max(a.y, b.y), c.y), sel_max(sel_max(a.z, b.z), c.z));
}

// A stack entry of a deferred child: the reference alone (int: the order of visits does not matter) or (reference, key) (uint2: the key is
// tested again when the entry is popped)
GX_DEV void walk_entry(int *e, int ref, unsigned) { *e = ref; }
GX_DEV void walk_entry(uint2 *e, int ref, unsigned key) { *e = make_uint2((unsigned)ref, key); }
GX_DEV int walk_ref(int e) { return e; }
GX_DEV int walk_ref(uint2 e) { return (int)e.x; }
// is a popped entry still within `bound`?  An entry without a key always is.
GX_DEV bool walk_within(int, float) { return true; }
GX_DEV bool walk_within(uint2 e, float bound) { return !(__uint_as_float(e.y) > bound); }

// One lane's stack: entry `level`.  Levels below lds_entries are in the block's LDS as stack[level][lane], the others in a global spill,
// [level][thread] as well.  Entry is 4 bytes (int: bank == lane, conflict-free whatever level each lane is at) or 8 (uint2: lane l of a
// 32-lane half reads banks 2 l and 2 l + 1 of 64, so ds_read_b64 is conflict-free too; a ds_write_b64, banked modulo 32, costs two passes,
// where two 4-byte planes would cost two instructions instead).
template <typename Entry>
struct WalkStack {
    Entry *lds;        // this lane's column of the block's LDS stack (stride kBlock)
    Entry *spill;      // this thread's column of the global spill (stride `threads`)
    int lds_entries, entries;   // entries: LDS and spill levels together, the bound of the walk (never reached past: put() refuses)
    long long threads;          // of the grid: the stride of the spill and of the grid-stride loop
    GX_DEV void init(Entry *lds_base, Entry *spill_base, int lds_entries_, int entries_) {
        lds = lds_base + threadIdx.x;
        threads = (long long)gridDim.x * kBlock;
        spill = spill_base + (blockIdx.x * (long long)kBlock + threadIdx.x);
        lds_entries = lds_entries_;
        entries = entries_;
    }
    GX_DEV void put(int &sp, Entry e) {
        if (sp >= entries) return;
        if (sp < lds_entries) lds[sp * kBlock] = e;
        else spill[(long long)(sp - lds_entries) * threads] = e;
        ++sp;
    }
    GX_DEV void put_child(int &sp, int ref, unsigned key) {   // a deferred child as this stack's entry (walk_entry, below)
        Entry e;
        walk_entry(&e, ref, key);
        put(sp, e);
    }
    GX_DEV Entry get(int level) const { return level < lds_entries ? lds[level * kBlock] : spill[(long long)(level - lds_entries) * threads]; }
};

// What a reference says.  WIDE (the 4-wide tree, from DScene::root4): cur < 0 is a leaf and ~cur = first | count << 24, as in k_trace4.
// Binary (DScene::nodes, from node 0): the node's second dwordx4 holds the count (0: interior) and `first`, which is a leaf's first
// triangle and an interior node's second child.
struct WalkNode { bool leaf; int first, count; };
template <bool WIDE>
GX_DEV WalkNode walk_decode(const DScene &sc, int cur) {
    if (WIDE) {
        const unsigned code = (unsigned)~cur;
        return cur < 0 ? WalkNode{true, (int)(code & 0xffffffu), (int)(code >> 24)} : WalkNode{false, 0, 0};
    }
    const float4 n1 = sc.nodes[2 * cur + 1];
    const int count = (int)(__float_as_uint(n1.w) & 0xffffu);
    return {count > 0, __float_as_int(n1.z), count};
}

// The children of interior node `cur`: f(slot, ref, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) once per slot, slot a constant.  WIDE: four
// slots from one load of the DNode4's six SoA planes and its child dwordx4; a slot whose ref is kNode4Empty is absent (f decides what
// that means).  Binary: slots 0 and 1, the DNode children cur + 1 and `second` (WalkNode::first of cur).
template <bool WIDE, typename F>
GX_DEV void walk_children(const DScene &sc, int cur, int second, F f) {
    if (WIDE) {
        const float4 *nd = sc.nodes4 + 8 * (long long)cur;
        const float4 lox = nd[0], loy = nd[1], loz = nd[2], hix = nd[3], hiy = nd[4], hiz = nd[5], ch = nd[6];
        f(0, __float_as_int(ch.x), lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x);
        f(1, __float_as_int(ch.y), lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y);
        f(2, __float_as_int(ch.z), lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z);
        f(3, __float_as_int(ch.w), lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w);
    } else {
        const int c0 = cur + 1, c1 = second;
        const float4 a0 = sc.nodes[2 * c0], a1 = sc.nodes[2 * c0 + 1], b0 = sc.nodes[2 * c1], b1 = sc.nodes[2 * c1 + 1];
        f(0, c0, a0.x, a0.y, a0.z, a0.w, a1.x, a1.y);
        f(1, c1, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y);
    }
}

// ---- the descent step: which child is entered, which are deferred ----

// Keys of the child sort.  A child's key is the bits of its lower bound `lb`, a non-negative float the caller computed (a squared distance,
// an entry time): they order as the float does (a NaN, which only a box with a NaN bound gives, sorts behind +inf and is still entered).
// An absent child and one whose lb exceeds the caller's `bound` sort last, as kWalkDropped.
constexpr unsigned kWalkDropped = 0xffffffffu;
template <bool WIDE>
GX_DEV unsigned walk_key(int ref, float lb, float bound) { return ((WIDE && ref == kNode4Empty) || lb > bound) ? kWalkDropped : __float_as_uint(lb); }
GX_DEV void walk_sort2(unsigned &ka, int &ra, unsigned &kb, int &rb) {
    if (kb < ka) { const unsigned k = ka; ka = kb; kb = k; const int r = ra; ra = rb; rb = r; }
}

// Nearest first: the children r[] with keys k[] (slots 2 and 3 are read on the 4-wide tree only) are sorted by key (the five-exchange
// network), put(ref, key) defers those that are not dropped, farthest first, and the nearest is returned to be entered -- kNode4Empty
// when all are dropped.
template <bool WIDE, typename Put>
GX_DEV int walk_enter_nearest(const int (&r)[4], const unsigned (&k)[4], Put put) {
    int r0 = r[0], r1 = r[1];   // scalars for the sort: on the arrays' elements hipcc builds the exchanges from selects, 6 VGPRs more
    unsigned k0 = k[0], k1 = k[1];
    if (WIDE) {
        int r2 = r[2], r3 = r[3];
        unsigned k2 = k[2], k3 = k[3];
        walk_sort2(k0, r0, k1, r1); walk_sort2(k2, r2, k3, r3); walk_sort2(k0, r0, k2, r2); walk_sort2(k1, r1, k3, r3); walk_sort2(k1, r1, k2, r2);
        if (k3 != kWalkDropped) put(r3, k3);
        if (k2 != kWalkDropped) put(r2, k2);
    } else {
        walk_sort2(k0, r0, k1, r1);
    }
    if (k1 != kWalkDropped) put(r1, k1);
    return k0 != kWalkDropped ? r0 : kNode4Empty;
}

// Every child that stays (e[]), in slot order: the first is returned to be entered, put(ref) defers the others; kNode4Empty when none stays
template <bool WIDE, typename Put>
GX_DEV int walk_enter_all(const int (&r)[4], const bool (&e)[4], Put put) {
    int next = kNode4Empty;
    if (WIDE) {
        if (e[3]) { if (e[0] || e[1] || e[2]) put(r[3]); else next = r[3]; }
        if (e[2]) { if (e[0] || e[1]) put(r[2]); else next = r[2]; }
    }
    if (e[1]) { if (e[0]) put(r[1]); else next = r[1]; }
    if (e[0]) next = r[0];
    return next;
}

// After the step: `next` when a child is entered; else the topmost deferred entry that still_in(entry) keeps (the caller's bound may have
// shrunk since the push), and kNode4Empty when the stack runs empty -- the walk is over
template <typename Entry, typename StillIn>
GX_DEV int walk_pop(const WalkStack<Entry> &stack, int &sp, int next, StillIn still_in) {
    while (next == kNode4Empty && sp > 0) {
        const Entry e = stack.get(--sp);
        if (still_in(e)) next = walk_ref(e);
    }
    return next;
}

}  // namespace gnxr
