// trace4_kernel.hip.h -- k_trace4: the 4-wide BVH traversal stage (BVHAccel::Intersect / IntersectP, accelerator/BVHAccel.cpp:653-729)
// for every ray a path vertex produces (continuation: closest hit; shadow: any hit; MIS: closest hit), second generation.
//
// Same contract and the same visiting order as k_trace<*, WIDE = true> (trace_kernel.hip.h), whose wave statistics
// (tests/dev_stats.py, -DGX_TRACE_STATS) showed where the VALU issue slots went: node steps 56 % (at 69 % of the lanes), triangle
// tests 24 % (29 %), per-ray set-up 17 % -- the set-up (six IEEE divisions: 1 / d, the shear of the watertight test) ran whenever ANY
// lane was idle, for ~11 of 64 lanes at a time.  What changed:
//   * set-up in batches of 64 through LDS: when a wave's ready queue is empty ALL its lanes set one ray up each (lanes that are in
//     the middle of a traversal included -- their state is untouched) and park the 11-dword records in LDS; an idle lane then just
//     pops a record.  The divisions run with every lane on, and the wave stalls on the three dependent loads of a ray once per 64
//     rays instead of once per refill;
//   * node step: for rays whose 1 / d is finite the three slab intervals of a child are merged with v_max3 / v_min3 and ONE
//     interval test (equivalent to Bounds3::IntersectP's pairwise tests, Geometry.h:1380-1406, whenever no product is NaN -- shown in
//     DESIGN.md section 4; a ray with a zero direction component can produce 0 * inf and takes the reference's exact sequence);
//   * the hit children are put in visiting order by one LDS table lookup (the three bits that fix a node's visiting order for the
//     ray's octant x hit mask -> compacted slot list) instead of a four-step select / push chain;
//   * the breadth-first top 64 nodes of the tree are read from an LDS copy: the kernel turned out to be bound by the rate at which a
//     CU's vector-memory path takes per-lane gathers (~1 lane per clock: 8 dwordx4 per node visit), not by VALU issue or by cache
//     misses, and 55 % of all node visits go to those 64 nodes;
//   * the traversal stack is LDS-only when the tree's worst case fits (template SPILL = false): no address-space branch per push / pop;
//   * node addresses are a uniform base + 32-bit offsets.
// The work list of a render launch is [n_closest continuation rays | n_nee NEE vertices] (TraceWork): ONE item per vertex.  A batch of vertex items
// sets the shadow rays up and parks them; the lanes whose record also has a MIS ray (flags bit 1) remember it in a spare bit of `pk`, the pool
// stays on the batch, and when the ready queue next runs empty -- before the pool moves on -- those lanes re-read their queue entries, load the
// MIS records and park the MIS rays as a batch of their own: never more than 64 records in the queue, no register, no LDS.  (Until this
// change a vertex was two items, and the MIS items formed a range of their own at the end of the list: with one small light a few percent
// of them held a ray; the others cost a queue read, three record gathers and a near-empty set-up batch each.)
// What the scheme costs: every batch of vertex items that holds at least one MIS lane pays a second wave-wide set-up (two ballots, a second
// read of q_nee by the owing lanes, a fence), and only after its shadow rays have all been drawn from the queue -- where most vertices have
// both rays that doubles the set-up batches of the NEE range (the parent's MIS batches were full ones there); and the ballot over `pk` that
// finds owing lanes runs at every refill that finds the queue empty, in the continuation range too.  Measured: profiles/README.md.
// Light estimates inside the launch (TraceWork::nee_in_trace): a set-up batch of the NEE range also looks, lane by lane, at the vertex items this
// wave set up kNeeLag = 128 items earlier in the chunk it owns.  retire_ray marks a traced ray in bit 1 of its result byte; a vertex whose rays
// are all back gets L += beta * Ld right there (nee_apply, the function k_nee_combine calls) and byte 3 of its word set, and k_nee_combine, which
// still runs after the launch, adds the others: the last 128 items of every chunk, the 128- and 64-item chunks of the tail, the vertices with
// a ray still under way.  Every lane is on in a set-up batch and the wave waits for dependent loads there anyway; the three loads of the
// lagging vertex (queue entry, word, records) are issued between the set-up's own.  An item has one owner and its rays are only ever taken by
// lanes of the wave that parked them, so nobody else touches the vertex's word or its L during the launch; a workgroup-scope fence before the
// word is read makes the wave's own retire stores visible (same CU, same L1).  Measured: profiles/README.md.
// Q selects where the rays come from and where results go: the render's path records (kT4Render), or caller-supplied rays of a batched
// query (kT4QueryClosest / kT4QueryAny, query_kernel.hip.h).  The walk between the two is the same code.
#pragma once
#include "kernels.hip.h"
#include "query_kernel.hip.h"
#include "wide_collapse.h"

namespace gnxr {

// Hit children in visiting order.  The order byte of a node for one ray octant (4 x 2-bit child slots, nearest first) is one of 16
// patterns, named by the node's 4-bit code for that octant: the shape of the cut the children are (balanced or chain) and three near / far
// decisions (wide_collapse.h).  order_entry(code, hitMask) = the slots that are hit, nearest first, 2 bits each from bit 0 (their number
// is the mask's population count).  The 256 entries live in LDS (filled at kernel start).
GX_DEV unsigned order_entry(unsigned code, unsigned hm) {
    const unsigned byte = wide_order_byte(code);
    unsigned e = 0, n = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned slot = (byte >> (2 * i)) & 3u;
        if ((hm >> slot) & 1u) { e |= slot << (2u * n); ++n; }
    }
    return e;
}
constexpr int kOrderTableBytes = 256;
#ifndef GX_T4_CACHE
#define GX_T4_CACHE 64
#endif
constexpr int kTopCache = GX_T4_CACHE;   // DNode4[0 .. kTopCache) -- the breadth-first top of the tree -- are served from LDS
// Hot leaves: the leaves the cached nodes reference (in a room, the walls: large triangles that SAH isolates next to the root, and where
// nearly every ray ends) are served from LDS too.  A hot reference keeps the count field of a leaf reference; its offset field is
// kHotBase + (box slot << 4) + triangle slot, from the top of the 24-bit range (a scene with that many triangles gets no hot table).
constexpr int kHotBytes = 768;           // 48 B per triangle + 32 B per leaf box: what five blocks per CU leave beside 11 stack levels
constexpr int kHotBase = 0x1000000 - 256;
static_assert(kHotBytes % 16 == 0 && kHotBytes / 48 <= 16 && kHotBytes / 80 <= 16, "triangle and box slots of a hot reference are 4 bits each");
constexpr int kRayRecDwords = 11;       // LDS record of a set-up ray: o.xyz tMax | 1/d.xyz Sx | Sy flags path  (+1 with spheres: hit code)
#ifndef GX_T4_RQ
#define GX_T4_RQ 64
#endif
constexpr int kRayQueue = GX_T4_RQ;      // set-up rays a wave parks in LDS per batch (32 frees LDS for 6 more stack levels but halves the set-up's lane use: slower)
constexpr int kRqStride = (kBlock / 64) * kRayQueue;   // dwords per record field per block
#ifndef GX_T4_NEE_LAG
#define GX_T4_NEE_LAG 128
#endif
constexpr int kNeeLag = GX_T4_NEE_LAG;   // a set-up batch adds the light estimates of the vertex items the wave set up this many items earlier (whole batches: the lagging items are behind the pool)
#ifndef GX_T4_NEE_TAIL
#define GX_T4_NEE_TAIL 0   // 1: a round over the last kNeeLag items of a chunk when it runs out (measured: more vertices in the kernel, no faster; profiles/README.md)
#endif
#ifndef GX_T4_NEE_BESIDE
#define GX_T4_NEE_BESIDE 0   // 1: the lagging vertex's sh_X / nbeta / L are loaded beside its word, not under the test of it
#endif
static_assert(kNeeLag >= 64 && kNeeLag % 64 == 0, "the lagging items must lie behind the batch that is being set up");
GX_DEV int trace4_lds_dwords_per_thread(bool sph) { return kRayRecDwords + (sph ? 1 : 0); }

// COUNT: count node steps / triangle tests / leaf re-tests.  SPH: the scene has spheres.  SPILL: the traversal stack may outgrow its LDS part.
// Q: the ray source / retire step (kT4Render: `pa` is the render's PathArrays; the query modes: `pa` is a QueryArrays, `w` has n_closest
// work items and nothing else, and the cursor / spill buffers belong to the call).
// Tuning switches (tools/build_variant.sh + tests/dev_ab.py; the A/B table is in profiles/README.md).  Defaults = the fastest measured:
// 5 waves per SIMD (96 VGPRs), scalar slab arithmetic (the packed-fp32 forms measured in round 2 -- 124 VGPRs, 4 waves -- are gone), 64-ray set-up batches, 64 cached nodes.
#ifndef GX_T4_WAVES
#define GX_T4_WAVES 5
#endif
#if GX_T4_WAVES > 0
#define GX_T4_BOUNDS __launch_bounds__(kBlock, GX_T4_WAVES)
#else
#define GX_T4_BOUNDS __launch_bounds__(kBlock)
#endif
template <bool COUNT, bool SPH, bool SPILL, int Q = kT4Render>
__global__ void GX_T4_BOUNDS k_trace4(DScene sc, typename Trace4Src<Q>::type pa, TraceWork w, unsigned int *cursor, Counters *ctr, int lds_entries, int *spill, int chunk, int n_top, int hot_bytes) {
    // LDS: [lds_entries * kBlock] stack columns | [(11 | 12) * kRqStride] ray records (SoA: field * kRqStride + wave * kRayQueue + slot) |
    //      [8 * kTopCache float4] top-of-tree nodes, SoA by plane (plane * kTopCache + node: conflict-free across nodes) | [kOrderTableBytes] order table |
    //      [kHotBytes] hot leaves (hot_bytes != 0): triangles as 3 float4 each from the front (.w of the first = the triangle's leaf-order
    //      index; a 48-byte stride puts up to 16 triangles on 16 different groups of four banks), leaf boxes as 2 float4 each from the back
    extern __shared__ int smem[];
    typedef __attribute__((address_space(3))) float lds_float;
    lds_int *const stk = (lds_int *)&smem[threadIdx.x];
    global_int *const spl = (global_int *)(spill + (size_t)blockIdx.x * kBlock + threadIdx.x);
    const int spillStride = (int)gridDim.x * kBlock;
    const int lane = __lane_id();
    lds_int *const rq = (lds_int *)&smem[lds_entries * kBlock + (threadIdx.x >> 6) * kRayQueue];   // this wave's records: rq[field * kRqStride + slot]
    trace_work_counts(w);
    const unsigned total = (unsigned)w.n_closest + (unsigned)w.n_nee;   // [continuation rays | NEE vertices]
    chunk = trace_chunk(total, chunk);
    const ChunkPlan plan = chunk_plan(total, (unsigned)chunk);
    const unsigned nWaves = gridDim.x * (kBlock / 64u), waveId = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    bool firstFetch = true;   // wave-uniform
#ifdef GX_TAIL_STAMP
    const unsigned tailFrom = total;   // the stamped point: the end of the work list
    bool tailSeen = false;             // wave-uniform: this wave has stamped it
    if (Q == kT4Render && waveId == 0 && lane == 0) atomicMin(&g_tail[2], (unsigned long long)wall_clock64());
#endif
    const DTri *__restrict__ tris = sc.tris;
    const char *__restrict__ nb = reinterpret_cast<const char *>(sc.nodes4);
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4v lds_f4;
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    lds_f4 *const topN = (lds_f4 *)&smem[lds_entries * kBlock + (kRayRecDwords + (SPH ? 1 : 0)) * kRqStride];
    lds_u8 *const lut = (lds_u8 *)(topN + 8 * kTopCache);
    lds_f4 *const hotT = (lds_f4 *)(lut + kOrderTableBytes);   // hot triangles upwards from here, hot leaf boxes downwards from hotT + kHotBytes / 16
    {   // fill the block's node cache and order table.  A vector-memory gather costs ~1 lane per clock per CU whatever it hits
        // (tools/probes/gather_probe.hip: 18 B/clk/CU for 16-byte gathers, L1-resident or not), and over half of all node visits go to
        // these few nodes (tests/dev_stats.py): from LDS they cost a ds_read instead.
        const f4v *gn = reinterpret_cast<const f4v *>(sc.nodes4);
        for (int i = threadIdx.x; i < n_top * 8; i += kBlock) topN[(i & 7) * kTopCache + (i >> 3)] = gn[i];
        if (threadIdx.x < kOrderTableBytes) lut[threadIdx.x] = (unsigned char)order_entry(threadIdx.x >> 4, threadIdx.x & 15u);
        if (hot_bytes) {   // block-uniform; only ever 0 or kHotBytes: the launch has reserved the region or it has not
            // the hot leaves: thread i looks at child slot i & 3 of cached node i >> 2.  A leaf needs 48 B per triangle and 32 B for its box
            // where phase B can ask for it; leaves are admitted in thread order -- a prefix sum over (triangles | boxes << 16), no atomics, the
            // same table in every block -- until the first one that does not fit whole: the sum runs over every leaf, so no later, smaller
            // leaf gets in behind it.  The live device tables are read at every launch: an edit needs nothing.
            const int node = threadIdx.x >> 2, slot = threadIdx.x & 3;
            int ref = -1;
            if (node < n_top) ref = reinterpret_cast<const int *>(sc.nodes4)[node * 32 + 24 + slot];
            const bool leaf = ref < -1;   // (kNode4Empty is positive)
            const int lr = ~ref, first = lr & 0xffffff, n = (lr >> 24) & 0x7f;
            const int box = (n > 1 || !sc.leaf1_from_verts) ? 1 : 0;
            unsigned incl = leaf ? (unsigned)n | ((unsigned)box << 16) : 0u;
            for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o); if (lane >= o) incl += v; }
            if (lane == 63) smem[threadIdx.x >> 6] = (int)incl;   // (the stack columns are not in use yet)
            __syncthreads();                                      // the waves' totals; and the node copy above is complete
            for (unsigned wv = 0; wv < (threadIdx.x >> 6); ++wv) incl += (unsigned)smem[wv];
            const unsigned nT = incl & 0xffffu, nB = incl >> 16;   // triangles / boxes up to and including this leaf
            if (leaf && nT * 48u + nB * 32u <= (unsigned)kHotBytes) {
                const f4v *gt = reinterpret_cast<const f4v *>(tris + first);
                lds_f4 *dt = hotT + 3 * (nT - (unsigned)n);
                for (int j = 0; j < n; ++j) {
                    f4v a = gt[3 * j];
                    a.w = __int_as_float(first + j);   // what hitLeaf gets
                    dt[3 * j] = a; dt[3 * j + 1] = gt[3 * j + 1]; dt[3 * j + 2] = gt[3 * j + 2];
                }
                if (box) {
                    const f4v *gb = reinterpret_cast<const f4v *>(sc.leaf_box) + 2 * (size_t)first;
                    lds_f4 *db = hotT + kHotBytes / 16 - 2 * nB;
                    db[0] = gb[0]; db[1] = gb[1];
                }
                ((lds_int *)(topN + 6 * kTopCache + node))[slot] = ~((n << 24) | (kHotBase + (int)(((nB - (unsigned)box) << 4) + nT - (unsigned)n)));
            }
        }
        __syncthreads();
    }

    auto push = [&](int &n, int v) {
        if (!SPILL || n < lds_entries) stk[n * kBlock] = v;
        else spl[(n - lds_entries) * spillStride] = v;
        ++n;
    };
    auto pop = [&](int &n) -> int {
        --n;
        return (!SPILL || n < lds_entries) ? stk[n * kBlock] : spl[(n - lds_entries) * spillStride];
    };

#ifndef GX_T4_REFILL_IN_A
#define GX_T4_REFILL_IN_A 0   // measured: 48.2 vs 37.9 ms (profiles/README.md) -- the extra code in the node loop costs more than the lanes it keeps on
#endif
    unsigned poolBase = 0, poolCount = 0;   // wave-uniform: the chunk of work items this wave owns
    bool exhausted = false;                 // wave-uniform: the global cursor ran past `total`
    unsigned rqHead = 0, rqCount = 0;       // wave-uniform: set-up rays waiting in LDS
    unsigned nNeeApplied = 0;               // wave-uniform: light estimates this wave has added (Counters::nee_applied_trace)

    // per-lane ray state
    bool live = false;
    int pk = 0, path = -1;   // pk: kind (bits 0-1: 0 continuation, 1 shadow, 2 MIS) | kz << 2 (Triangle.cpp:91) | done << 4 | exact << 5 | first hit ends the walk << 6 | the staged leaf is in progress (its box is decided) << 7
    // Bit 8 of pk (kMisOwed) does not belong to the lane's ray but to the lane as a set-up slot: the vertex item this lane set up in the last
    // batch has a MIS ray that is still to be set up.  The kernel has no register to spare, scalar or vector, and this bit costs none.
    constexpr int kMisOwed = 256;
    V3 ro, inv;
    float Sx = 0, Sy = 0, tMax = 0;
    unsigned oNX = 0, oNY = 16, oNZ = 32;   // byte offset of the near plane of each axis inside a DNode4 (far = 48 | 80 | 112 - near ... see below)
    unsigned ordShift = 0;                  // bit offset of this octant's 4-bit code in the node's `codes`
    int cur = -1, toVisit = 0, leafOff = 0, leafN = 0, hitLeaf = -1;
    uint32_t cntNodes = 0, cntTris = 0, cntRetests = 0, cntNodesGlobal = 0, cntTrisHot = 0;   // cntTris counts every triangle loaded, the hot ones (cntTrisHot) too
#ifdef GX_TRACE_STATS
    unsigned long long st_[24] = {0};
#endif

    // take record `slot` of this wave's ready queue into the lane
    auto take_ray = [&](unsigned slot) {
        const lds_float *q = (const lds_float *)(rq + slot);
        ro = V3(q[0 * kRqStride], q[1 * kRqStride], q[2 * kRqStride]); tMax = q[3 * kRqStride];
        inv = V3(q[4 * kRqStride], q[5 * kRqStride], q[6 * kRqStride]); Sx = q[7 * kRqStride];
        Sy = q[8 * kRqStride];
        pk = (pk & kMisOwed) | __float_as_int(q[9 * kRqStride]);
        path = __float_as_int(q[10 * kRqStride]);
        hitLeaf = SPH ? rq[slot + 11 * kRqStride] : -1;
        const int neg0 = inv.x < 0, neg1 = inv.y < 0, neg2 = inv.z < 0;
        oNX = neg0 ? 48u : 0u; oNY = neg1 ? 64u : 16u; oNZ = neg2 ? 80u : 32u;   // lox 0 loy 16 loz 32 hix 48 hiy 64 hiz 80
        ordShift = 4u * (unsigned)(neg0 | (neg1 << 1) | (neg2 << 2));
        cur = ((pk >> 4) & 1) ? -1 : sc.root4; toVisit = 0; leafN = 0;
        live = true;
    };
    // write the result of the lane's finished ray
    auto retire_ray = [&]() {
        const int kind = pk & 3;
        if constexpr (Q == kT4QueryClosest) pa.hits[path].prim = hitLeaf;   // k_query_finish writes the rest of the record
        else if constexpr (Q == kT4QueryAny) pa.occluded[path] = hitLeaf != -1 ? 1 : 0;
        else if (kind == 0) {
            pa.hit[path] = hitLeaf;
            // The shade class of a triangle hit is looked up from `hit` by the binning pass (k_compact<COMPACT_HITCLASS>: tri_class[hit]) --
            // a dependent gather here would stall the whole wave once per retire.  Only hits without a triangle get their class here.
            if (hitLeaf < 0) {
                int cls = sc.escape_class;   // misses that still have to collect an infinite light: a queue of their own, or the code of class 0
                if (SPH && hitLeaf != -1) { const int mat = sc.spheres[-2 - hitLeaf].material; if (mat >= 0) cls = sc.materials[mat].shade_class; }
                else if (sc.lt.n_infinite == 0) {
                    // a ray that escapes a scene without infinite lights adds nothing and ends its path (PathIntegrator.cpp:101-113):
                    // no shading class (4 is binned nowhere), so it does not take a lane in a k_shade wave
                    cls = 4;
                    pa.pflags[path] = 0;
                }
                pa.pclass[path] = (unsigned char)cls;
            }
        }
        else if (kind == 1) {
            // (bit 1 of a result byte: this ray has been traced -- what the set-up batch that adds light estimates waits for, nee_ready)
            if (w.vis) w.vis[4 * (size_t)path] = hitLeaf == -1 ? 3 : 2;
            else reinterpret_cast<float *>(&pa.sh_o[(size_t)path * kRS])[3] = hitLeaf == -1 ? 1.f : 0.f;
        } else {
            const int expect = __float_as_int(pa.mis_o[(size_t)path * kRS].w);   // the leaf triangle the light sample expects (-1: nothing), written by k_shade
            bool ok = (expect >= 0) ? (hitLeaf == expect) : (hitLeaf == -1);
            if (w.vis) w.vis[4 * (size_t)path + 1] = ok ? 3 : 2;
            else reinterpret_cast<float *>(&pa.mis_o[(size_t)path * kRS])[3] = ok ? 1.f : 0.f;
        }
        live = false;
    };
    // One round of light estimates: lane l looks at work item first + l where that lies in [lo, hi) -- vertex items this wave has set up
    // and nobody else touches -- and adds the estimate of a vertex whose rays are all back (nee_ready), marking it; the others are left
    // to k_nee_combine.  (first may have wrapped below 0: such lanes fail the test against hi.)
    auto nee_round = [&](unsigned first, unsigned lo, unsigned hi) {
        if constexpr (Q == kT4Render) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // this wave's retire stores have landed (the CU's L1 serves its own stores)
            const unsigned j = first + (unsigned)lane;
            bool did = false;
            if (j >= lo && j < hi) {
                const int p = w.q_nee[j - (unsigned)w.n_closest];
                unsigned *vw = reinterpret_cast<unsigned *>(w.vis) + p;
                const unsigned v = __hip_atomic_load(vw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (nee_ready(v)) {
                    nee_apply(pa, p, v);
                    reinterpret_cast<unsigned char *>(vw)[3] = 1;
                    did = true;
                }
            }
            nNeeApplied += (unsigned)__popcll(__ballot(did));
        }
    };
#ifdef GX_TRACE_STATS
#define GX_TICK(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); GX_STAT(i, t_ - tick_); tick_ = t_; } while (0)
    unsigned long long tick_ = __builtin_amdgcn_s_memtime();
#else
#define GX_TICK(i) do {} while (0)
#endif
    while (true) {
        GX_STAT(0, 1);
        GX_TICK(15);   // retire + loop overhead of the previous trip
        // ---------------- refill ----------------
        const bool need = !live;
        const unsigned long long needMask = __ballot(need);
        if (needMask) {
            if (rqCount == 0) {
                // the last batch left MIS rays behind: they are set up (as a batch of their own) before the pool moves on or new work is fetched
                const bool misPass = Q == kT4Render && __ballot((pk & kMisOwed) != 0) != 0;
                if (!misPass && poolCount == 0 && !exhausted) {
#if GX_T4_NEE_TAIL
                    // the chunk that has just run out: its last kNeeLag items have had no set-up batch behind them.  Their rays have all been
                    // drawn from the queue, most of the older ones are back: one round per 64 of them before the wave asks for more work
                    if (Q == kT4Render && !firstFetch && w.nee_in_trace && w.vis && !w.order && poolBase > (unsigned)w.n_closest) {
                        const unsigned len = poolBase <= plan.big ? plan.c : (poolBase <= plan.mid_end ? 128u : (poolBase - 1u - plan.mid_end) % 64u + 1u);
                        const unsigned lo = max(poolBase - len, (unsigned)w.n_closest);
                        for (unsigned back = (unsigned)kNeeLag; back >= 64u; back -= 64u)
                            if (poolBase - lo + 64u > back) nee_round(poolBase - back, lo, poolBase);
                    }
#endif
                    // the cursor counts chunks (chunk_plan / chunk_range, trace_kernel.hip.h); a wave's FIRST chunk is its own number -- no
                    // atomic: 5120 waves asking at once at the start of a launch queue up behind one address for ~60 us
                    unsigned v = waveId;
                    if (!firstFetch) {
                        if (lane == 0) v = nWaves + atomicAdd(cursor, 1u);
                        v = __shfl(v, 0);
                    }
                    firstFetch = false;
                    if (!chunk_range(plan, v, total, &poolBase, &poolCount)) { exhausted = true; poolCount = 0; }
#ifdef GX_TAIL_STAMP
                    if (Q == kT4Render && !tailSeen && (exhausted || poolBase + poolCount >= tailFrom)) {
                        tailSeen = true;
                        if (lane == 0) atomicMin(&g_tail[0], (unsigned long long)wall_clock64());
                    }
#endif
                }
                if (misPass || poolCount > 0) {
                    // ---- batch set-up: every lane prepares one ray (the ray-only part of Bounds3::IntersectP and Triangle::Intersect) -- of the
                    // next `take` work items, or (misPass) the MIS rays of the vertex items of the previous batch, over which the pool has
                    // not moved on yet: lane l has item poolBase + l in both
                    const unsigned take = min(poolCount, (unsigned)kRayQueue);
                    // ---- light estimates of the vertices this wave set up kNeeLag items earlier in this chunk: lane l looks at item
                    // poolBase + l - kNeeLag.  Their rays were parked by this wave and taken by its lanes alone, so no other wave touches the
                    // vertex's word or its L; where all its rays are back (nee_ready) the lane adds the estimate and marks the vertex, the others
                    // are left to k_nee_combine.  The chunk's first item follows from its end and the plan (chunk_range): the kernel has no
                    // register for it.  The three dependent loads ride on the set-up's own: the queue entry is asked for here, the vertex's
                    // word once the set-up's records are in, and the estimate is added after the set-up's arithmetic.
                    int neeP = -1;   // the lagging vertex's path
                    bool neeOn = false;   // wave-uniform: this batch has lagging items
                    if constexpr (Q == kT4Render) {
                        const unsigned chunkEnd = poolBase + poolCount;
                        // (a 64-item chunk, the only kind that can be cut short by the end of the list, never has a lagging item of its own)
                        const unsigned chunkLen = chunkEnd <= plan.big ? plan.c : (chunkEnd <= plan.mid_end ? 128u : 0u);
                        const unsigned lo = max(chunkEnd - chunkLen, (unsigned)w.n_closest) + (unsigned)kNeeLag;   // first position whose lagging item is a vertex of this chunk
                        neeOn = !misPass && w.nee_in_trace && w.vis && !w.order && poolBase + 63u >= lo;
                        if (neeOn && poolBase + (unsigned)lane >= lo) neeP = w.q_nee[poolBase + (unsigned)lane - (unsigned)kNeeLag - (unsigned)w.n_closest];
                    }
                    bool valid = false, wantMis = false;
                    float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;
                    int sphHit = -1;
                    float4 o4 = make_float4(0, 0, 0, 0), d4 = o4;
                    int kind_ = 0, path_ = 0, any_ = 0;
                    float tMax_ = 0.f;
                    if (misPass ? (pk & kMisOwed) != 0 : (unsigned)lane < take) {
                        unsigned i = poolBase + (unsigned)lane;
                        if (w.order) i = w.order[i];
                        valid = true;
                        if constexpr (Q != kT4Render) {   // a query: the caller's gnxr_ray i, one kind for the whole launch
                            path_ = (int)i;
                            o4 = pa.rays[2 * (size_t)i]; d4 = pa.rays[2 * (size_t)i + 1];
                            tMax_ = o4.w;
                            kind_ = Q == kT4QueryAny ? 1 : 0; any_ = kind_;
                        } else if (i < (unsigned)w.n_closest) {
                            path_ = w.q_closest ? w.q_closest[i] : (int)i;
                            o4 = pa.ray_o[(size_t)path_ * kRS]; d4 = pa.ray_d[(size_t)path_ * kRS];
                            tMax_ = o4.w;
                        } else {
                            // one work item per NEE vertex.  Its set-up loads the shadow record, whose flags say which rays the vertex spawned: bit 0
                            // the shadow ray (set up here), bit 1 the MIS ray.  The MIS records are read by the lanes that have one only -- the
                            // direction k_shade sampled from the BSDF hits the sampled light at a few percent of the vertices of a scene with
                            // one small light -- in the batch that follows (misPass): a second round trip for the batches that hold such a lane,
                            // none for the others.  (The MIS arrays of integrators without w.vis are sized by what they use: nothing else reads them.)
                            path_ = w.q_nee[i - (unsigned)w.n_closest];
                            if (!misPass) {
                                kind_ = 1; any_ = 1;
                                o4 = pa.sh_o[(size_t)path_ * kRS]; d4 = pa.sh_d[(size_t)path_ * kRS]; tMax_ = o4.w;
                                const int nflags = __float_as_int(d4.w);
                                valid = (nflags & 1) != 0;     // else: this vertex spawned no shadow ray
                                wantMis = (nflags & 2) != 0;
                            } else {
                                kind_ = 2;
                                o4 = pa.mis_o[(size_t)path_ * kRS]; d4 = pa.mis_d[(size_t)path_ * kRS];
                                tMax_ = GX_INF;
                                // a MIS ray that expects to escape (an infinite light was sampled) asks "is there any hit at all": with tMax = inf
                                // the closest-hit walk and the any-hit walk visit the same nodes up to the first accepted triangle, and that
                                // triangle already decides the answer
                                any_ = __float_as_int(o4.w) < 0 ? 1 : 0;
                            }
                        }
                    }
                    unsigned neeV = 0;   // the lagging vertex's word
#if GX_T4_NEE_BESIDE
                    float4 neeX = make_float4(0, 0, 0, 0), neeB = neeX, neeL = neeX;   // ... and its records, asked for beside the word (one dependent level less, bytes for the vertices that add nothing)
#endif
                    if constexpr (Q == kT4Render) {
                        if (neeOn) {
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // this wave's retire stores have landed (the CU's L1 serves its own stores)
                            if (neeP >= 0) {
                                neeV = __hip_atomic_load(reinterpret_cast<unsigned *>(w.vis) + neeP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#if GX_T4_NEE_BESIDE
                                neeX = pa.sh_X[(size_t)neeP * kRS]; neeB = pa.nbeta[(size_t)neeP * kRS]; neeL = pa.L[neeP];
#endif
                            }
                        }
                    }
                    {
                        if (valid) {
                            const V3 o(o4.x, o4.y, o4.z), d(d4.x, d4.y, d4.z);
                            const V3 iv(1.f / d.x, 1.f / d.y, 1.f / d.z);          // BVHAccel.cpp:657
                            const RayShear sh = ray_shear(d);                       // Triangle.cpp:91-105 (Sz == 1 / d[kz] == iv[kz])
                            int done = 0;
                            for (int si = 0; SPH && si < sc.n_spheres; ++si) {     // spheres live outside the BVH and are tested first
                                float tH;
                                if (sphere_test(sc.spheres[si], o, d, tMax_, &tH)) {
                                    sphHit = -2 - si;
                                    if (any_) { done = 1; break; }
                                    tMax_ = tH;
                                }
                            }
                            // a zero direction component makes 1 / d infinite and (plane - o) * (1 / d) possibly NaN: such rays walk with the
                            // reference's exact comparison sequence
                            const int ex = (__builtin_isinf(iv.x) || __builtin_isinf(iv.y) || __builtin_isinf(iv.z)) ? 1 : 0;
                            r0 = make_float4(o.x, o.y, o.z, tMax_);
                            r1 = make_float4(iv.x, iv.y, iv.z, sh.Sx);
                            r2 = make_float4(sh.Sy, __int_as_float(kind_ | (sh.kz << 2) | (done << 4) | (ex << 5) | (any_ << 6)), __int_as_float(path_), 0.f);
                        }
                    }
                    const unsigned long long vm = __ballot(valid);
                    if (valid) {
                        const int slot = __popcll(vm & ((1ull << lane) - 1ull));
                        lds_float *q = (lds_float *)(rq + slot);
                        q[0 * kRqStride] = r0.x; q[1 * kRqStride] = r0.y; q[2 * kRqStride] = r0.z; q[3 * kRqStride] = r0.w;
                        q[4 * kRqStride] = r1.x; q[5 * kRqStride] = r1.y; q[6 * kRqStride] = r1.z; q[7 * kRqStride] = r1.w;
                        q[8 * kRqStride] = r2.x; q[9 * kRqStride] = r2.y; q[10 * kRqStride] = r2.z;
                        if (SPH) rq[slot + 11 * kRqStride] = sphHit;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the records are read by other lanes of this wave
                    rqCount = (unsigned)__popcll(vm); rqHead = 0;
                    if constexpr (Q == kT4Render) {
                        if (neeOn) {
                            const bool did = neeP >= 0 && nee_ready(neeV);
                            if (did) {
#if GX_T4_NEE_BESIDE
                                if (nee_adds(neeV)) pa.L[neeP] = nee_sum(pa, neeP, neeV, neeX, neeB, neeL);
#else
                                nee_apply(pa, neeP, neeV);
#endif
                                reinterpret_cast<unsigned char *>(w.vis)[4 * (size_t)neeP + 3] = 1;
                            }
                            nNeeApplied += (unsigned)__popcll(__ballot(did));
                        }
                    }
                    bool advance = true;
                    if (Q == kT4Render) {
                        // the vertex items of this batch that also have a MIS ray: their lanes remember it (kMisOwed), and the pool stays on the
                        // batch; when the queue has run empty those lanes read their queue entries again and set the MIS rays up
                        if (misPass) pk &= ~kMisOwed;
                        else if (wantMis) pk |= kMisOwed;
                        advance = misPass || __ballot(wantMis) == 0;
                    }
                    if (advance) { poolBase += take; poolCount -= take; }
                    GX_STAT(7, 1);
                    GX_STAT(8, misPass ? rqCount : take);
                }
            }
            if (rqCount > 0) {
                const unsigned rank = (unsigned)__popcll(needMask & ((1ull << lane) - 1ull));
                if (need && rank < rqCount) take_ray(rqHead + rank);
                const unsigned t = min(rqCount, (unsigned)__popcll(needMask));
                rqHead += t; rqCount -= t;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");       // all reads of the queue precede the next batch's writes
            }
        }
        GX_TICK(11);
        const unsigned long long liveMask = __ballot(live);
        if (liveMask == 0) {
            if (exhausted && rqCount == 0 && poolCount == 0) break;   // (poolCount > 0 while a batch still owes its MIS rays)
            continue;   // nothing was ready this round: fetch / set up on the next iteration
        }

        // ---------------- phase A: interior traversal until at most half of the live lanes still look for a leaf ----------------
        int nLive = __popcll(liveMask);
        GX_STAT(9, nLive);
        while (true) {
#if GX_T4_REFILL_IN_A
            // a lane whose ray has ended does not wait for phase C: it writes its result and takes the next set-up ray from the wave's
            // queue right here (a pop is a dozen ds_reads), so the node steps below run with more lanes on
            {
                const bool fin = live && cur == -1 && leafN == 0;
                const unsigned long long finMask = __ballot(fin);
                if (finMask != 0 && rqCount > 0) {
                    if (fin) retire_ray();
                    const unsigned rank = (unsigned)__popcll(finMask & ((1ull << lane) - 1ull));
                    if (fin && rank < rqCount) take_ray(rqHead + rank);
                    const unsigned t = min(rqCount, (unsigned)__popcll(finMask));
                    rqHead += t; rqCount -= t;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    nLive = __popcll(__ballot(live));
                }
            }
#endif
            if (live && leafN == 0 && cur < -1) {   // the next reference is a leaf: stage it, pre-pop its successor
                const int lr = ~cur;
                leafOff = lr & 0xffffff; leafN = (lr >> 24) & 0x7f;
                cur = (toVisit == 0) ? -1 : pop(toVisit);
            }
            // A lane that already holds a leaf keeps walking (speculatively, with the tMax it has) until it reaches a second
            // leaf: every node it visits is one the reference visits or a superset of them (tMax only shrinks), and each
            // leaf is re-tested against the current tMax before its triangles are (phase B), so results do not change.
            const bool searching = live && cur >= 0 && (kSpeculate || leafN == 0);
            const bool hungry = searching && leafN == 0;
            const int nSearching = __popcll(__ballot(hungry));
            if (nSearching * kTraceLeaveDiv <= nLive * kTraceLeaveMul && (nSearching == 0 || nSearching < nLive)) break;
#ifdef GX_TRACE_STATS
            { const int ns = __popcll(__ballot(searching)); GX_STAT(1, 1); GX_STAT(2, ns); const int nh_ = __popcll(__ballot(live && leafN > 0 && !searching)), nf_ = __popcll(__ballot(live && cur == -1 && leafN == 0)), nsp_ = __popcll(__ballot(searching && leafN > 0));
              GX_STAT(20, nLive); GX_STAT(21, nh_); GX_STAT(22, nf_); GX_STAT(23, nsp_);
              const int n16 = __popcll(__ballot(searching && cur < 16)), n64 = __popcll(__ballot(searching && cur < 64)), n256 = __popcll(__ballot(searching && cur < 256)), n1k = __popcll(__ballot(searching && cur < 1024));
              GX_STAT(16, n16); GX_STAT(17, n64); GX_STAT(18, n256); GX_STAT(19, n1k); }
#endif
            if (searching) {
                if (COUNT) cntNodes++;
                // ---- one 4-wide step: test the four children (Bounds3::IntersectP per box), continue with the first one hit in the
                // reference's visiting order, push the others farthest first
                f4v nX, fX, nY, fY, nZ, fZ, cf;
                unsigned codes;
                if (cur < n_top) {   // top of the tree: from the block's LDS copy
                    const lds_f4 *L = topN + cur;
                    nX = L[(oNX >> 4) * kTopCache]; fX = L[((48u - oNX) >> 4) * kTopCache];
                    nY = L[(oNY >> 4) * kTopCache]; fY = L[((80u - oNY) >> 4) * kTopCache];
                    nZ = L[(oNZ >> 4) * kTopCache]; fZ = L[((112u - oNZ) >> 4) * kTopCache];
                    cf = L[6 * kTopCache];
                    codes = __float_as_uint(L[7 * kTopCache].z);
                } else {
                    if (COUNT) cntNodesGlobal++;
                    const unsigned off = (unsigned)cur << 7;
#define GX_LD4(o) (*reinterpret_cast<const f4v *>(nb + (unsigned)(off + (o))))
                    nX = GX_LD4(oNX); fX = GX_LD4(48u - oNX); nY = GX_LD4(oNY); fY = GX_LD4(80u - oNY); nZ = GX_LD4(oNZ); fZ = GX_LD4(112u - oNZ);
                    cf = GX_LD4(96u);
                    codes = *reinterpret_cast<const unsigned *>(nb + (unsigned)(off + 120u));
#undef GX_LD4
                }
                const float k = 1 + 2 * GX_GAMMA(3);
                unsigned hitMask = 0;
                if (!(pk & 32)) {
                    // finite 1 / d: no product is NaN, and the pairwise tests of Geometry.h:1389-1403 hold exactly when the merged
                    // interval [max of the three entries, min of the three (k-scaled) exits] is non-empty and overlaps (0, tMax)
// (rounding is monotone and k > 0, so the smallest of the three k-scaled exits is the k-scaled smallest exit: one multiply instead of three)
#define GX_SLAB3(C, BIT)                                                                                       \
    {                                                                                                          \
        const float e = fmaxf(fmaxf((nX.C - ro.x) * inv.x, (nY.C - ro.y) * inv.y), (nZ.C - ro.z) * inv.z);      \
        const float x = fminf(fminf((fX.C - ro.x) * inv.x, (fY.C - ro.y) * inv.y), (fZ.C - ro.z) * inv.z) * k;  \
        hitMask |= (e <= x && e < tMax && x > 0.f) ? (BIT) : 0u;                                                \
    }
                    GX_SLAB3(x, 1u) GX_SLAB3(y, 2u) GX_SLAB3(z, 4u) GX_SLAB3(w, 8u)
#undef GX_SLAB3
                } else {
#define GX_SLAB(C, BIT)                                                                   \
    {                                                                                     \
        float tMin = (nX.C - ro.x) * inv.x, tMx = (fX.C - ro.x) * inv.x;                  \
        float tyMin = (nY.C - ro.y) * inv.y, tyMax = (fY.C - ro.y) * inv.y;               \
        tMx *= k; tyMax *= k;                                                             \
        bool ok = !(tMin > tyMax || tyMin > tMx);                                         \
        if (tyMin > tMin) tMin = tyMin;                                                   \
        if (tyMax < tMx) tMx = tyMax;                                                     \
        float tzMin = (nZ.C - ro.z) * inv.z, tzMax = (fZ.C - ro.z) * inv.z;               \
        tzMax *= k;                                                                       \
        ok = ok && !(tMin > tzMax || tzMin > tMx);                                        \
        if (tzMin > tMin) tMin = tzMin;                                                   \
        if (tzMax < tMx) tMx = tzMax;                                                     \
        ok = ok && (tMin < tMax) && (tMx > 0);                                            \
        hitMask |= ok ? (BIT) : 0u;                                                       \
    }
                    GX_SLAB(x, 1u) GX_SLAB(y, 2u) GX_SLAB(z, 4u) GX_SLAB(w, 8u)
#undef GX_SLAB
                }
                int next;
                if (hitMask == 0) next = (toVisit == 0) ? -1 : pop(toVisit);
                else {
                    const unsigned e = lut[(((codes >> ordShift) & 15u) << 4) | hitMask];   // (this octant's code, hit mask)
                    const int n = __popc(hitMask);
                    const int c0 = __float_as_int(cf.x), c1 = __float_as_int(cf.y), c2 = __float_as_int(cf.z), c3 = __float_as_int(cf.w);
                    auto child = [&](unsigned s) -> int { const int lo = (s & 1u) ? c1 : c0, hi = (s & 1u) ? c3 : c2; return (s & 2u) ? hi : lo; };
                    if (n >= 4) push(toVisit, child(e >> 6));
                    if (n >= 3) push(toVisit, child((e >> 4) & 3u));
                    if (n >= 2) push(toVisit, child((e >> 2) & 3u));
                    next = child(e & 3u);
                }
                cur = next;   // interior index (>= 0), leaf reference (< -1) or -1: done
            }
        }
        GX_TICK(12);
        // ---------------- phase B: triangle tests ----------------
#ifdef GX_TRACE_STATS
        {
            unsigned long long lm = __ballot(live && leafN > 0);
            if (lm) {
                int mx = leafN;
                for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
                int sm = live ? leafN : 0;
                for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
                const int nre = __popcll(__ballot(live && leafN > 0 && hitLeaf >= 0));
                GX_STAT(3, 1); GX_STAT(4, __popcll(lm)); GX_STAT(5, mx); GX_STAT(6, sm); GX_STAT(10, nre);
            }
        }
#endif
        if (live && leafN > 0) {
            bool visit = true;
            // BVHAccel::Intersect tests a leaf's box when it pops it, i.e. against the CURRENT ray.tMax; the 4-wide step tested it earlier with
            // an older tMax.  tMax only ever shrinks after a hit (before the first hit the earlier test stands), so a ray that has one re-tests
            // the leaf's own bounds -- exact ties (t == tMax on flat, axis-aligned boxes such as the Cornell walls) then resolve as in the
            // reference.  The bounds of a one-triangle leaf are the componentwise min / max of its vertices (Triangle::WorldBound, exact),
            // which this phase loads anyway; only larger leaves read the floats of their LinearBVHNode (leaf_box, addressed by the first triangle).
            //
            // ONE triangle per lane and trip.  A leaf of several triangles (the reference keys its build on the centroid of a primitive's BOUNDS,
            // so the two triangles of an axis-aligned quad -- every Cornell wall -- share a leaf, and almost every ray ends on a wall) stays staged
            // with its next triangle: looping over it here kept the whole wave for a second round with a handful of lanes on in more than half
            // of all trips (tests/dev_stats.py: 1.55 rounds per trip).  Its box is tested once, at its first triangle (pk bit 7 remembers);
            // the triangles are still tested in order, each against the tMax the previous ones left.
            const bool first = (pk & 128) == 0;
            const bool retest = first && (SPH ? hitLeaf != -1 : hitLeaf >= 0);
            const bool fromVerts = retest && leafN == 1 && sc.leaf1_from_verts;
            int neg[3] = {inv.x < 0, inv.y < 0, inv.z < 0};
            const bool hot = leafOff >= kHotBase;   // the leaf is in the block's LDS: the same bits from there
            if (retest && !fromVerts) {
                float4 b0, b1;
                if (hot) {
                    const lds_f4 *B = hotT + (kHotBytes / 16 - 2) - 2 * ((leafOff >> 4) & 15);
                    const f4v u = B[0], v = B[1];
                    b0 = make_float4(u.x, u.y, u.z, u.w); b1 = make_float4(v.x, v.y, v.z, v.w);
                } else { b0 = sc.leaf_box[2 * (size_t)leafOff]; b1 = sc.leaf_box[2 * (size_t)leafOff + 1]; }
                if (COUNT) cntRetests++;
                visit = slab_test(b0, b1, ro, inv, neg, tMax);
            }
            bool more = false;   // the leaf has further triangles to test
            if (visit) {
                RayShear shear;
                const int kz = (pk >> 2) & 3;
                shear.kz = kz; shear.kx = kz == 2 ? 0 : kz + 1; shear.ky = shear.kx == 2 ? 0 : shear.kx + 1;
                shear.Sx = Sx; shear.Sy = Sy; shear.Sz = kz == 0 ? inv.x : (kz == 1 ? inv.y : inv.z);
                V3 p0, p1, p2;
                int leafIdx = leafOff;   // the triangle's leaf-order index
                if (hot) {
                    const lds_f4 *T = hotT + 3 * (leafOff & 15);
                    const f4v a = T[0], b = T[1], c = T[2];
                    p0 = V3(a.x, a.y, a.z); p1 = V3(b.x, b.y, b.z); p2 = V3(c.x, c.y, c.z);
                    leafIdx = __float_as_int(a.w);
                    if (COUNT) cntTrisHot++;
                } else load_tri(tris, leafOff, &p0, &p1, &p2);
#ifndef GX_COUNT_TRI_TESTS   // the counter is the triangles LOADED (what the byte model of bench.py charges), box-culled one-triangle leaves included;
                if (COUNT) cntTris++;   // -DGX_COUNT_TRI_TESTS (development builds) counts the triangles TESTED: the same number for every collapse of one binary tree
#endif
                bool inBox = true;
                if (fromVerts) {
                    const float4 b0 = make_float4(fminf(fminf(p0.x, p1.x), p2.x), fminf(fminf(p0.y, p1.y), p2.y), fminf(fminf(p0.z, p1.z), p2.z), fmaxf(fmaxf(p0.x, p1.x), p2.x));
                    const float4 b1 = make_float4(fmaxf(fmaxf(p0.y, p1.y), p2.y), fmaxf(fmaxf(p0.z, p1.z), p2.z), 0.f, 0.f);
                    inBox = slab_test(b0, b1, ro, inv, neg, tMax);
                }
                more = leafN > 1;
#ifdef GX_COUNT_TRI_TESTS
                if (COUNT && inBox) cntTris++;
#endif
                TriHit h;
                if (inBox && tri_test_sheared(p0, p1, p2, ro, shear, tMax, &h)) {
                    hitLeaf = leafIdx;
                    if (pk & 64) { cur = -1; more = false; }   // IntersectP returns at the first hit (and so may a MIS ray that expects a miss)
                    else tMax = h.t;                            // GeometricPrimitive::Intersect shrinks ray.tMax
                }
            }
            if (more) { leafOff += 1; leafN -= 1; pk |= 128; }
            else { leafN = 0; pk &= ~128; }
        }
        GX_TICK(13);
        // ---------------- phase C: retire finished rays ----------------
        if (live && cur == -1 && leafN == 0) retire_ray();
    }
#ifdef GX_TRACE_STATS
    if (lane == 0) for (int i = 0; i < 24; ++i) if (st_[i]) atomicAdd(&g_trace_stats[i], st_[i]);
#endif
    if (Q == kT4Render && nNeeApplied != 0 && lane == 0) atomicAdd(&ctr->nee_applied_trace, (unsigned long long)nNeeApplied);
    if (COUNT) {
        atomicAdd(&ctr->nodes, (unsigned long long)cntNodes);
        atomicAdd(&ctr->tris, (unsigned long long)cntTris);
        atomicAdd(&ctr->retests, (unsigned long long)cntRetests);
        atomicAdd(&ctr->nodes_global, (unsigned long long)cntNodesGlobal);
        atomicAdd(&ctr->tris_hot, (unsigned long long)cntTrisHot);
    }
#ifdef GX_TAIL_STAMP
    if (Q == kT4Render && lane == 0) {
        atomicMax(&g_tail[1], (unsigned long long)wall_clock64());
        __threadfence();
        if (atomicAdd(&g_tail[3], 1ull) == (unsigned long long)nWaves - 1ull) {   // the last wave of the launch
            __threadfence();
            const unsigned long long tEnd = atomicExch(&g_tail[1], 0ull), tCross = atomicExch(&g_tail[0], ~0ull), tStart = atomicExch(&g_tail[2], ~0ull);
            atomicExch(&g_tail[3], 0ull);
            const unsigned long long behind = tEnd > tCross ? tEnd - tCross : 0ull, all = tEnd > tStart ? tEnd - tStart : 0ull;
            const int o = total >= (1u << 24) ? 8 : 4;
            g_tail[o] += behind; g_tail[o + 1] += all; g_tail[o + 2] += 1ull; g_tail[o + 3] += total;
            if (o == 8) { g_tail[4] += behind; g_tail[5] += all; g_tail[6] += 1ull; g_tail[7] += total; }
        }
    }
#endif
}

}  // namespace gnxr
