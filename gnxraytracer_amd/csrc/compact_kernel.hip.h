// compact_kernel.hip.h -- order-preserving stream compaction of the path queues in ONE pass over memory.
//
// Atomic appends cap out at ~88 increments/us per address on MI355X (MI355X_MICROARCH.md, row "dequeue"): with one append per wave the
// first version spent 1.3 ms per launch just binning 16 M paths (profiles/r01_c_*), and appends lose the slot order that keeps the float4
// state arrays read in (mostly) ascending, coalesced order.  Rounds 1 - 3 therefore ran three launches per binning -- count per tile, a
// single-block scan of the tile counts, scatter -- which read every queue entry and gathered every key twice.  k_compact does the same
// binning with one read: a chained scan with decoupled look-back (Merrill & Garland 2016).
//
//   mode FLAGS    : predicate o = bit o of pflags[path]   (bit0 path continues, bit1 has NEE record, bit2 shadow ray valid, bit3 MIS ray
//                   valid -- 2, 3 counted only; a fifth count: continues AND lives below `split`)
//   mode CLASS    : predicate o = (keys[path] == o)       (VolPath: the state of the path)
//   mode HITCLASS : as CLASS, with the key of a path whose ray hit a triangle looked up here (tri_class[hit[path]]); keys[path] (pclass) is
//                   written by the traversal kernels for misses and sphere hits only, so that their retire step has no dependent gather.
//                   Nothing else reads pclass, so the class of a triangle hit is no longer written back to it.  The byte holds the shade
//                   class and, above it, the kind of a class-1 material (gnxr_device_types.h MATERIAL_KIND_*); the render plan's table
//                   `kind_queue` (one byte per kind) names the shade queue of each kind: o = class == 1 ? kind_queue[kind] : class.
//                   (pclass holds plain classes: sphere hits go to queue 1, and the plan gives a scene with spheres no other glossy queue.)
//
// What a block does per tile (kCompactTile consecutive queue entries, kCompactChunks per thread;
// a wave holds kCompactSpan consecutive entries, 64 per chunk, so that every load instruction is coalesced):
//   1. take the next tile from the ticket counter;
//   2. load its entries and gather their keys ONCE; the entries stay in registers, the keys shrink to one bit per chunk and scattered
//      predicate (a 32-bit mask per predicate);
//   3. count every chunk with a ballot; the waves' counts meet in LDS: offsets of the waves in the tile + the tile's count per predicate;
//   4. wave o publishes the count of predicate o in the tile's descriptor and obtains the tile's exclusive prefix by looking back over the
//      descriptors of the tiles before it, 64 at a time: it adds counts until it meets a tile whose inclusive prefix is already known, then
//      publishes its own inclusive prefix;
//   5. scatter from the registers to prefix + offset + rank in the wave;
//   6. the last tile writes totals[o] = its inclusive prefix, counted-only predicates included.
//
// Descriptor: one 64-bit word per (predicate, tile) = {tag, value}, tag = sequence number of the compaction << 2 | state (1 count, 2
// inclusive prefix), written with ONE relaxed agent-scope 64-bit store and read with one such load: tag and value are never seen apart, there
// is no payload besides the word and hence no fence.  Every compaction of a handle has a sequence number of its own (RenderState::compact_seq),
// so what an earlier pass left reads as "not ready" and nothing is cleared between passes (the buffer is zeroed when it is allocated and
// when the 30-bit number wraps).
//
// Why it cannot stall: tiles are handed out in increasing order by ONE ticket counter, also a block's first, so a block only ever waits for
// tiles that a running block took before -- the lowest unfinished tile never waits.  Nothing rests on the whole grid being resident.  The
// look-back poll is bounded all the same (kCompactPollCap polls with a sleep between them, seconds where a wait takes microseconds): a block
// that reaches the cap raises Counters::compact_stall, parks the ticket counter beyond every tile so that the other blocks leave, and
// returns; the host turns the flag into GNXR_ERR_RUNTIME at its next look at the counters.  After a stall the output queues and the totals of
// that compaction are undefined (the last tile may never write them): what is queued behind it on the stream runs on the counts of an
// earlier compaction -- valid bounds, wrong work -- and the render is abandoned with an error, never returned as an image.
//
// Ticket arithmetic.  A block that took a run of R > 1 tiles and worked through it in order would make its successor wait for its LAST tile:
// the blocks would run one after another.  So the run a ticket covers is held in registers as a whole -- it IS the tile: 512 threads x 32
// entries = 16384 entries = eight of the former 2048-entry tiles per ticket (a wave holds 2048 consecutive entries, entry = wave span +
// chunk * 64 + lane).  The largest pass (265 M paths) has 16.2 k tiles: 16.2 k atomics on one address are 0.18 ms back to back at 88 / us,
// against >= 0.6 ms that such a pass needs to move its >= 2.4 GB, i.e. the counter runs below a third of what one address sustains; a
// ticket per 2048 entries (130 k) would have been 1.5 ms.  The two counters of a handle alternate: a pass uses ticket[seq & 1] and zeroes
// the other for its successor (same stream), so no launch clears a counter either.
//
// Registers (tools/kernel_regs.py): 108 - 133 VGPRs, no scratch (scalar registers spill to vector lanes: the ballots), i.e. one or two
// 512-thread blocks per CU with 32 independent loads per thread in flight each.  With 16 entries per thread it is 58 - 77 VGPRs.
// Measured on cfg 3 (profiles/README.md, "Single-pass compaction"): 71.6 ms per 10 steps against 103.5 ms for the three launches it
// replaces; 16 entries per thread: 79.7 ms at two blocks per CU, 74.0 ms at three.  k_compact<FLAGS, 4, 3> (Whitted) has 133 VGPRs and runs
// one block per CU.  The no-scratch figure rests on the lane permute of the masks below; profiles/kernel_regs_single_pass.txt is the
// tools/kernel_regs.py report of this build -- re-run it after a compiler change.
#pragma once
#include "device_math.h"
#include "gnxr_device_types.h"

namespace gnxr {

constexpr int kCompactBlock = 512;
enum CompactMode { COMPACT_FLAGS = 0, COMPACT_CLASS = 1, COMPACT_HITCLASS = 2 };

template <int MODE>
GX_DEV bool compact_pred(unsigned key, int o) { return MODE == COMPACT_FLAGS ? ((key >> o) & 1u) != 0 : key == (unsigned)o; }
// HITCLASS: the shade queue of a key byte (shade class | kind << kClassKeyKindShift); kind_queue: byte k = the queue of class-1 kind k
GX_DEV unsigned compact_class_queue(unsigned key, unsigned kind_queue) {
    const unsigned cls = key & (unsigned)kClassKeyClassMask;
    return cls == 1u ? (kind_queue >> ((key >> kClassKeyKindShift) * 8u)) & 0xffu : cls;
}

constexpr int kCompactChunks = 32;   // entries per thread: one bit each in a 32-bit predicate mask
constexpr int kCompactTile = kCompactBlock * kCompactChunks;
constexpr int kCompactWaves = kCompactBlock / 64;
constexpr int kCompactSpan = 64 * kCompactChunks;                  // consecutive entries of a tile that one wave holds
constexpr int kCompactBlocksPerCu = 2;                            // resident at <= 128 registers; more blocks would only queue for tickets
constexpr int kCompactGather = 8;                                  // chunks whose keys are gathered together (bounds the registers in flight)
constexpr unsigned kCompactPollCap = 1u << 21;
constexpr int kCompactMaxOut = 5;                                  // predicates a compaction counts at most (descriptor rows)
static_assert(kCompactChunks <= 32 && kCompactChunks % kCompactGather == 0, "predicate masks are 32-bit");
static_assert(kCompactMaxOut <= kCompactWaves, "one wave per predicate looks back");

enum : unsigned { COMPACT_DESC_COUNT = 1u, COMPACT_DESC_PREFIX = 2u };
GX_DEV unsigned long long compact_desc(unsigned tag, unsigned value) { return ((unsigned long long)tag << 32) | value; }

// the scratch of a handle as one compaction sees it (RenderRun::compact)
struct CompactScratch {
    unsigned long long *desc;   // [predicate * stride + tile]
    int stride;                 // tiles the launch was sized for
    unsigned *ticket;           // this pass's ticket counter (zero at launch)
    unsigned *ticket_next;      // the next pass's: zeroed here
    unsigned seq;               // sequence number of this compaction, 1 .. 2^30 - 1
};

// NOUT predicates are counted (totals[0 .. NOUT)), the first NSCATTER of them are scattered to out0 .. out3.
// n_dev: the entry count lives on the device (the device-driven path loop); `n` then bounds it and sized the launch.
template <int MODE, int NOUT, int NSCATTER>
__global__ void __launch_bounds__(kCompactBlock) k_compact(const int *__restrict__ q_in, int n, const unsigned char *__restrict__ keys, CompactScratch cs,
                                                           unsigned int *totals, int *out0, int *out1, int *out2, int *out3, const int *__restrict__ hit,
                                                           const unsigned char *__restrict__ tri_class, unsigned kind_queue, int split, const unsigned *n_dev, Counters *ctr) {
    __shared__ unsigned int wtot[NOUT][kCompactWaves];   // counts per wave of the tile
    __shared__ unsigned int s_excl[NOUT];
    __shared__ unsigned int s_ticket;
    __shared__ int s_stop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *outs[4] = {out0, out1, out2, out3};
    if (n_dev) n = (int)min(*n_dev, (unsigned)n);
    const int tilesUsed = (n + kCompactTile - 1) / kCompactTile;
    if (blockIdx.x == 0 && tid == 0) *cs.ticket_next = 0u;
    if (tilesUsed == 0) {
        if (blockIdx.x == 0 && tid < NOUT) totals[tid] = 0u;
        return;
    }
    if (tid == 0) s_stop = 0;
    const unsigned tag_count = (cs.seq << 2) | COMPACT_DESC_COUNT, tag_prefix = (cs.seq << 2) | COMPACT_DESC_PREFIX;
    for (;;) {
        __syncthreads();   // the previous tile's counts and prefixes have been read
        if (tid == 0) s_ticket = atomicAdd(cs.ticket, 1u);
        __syncthreads();
        const unsigned tile = s_ticket;
        if (tile >= (unsigned)tilesUsed) break;
        // 2. the entries, once
        const long long base = (long long)tile * kCompactTile + wave * kCompactSpan + lane;
        const int *q = q_in ? q_in + base : nullptr;
        const int left = (int)min((long long)n - base, (long long)kCompactSpan);   // entry c of this lane exists if c * 64 < left
        int path[kCompactChunks];   // -1: beyond the end of the queue
#pragma unroll
        for (int c = 0; c < kCompactChunks; ++c) path[c] = c * 64 < left ? (q ? q[c * 64] : (int)base + c * 64) : -1;
        unsigned m[NSCATTER];
#pragma unroll
        for (int o = 0; o < NSCATTER; ++o) m[o] = 0u;
        unsigned acc[NOUT];   // 3. this wave's counts (wave-uniform)
#pragma unroll
        for (int o = 0; o < NOUT; ++o) acc[o] = 0u;
#pragma unroll
        for (int c0 = 0; c0 < kCompactChunks; c0 += kCompactGather) {
            unsigned key[kCompactGather];
            if (MODE == COMPACT_HITCLASS) {
                int h[kCompactGather];
#pragma unroll
                for (int j = 0; j < kCompactGather; ++j) h[j] = path[c0 + j] >= 0 ? hit[path[c0 + j]] : -1;
#pragma unroll
                for (int j = 0; j < kCompactGather; ++j) key[j] = path[c0 + j] < 0 ? 0xffu : (h[j] >= 0 ? compact_class_queue((unsigned)tri_class[h[j]], kind_queue) : (unsigned)keys[path[c0 + j]]);
            } else {
#pragma unroll
                for (int j = 0; j < kCompactGather; ++j) key[j] = path[c0 + j] >= 0 ? (unsigned)keys[path[c0 + j]] : 0xffu;
            }
#pragma unroll
            for (int j = 0; j < kCompactGather; ++j) {
                const int c = c0 + j;
                const bool valid = path[c] >= 0;
#pragma unroll
                for (int o = 0; o < NOUT; ++o) {
                    // FLAGS, fifth count: continues and lives below `split` (the sub-pass in the lower half of the state arrays)
                    const bool pr = valid && ((MODE == COMPACT_FLAGS && o == 4) ? ((key[j] & 1u) != 0 && path[c] < split) : compact_pred<MODE>(key[j], o));
                    if (o < NSCATTER) m[o < NSCATTER ? o : 0] |= (pr ? 1u : 0u) << c;
                    acc[o] += (unsigned)__popcll(__ballot(pr));
                }
            }
        }
        // (the masks come back through a lane permute of themselves: the compiler otherwise keeps all 32 x NSCATTER ballots of this phase
        // alive in scalar registers for the scatter phase, and spills them)
#pragma unroll
        for (int o = 0; o < NSCATTER; ++o) m[o] = (unsigned)__shfl((int)m[o], lane);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) if (lane == 0) wtot[o][wave] = acc[o];
        __syncthreads();
        // 4. wave o: publish the tile's count of predicate o, look back for its exclusive prefix
        if (wave < NOUT) {
            const int o = wave;
            unsigned agg = 0;
            for (int w = 0; w < kCompactWaves; ++w) agg += wtot[o][w];
            unsigned long long *d = cs.desc + (size_t)o * cs.stride;
            if (lane == 0) __hip_atomic_store(&d[tile], compact_desc(tile == 0 ? tag_prefix : tag_count, agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned excl = 0, polls = 0;
            bool stalled = false;
            long long j = (long long)tile - 1;   // the nearest tile not yet added
            while (j >= 0) {
                const long long idx = j - lane;
                const unsigned long long w = idx >= 0 ? __hip_atomic_load(&d[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : compact_desc(tag_prefix, 0u);
                const unsigned tag = (unsigned)(w >> 32);
                const unsigned long long has_prefix = __ballot(tag == tag_prefix), not_ready = __ballot(tag != tag_prefix && tag != tag_count);
                const int first = has_prefix ? __ffsll((long long)has_prefix) - 1 : 63;   // the nearest tile with a prefix; none: the whole window
                const unsigned long long needed = first >= 63 ? ~0ull : ((2ull << first) - 1ull);
                if (not_ready & needed) {
                    if (++polls > kCompactPollCap) { stalled = true; break; }
                    __builtin_amdgcn_s_sleep(2);
                    continue;
                }
                unsigned sum = lane <= first ? (unsigned)w : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
                excl += sum;
                if (has_prefix) break;
                j -= 64;
            }
            if (lane == 0) {
                if (stalled) {   // never in a correct run: end as an error, not as a hung queue
                    s_stop = 1;
                    atomicOr(&ctr->compact_stall, 1u);
                    __hip_atomic_store(cs.ticket, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    s_excl[o] = excl;
                    if (tile > 0) __hip_atomic_store(&d[tile], compact_desc(tag_prefix, excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (tile == (unsigned)tilesUsed - 1u) totals[o] = excl + agg;   // 6.
                }
            }
        }
        __syncthreads();
        if (s_stop) return;
        // 5. scatter from the registers: the tile's prefix + the waves before this one + the chunks before this one + the rank in the chunk
        unsigned run[NSCATTER];
#pragma unroll
        for (int o = 0; o < NSCATTER; ++o) {
            run[o] = s_excl[o];
            for (int w = 0; w < wave; ++w) run[o] += wtot[o][w];
        }
#pragma unroll
        for (int c = 0; c < kCompactChunks; ++c) {
#pragma unroll
            for (int o = 0; o < NSCATTER; ++o) {
                const bool pr = ((m[o] >> c) & 1u) != 0;
                const unsigned long long b = __ballot(pr);
                const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                if (pr) outs[o][run[o] + rank] = path[c];
                run[o] += (unsigned)__popcll(b);
            }
        }
    }
}

}  // namespace gnxr
