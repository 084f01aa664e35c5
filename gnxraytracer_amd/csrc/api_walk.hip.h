// api_walk.hip.h -- how a per-lane query walk (bvh_walk.hip.h) is run: the one driver under closest points, all hits, neighbours,
// sphere casts, box overlaps and triangle overlaps.  It owns the launch plan (WalkLaunch), the Morton binning of point queries (QueryBinning), the chunk loop with its
// launches (walk_launch), the front end of the entry points on device memory (walk_device: the null tests, the n == 0 return, the
// alignment, DeviceCall, query_device_scene) and the upload / walk / download of the entry points on host arrays (walk_host).  A query
// kind describes itself to it in a small struct (ClosestWalk, AllHitsWalk, NearWalk, SphereCastWalk, OverlapWalk, OverlapTriWalk in the six api_*.hip.h that follow):
//     Arrays, Spill       the kernel's arrays struct and the type of its spill pointer
//     kBinnable           the queries are 16-byte point records QueryBinning can sort; the kernel then takes their order
//     work                nullptr, or the device words the counting instantiation adds its counters to
//     entry_bytes()       of a stack entry
//     lds_levels()        the kind's LDS-levels knob, read per call
//     at(base)            the arrays of the chunk that starts at query `base`
//     kernel(wide)        the instantiation to launch for (wide, the kind's own mode, work != nullptr)
// The launch path is a template over that struct: no virtual call, nothing type-erased.  Part of api.hip's translation unit (after
// api_query.hip.h, before the six kinds).
#pragma once

// blocks per CU of a walk's grid: at the default 16 LDS levels a block's stack is 32 KB with 8-byte entries, 16 KB with 4-byte ones
static const int kWalkBlocksPerCu = 5;
// queries of one binned launch: bounds the sort's scratch (24 bytes per query) at 96 MB whatever n is, and keeps its indices in 32 bits
static const long long kClosestBinChunk = 1ll << 22;
// queries of one launch in caller order: the kernels index queries and list slots in 64 bits, a thread's spill column by its number in
// the grid; the cut keeps n * K of one launch far inside them
static const long long kWalkLaunchMax = 1ll << 30;

struct WalkLaunch {
    bool wide;                  // the 4-wide tree, else the binary one
    int entries, lds_entries;   // the bound of the stack ("The walk the queries share"), and how much of it is in LDS
    int blocks;                 // the grid of the call's largest launch: the spill has a column per thread of these
    size_t lds;                 // dynamic LDS bytes of a launch
    StreamScratch spill_scratch;
    void *spill = nullptr;      // the levels above lds_entries, on the caller's stream; nullptr when there are none
    // entry_bytes: of a stack entry; lds_levels: the call's knob, read per call; per_launch: the most queries one launch of the call takes
    int plan(const gnxr_scene *r, size_t entry_bytes, int lds_levels, long long per_launch, hipStream_t st) {
        // scene creation and gnxr_scene_set_geometry refuse a mesh without triangles; a walk has no answer for one either
        if (r->cs.n_triangles == 0) { set_error("the scene holds no triangles: there is no tree to walk"); return GNXR_ERR_INVALID; }
        wide = r->wide_ok;
        entries = wide ? r->cs.stack4_need + 1 : r->cs.bvh_max_depth + 2;   // (children - 1) per node of the deepest path, and one of slack
        lds_entries = std::min(entries, lds_levels);
        blocks = grid_for(per_launch, kWalkBlocksPerCu);
        lds = (size_t)lds_entries * kBlock * entry_bytes;
        if (entries > lds_entries) {
            HIP_TRY(spill_scratch.alloc((size_t)(entries - lds_entries) * (size_t)blocks * kBlock * entry_bytes, st));
            spill = spill_scratch.p;
        }
        return GNXR_OK;
    }
    // the grid of a launch over cnt queries: never more blocks than the spill has columns for
    int grid(long long cnt) const { return std::min(blocks, grid_for(cnt, kWalkBlocksPerCu)); }
};

// The Morton binning of a batch of point queries (closest_kernel.hip.h: k_closest_keys, then three passes of the HLBVH stage's radix sort
// over (key, index)).  reserve() takes the sort's arrays for launches of at most `most` queries from the stream-ordered allocator; sort()
// queues the key and the passes for the m queries at `queries` and returns their indices in Morton order (valid until the next sort()).
// The key orders the work and nothing more.
struct QueryBinning {
    StreamScratch scratch;
    uint32_t *k_a = nullptr, *k_b = nullptr, *v_a = nullptr, *v_b = nullptr, *hist = nullptr, *sums = nullptr;
    int reserve(long long most, hipStream_t st) {
        // keys and indices twice, the per-tile digit histograms and the scan's tile sums
        const int max_cnt = (int)most;
        const int max_tiles = (max_cnt + hlbvh::kTile - 1) / hlbvh::kTile;
        const size_t hist_words = (size_t)64 * max_tiles, sums_words = (size_t)std::max(max_tiles, (64 * max_tiles + hlbvh::kTile - 1) / hlbvh::kTile) + 1;
        HIP_TRY(scratch.alloc((4 * (size_t)max_cnt + hist_words + sums_words) * sizeof(uint32_t), st));
        k_a = reinterpret_cast<uint32_t *>(scratch.p); k_b = k_a + max_cnt; v_a = k_b + max_cnt; v_b = v_a + max_cnt;
        hist = v_b + max_cnt; sums = hist + hist_words;
        return GNXR_OK;
    }
    const uint32_t *sort(const DScene &sc, const float4 *queries, int m, hipStream_t st) {
        const int n_tiles = (m + hlbvh::kTile - 1) / hlbvh::kTile;
        hipLaunchKernelGGL(k_closest_keys, dim3(grid_for(m)), dim3(kBlock), 0, st, sc.nodes, queries, m, k_a, v_a);
        uint32_t *kin = k_a, *kout = k_b, *vin = v_a, *vout = v_b;
        for (int pass = 0; pass < 3; ++pass) {   // 18 bits, 6 per pass, least significant first
            hipLaunchKernelGGL(hlbvh::k_rs_hist, dim3(n_tiles), dim3(hlbvh::kB), 0, st, (const uint32_t *)kin, m, 6 * pass, n_tiles, hist);
            hl_scan(hist, 64 * n_tiles, sums, nullptr, st);
            hipLaunchKernelGGL(hlbvh::k_rs_scatter, dim3(n_tiles), dim3(hlbvh::kB), 0, st, (const uint32_t *)kin, (const uint32_t *)vin, m, 6 * pass, n_tiles, (const uint32_t *)hist, kout, vout);
            std::swap(kin, kout); std::swap(vin, vout);
        }
        return vin;
    }
};

// The walk of kind `q` over n queries on `st`.  A binnable kind is binned by Morton key from Knobs::closest_bin_min() queries on, a chunk
// of kClosestBinChunk at a time, and the kernel takes its queries through the sorted indices; below, and for the other kinds, a launch
// walks up to kWalkLaunchMax queries in caller order.
template <class Kind>
static int walk_launch(gnxr_scene *r, const DScene &sc, const Kind &q, int64_t n, hipStream_t st) {
    const bool binned = Kind::kBinnable && n >= Knobs::closest_bin_min();
    const long long per_launch = binned ? kClosestBinChunk : kWalkLaunchMax;
    const long long most = std::min<long long>(n, per_launch);   // queries of one launch
    WalkLaunch w;
    if (int rc = w.plan(r, q.entry_bytes(), q.lds_levels(), most, st)) return rc;
    QueryBinning bins;
    if (binned) { if (int rc = bins.reserve(most, st)) return rc; }
    const auto kernel = q.kernel(w.wide);
    typename Kind::Spill *spill = reinterpret_cast<typename Kind::Spill *>(w.spill);
    for (long long base = 0; base < n; base += per_launch) {
        const long long cnt = std::min<long long>(n - base, per_launch);
        const typename Kind::Arrays qa = q.at(base);
        if constexpr (Kind::kBinnable) {
            const uint32_t *order = binned ? bins.sort(sc, qa.queries, (int)cnt, st) : nullptr;
            hipLaunchKernelGGL(kernel, dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, order, cnt, w.lds_entries, w.entries, spill, q.work);
        } else {
            hipLaunchKernelGGL(kernel, dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, cnt, w.lds_entries, w.entries, spill, q.work);
        }
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

// K of a kind that keeps a list per query, and the records that go with it.  what: K's name in the call ("max_hits"); lowest: the
// smallest K of the mode; of: the mode or "" (it ends the message); records: the record array, in the message's words
static bool walk_list_ok(const char *what, int32_t K, int lowest, int highest, const char *of, const void *records, const char *records_what) {
    if (K < lowest || K > highest) { set_error("%s = %d is outside [%d, %d]%s", what, K, lowest, highest, of); return false; }
    if (K == 0 && records) { set_error("%s == 0 is the count-only form: the %s array must be NULL", what, records_what); return false; }
    return true;
}

// What every entry point checks first, in this order: the handle, n and the arrays the caller says are missing (`missing`: a required
// array is null), then the kind's own argument rule (it sets its message).  Neither touches the handle's contents.
template <class Rule>
static int walk_args(const gnxr_scene *s, int64_t n, bool missing, Rule rule) {
    if (!s || n < 0 || missing) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    return rule() ? GNXR_OK : GNXR_ERR_INVALID;
}

// An entry point on device memory: walk_args, nothing to do for n == 0, then every array on a multiple of its align[] bytes (before the
// handle is looked at), the copy of the scene that holds them (DeviceCall) and the walk on the caller's stream.
template <class Kind, class Rule, int N>
static int walk_device(const char *name, gnxr_scene *s, int64_t n, bool missing, Rule rule, const QueryArg (&args)[N], const unsigned (&align)[N], const Kind &q,
                       void *hip_stream) {
    if (int rc = walk_args(s, n, missing, rule)) return rc;
    if (n == 0) return GNXR_OK;
    if (int rc = check_aligned(name, args, align, N)) return rc;
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    return walk_launch(call.r, query_device_scene(call.r), q, n, (hipStream_t)hip_stream);
}

// One array of an entry point on host arrays: `in` is uploaded (nullptr: device memory is only allocated), `out` receives the device's
// bytes after the walk (nullptr: nothing comes back); bytes == 0: the array is absent and the kind sees nullptr
struct HostArray { const void *in; void *out; size_t bytes; };

// An entry point on host arrays: walk_args, nothing to do for n == 0, then copy in, the device call's walk on the null stream, copy out.
// make(d): the kind over the device copies d[0 .. N) of the arrays.
template <class Rule, int N, class Make>
static int walk_host(gnxr_scene *s, int64_t n, bool missing, Rule rule, const HostArray (&arrays)[N], Make make) {
    if (int rc = walk_args(s, n, missing, rule)) return rc;
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<char> bufs[N];
    char *d[N];
    for (int i = 0; i < N; ++i) {
        if (arrays[i].bytes == 0) { d[i] = nullptr; continue; }
        if (int rc = arrays[i].in ? bufs[i].upload((const char *)arrays[i].in, arrays[i].bytes) : bufs[i].alloc(arrays[i].bytes)) return rc;
        d[i] = bufs[i].p;
    }
    if (int rc = walk_launch(s, query_device_scene(s), make(d), n, nullptr)) return rc;
    for (int i = 0; i < N; ++i)
        if (arrays[i].out && arrays[i].bytes) HIP_TRY(hipMemcpy(arrays[i].out, d[i], arrays[i].bytes, hipMemcpyDeviceToHost));
    return GNXR_OK;
}
