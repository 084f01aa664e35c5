// api_closest.hip.h -- closest-point queries (closest_kernel.hip.h): gnxr_closest_point_device on device memory, its counting form for
// the measurement, and gnxr_closest_point for host arrays.  Part of api.hip's translation unit (after api_query.hip.h: the front end is
// trace_device's -- the same checks, DeviceCall, query_device_scene, scratch from the stream-ordered allocator on the caller's stream).
#pragma once

// queries of one binned launch: bounds the sort's scratch (24 bytes per query) at 96 MB whatever n is, and keeps its indices in 32 bits
static const long long kClosestBinChunk = 1ll << 22;

// The Morton binning of a batch of point queries (closest_kernel.hip.h: k_closest_keys, then three passes of the HLBVH stage's radix sort
// over (key, index)), shared by closest_launch and near_launch.  reserve() takes the sort's arrays for launches of at most `most` queries
// from the stream-ordered allocator; sort() queues the key and the passes for the m queries at `queries` and returns their indices in
// Morton order (valid until the next sort()).  The key orders the work and nothing more.
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

// The walk over n queries on `st`.  d_counts: nullptr, or two device words the counting instantiation adds nodes visited and triangles
// tested to.  From Knobs::closest_bin_min() queries on they are binned by Morton key first (QueryBinning), a chunk at a time;
// below, one launch walks them in caller order (queries are indexed in 64 bits, a thread's spill column by its number in the grid).
static int closest_launch(gnxr_scene *r, const DScene &sc, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, unsigned long long *d_counts, hipStream_t st) {
    if (r->cs.n_triangles == 0) {
        hipLaunchKernelGGL(k_closest_none, dim3(grid_for(n)), dim3(kBlock), 0, st, reinterpret_cast<float4 *>(d_out), (long long)n);
        HIP_TRY(hipGetLastError());
        return GNXR_OK;
    }
    const bool binned = n >= Knobs::closest_bin_min();
    const long long per_launch = binned ? kClosestBinChunk : (long long)n;
    const long long most = std::min<long long>(n, per_launch);   // queries of one launch
    WalkLaunch w;
    if (int rc = w.plan(r, sizeof(uint2), Knobs::closest_lds_levels(), most, st)) return rc;
    QueryBinning bins;
    if (binned) { if (int rc = bins.reserve(most, st)) return rc; }
    for (long long base = 0; base < n; base += per_launch) {
        const long long cnt = std::min<long long>(n - base, per_launch);
        ClosestArrays qa;
        qa.queries = reinterpret_cast<const float4 *>(d_queries + base);
        qa.out = reinterpret_cast<float4 *>(d_out + base);
        const uint32_t *order = binned ? bins.sort(sc, qa.queries, (int)cnt, st) : nullptr;
#define GX_CLOSEST(W, C) hipLaunchKernelGGL((k_closest_point<W, C>), dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, order, (long long)cnt, w.lds_entries, w.entries, \
                                            (uint2 *)w.spill, d_counts)
        if (d_counts) { if (w.wide) GX_CLOSEST(true, true); else GX_CLOSEST(false, true); }
        else { if (w.wide) GX_CLOSEST(true, false); else GX_CLOSEST(false, false); }
#undef GX_CLOSEST
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

static int closest_point_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_counts, bool counted, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_queries || !d_out)) || (counted && !d_counts)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_queries & 15u) != 0) { set_error("d_queries is not 16-byte aligned (one dwordx4 load per query)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_out & 15u) != 0) { set_error("d_out is not 16-byte aligned (two dwordx4 stores per record)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_counts & 7u) != 0) { set_error("d_counts is not 8-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_queries, (size_t)n * sizeof(gnxr_point_query), "d_queries"}, {d_out, (size_t)n * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_counts, 2 * sizeof(uint64_t), "d_counts"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    return closest_launch(r, query_device_scene(r), d_queries, n, d_out, reinterpret_cast<unsigned long long *>(d_counts), (hipStream_t)hip_stream);
}

extern "C" {

int gnxr_closest_point_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, void *hip_stream) {
    return closest_point_device(s, d_queries, n, d_out, nullptr, false, hip_stream);
}
int gnxr_closest_point_counted_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_counts, void *hip_stream) {
    return closest_point_device(s, d_queries, n, d_out, d_counts, true, hip_stream);
}

// host arrays: copy in, the device call's walk on the null stream, copy out
int gnxr_closest_point(gnxr_scene *s, const gnxr_point_query *queries, int64_t n, struct gnxr_closest_point *out) {
    if (!s || !queries || !out || n < 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<gnxr_point_query> dq;
    DevBuf<struct gnxr_closest_point> dout;
    int rc;
    if ((rc = dq.upload(queries, (size_t)n)) || (rc = dout.alloc((size_t)n))) return rc;
    if ((rc = closest_launch(s, query_device_scene(s), dq.p, n, dout.p, nullptr, nullptr)) != GNXR_OK) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(struct gnxr_closest_point), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"
