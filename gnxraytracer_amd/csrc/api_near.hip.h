// api_near.hip.h -- neighbour queries (near_kernel.hip.h): gnxr_near_device on device memory, its counting form for the measurement, and
// gnxr_near for host arrays.  Part of api.hip's translation unit (after api_allhits.hip.h: the front end is its siblings' -- the same
// checks, DeviceCall, query_device_scene, WalkLaunch, scratch from the stream-ordered allocator on the caller's stream -- and the Morton
// binning is closest_launch's, QueryBinning).
#pragma once

// queries of one launch in caller order: the kernel indexes queries and slots in 64 bits, a thread's spill column by its number in the
// grid; the cut keeps n * max_near of one launch far inside them.  A binned launch takes kClosestBinChunk.
static const long long kNearLaunchMax = 1ll << 30;

// The walk over n queries on `st`.  d_work: nullptr, or two device words the counting instantiation adds nodes visited and triangles
// tested to.  From Knobs::closest_bin_min() queries on they are binned by Morton key first, a chunk at a time, as in closest_launch.
static int near_launch(gnxr_scene *r, const DScene &sc, const gnxr_point_query *d_queries, int64_t n, int32_t K, uint32_t flags, struct gnxr_closest_point *d_out,
                       int32_t *d_counts, unsigned long long *d_work, hipStream_t st) {
    if (r->cs.n_triangles == 0) {
        hipLaunchKernelGGL(k_near_none, dim3(grid_for(n)), dim3(kBlock), 0, st, reinterpret_cast<float4 *>(d_out), d_counts, (long long)n, (int)K);
        HIP_TRY(hipGetLastError());
        return GNXR_OK;
    }
    const bool nearest = (flags & GNXR_NEAR_NEAREST) != 0;
    const bool binned = n >= Knobs::closest_bin_min();
    const long long per_launch = binned ? kClosestBinChunk : kNearLaunchMax;
    const long long most = std::min<long long>(n, per_launch);   // queries of one launch
    WalkLaunch w;
    if (int rc = w.plan(r, nearest ? sizeof(uint2) : sizeof(int), Knobs::near_lds_levels(), most, st)) return rc;
    QueryBinning bins;
    if (binned) { if (int rc = bins.reserve(most, st)) return rc; }
    for (long long base = 0; base < n; base += per_launch) {
        const long long cnt = std::min<long long>(n - base, per_launch);
        NearArrays qa;
        qa.queries = reinterpret_cast<const float4 *>(d_queries + base);
        qa.out = K > 0 ? reinterpret_cast<float4 *>(d_out + base * K) : nullptr;
        qa.counts = d_counts + base;
        qa.K = K;
        const uint32_t *order = binned ? bins.sort(sc, qa.queries, (int)cnt, st) : nullptr;
#define GX_NEAR(W, N, L, C) hipLaunchKernelGGL((k_near<W, N, L, C>), dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, order, (long long)cnt, w.lds_entries, w.entries, \
                                               w.spill, d_work)
#define GX_NEAR_W(W, C) do { if (nearest) GX_NEAR(W, true, true, C); else if (K > 0) GX_NEAR(W, false, true, C); else GX_NEAR(W, false, false, C); } while (0)
        if (d_work) { if (w.wide) GX_NEAR_W(true, true); else GX_NEAR_W(false, true); }
        else { if (w.wide) GX_NEAR_W(true, false); else GX_NEAR_W(false, false); }
#undef GX_NEAR_W
#undef GX_NEAR
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

// the mode and its K, and the records that go with it
static bool near_args_ok(int32_t max_near, uint32_t flags, const void *out) {
    if (flags & ~(uint32_t)GNXR_NEAR_NEAREST) { set_error("flags = 0x%x: only GNXR_NEAR_ALL (0) and GNXR_NEAR_NEAREST (1) are defined", flags); return false; }
    const int lowest = (flags & GNXR_NEAR_NEAREST) ? 1 : 0;
    if (max_near < lowest || max_near > GNXR_NEAR_MAX) {
        set_error("max_near = %d is outside [%d, %d] of %s", max_near, lowest, GNXR_NEAR_MAX, lowest ? "GNXR_NEAR_NEAREST" : "GNXR_NEAR_ALL");
        return false;
    }
    if (max_near == 0 && out) { set_error("max_near == 0 is the count-only form: the record array must be NULL"); return false; }
    return true;
}

static int near_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out, int32_t *d_counts,
                       uint64_t *d_work, bool counted, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_queries || !d_counts || (max_near > 0 && !d_out))) || (counted && !d_work)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (!near_args_ok(max_near, flags, d_out)) return GNXR_ERR_INVALID;
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_queries & 15u) != 0) { set_error("d_queries is not 16-byte aligned (one dwordx4 load per query)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_out & 15u) != 0) { set_error("d_out is not 16-byte aligned (two dwordx4 stores per record)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_counts & 3u) != 0) { set_error("d_counts is not 4-byte aligned"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_work & 7u) != 0) { set_error("d_work is not 8-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_queries, (size_t)n * sizeof(gnxr_point_query), "d_queries"},
                             {d_out, (size_t)n * (size_t)max_near * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_counts, (size_t)n * sizeof(int32_t), "d_counts"}, {d_work, 2 * sizeof(uint64_t), "d_work"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    return near_launch(r, query_device_scene(r), d_queries, n, max_near, flags, d_out, d_counts, reinterpret_cast<unsigned long long *>(d_work), (hipStream_t)hip_stream);
}

extern "C" {

int gnxr_near_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out, int32_t *d_counts,
                     void *hip_stream) {
    return near_device(s, d_queries, n, max_near, flags, d_out, d_counts, nullptr, false, hip_stream);
}
int gnxr_near_counted_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out,
                             int32_t *d_counts, uint64_t *d_work, void *hip_stream) {
    return near_device(s, d_queries, n, max_near, flags, d_out, d_counts, d_work, true, hip_stream);
}

// host arrays: copy in, the device call's walk on the null stream, copy out
int gnxr_near(gnxr_scene *s, const gnxr_point_query *queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *out, int32_t *counts) {
    if (!s || n < 0 || (n > 0 && (!queries || !counts || (max_near > 0 && !out)))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (!near_args_ok(max_near, flags, out)) return GNXR_ERR_INVALID;
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<gnxr_point_query> dq;
    DevBuf<struct gnxr_closest_point> dout;
    DevBuf<int32_t> dc;
    int rc;
    if ((rc = dq.upload(queries, (size_t)n)) || (rc = dc.alloc((size_t)n)) || (max_near > 0 && (rc = dout.alloc((size_t)n * (size_t)max_near)))) return rc;
    if ((rc = near_launch(s, query_device_scene(s), dq.p, n, max_near, flags, max_near > 0 ? dout.p : nullptr, dc.p, nullptr, nullptr)) != GNXR_OK) return rc;
    if (max_near > 0) HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * (size_t)max_near * sizeof(struct gnxr_closest_point), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, dc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"
