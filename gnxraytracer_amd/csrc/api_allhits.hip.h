// api_allhits.hip.h -- all-hits ray queries (allhits_kernel.hip.h): gnxr_trace_all_device on device memory, its counting form for the
// measurement, and gnxr_trace_all for host arrays.  Part of api.hip's translation unit (after api_closest.hip.h: the front end is
// trace_device's and closest_point_device's -- the same checks, DeviceCall, query_device_scene, scratch from the stream-ordered
// allocator on the caller's stream).
#pragma once

// rays of one launch: the kernel indexes rays and slots in 64 bits, a thread's spill column by its number in the grid; the cut keeps
// n * max_hits of one launch far inside them
static const long long kAllHitsLaunchMax = 1ll << 30;

// The walk over n rays on `st`.  d_work: nullptr, or three device words the counting instantiation adds nodes visited, own-box tests and
// triangle tests to.
static int all_hits_launch(gnxr_scene *r, const DScene &sc, const gnxr_ray *d_rays, int64_t n, int32_t K, gnxr_ray_hit *d_hits, int32_t *d_counts, unsigned long long *d_work,
                           hipStream_t st) {
    if (r->cs.n_triangles == 0) {
        hipLaunchKernelGGL(k_all_hits_none, dim3(grid_for(n)), dim3(kBlock), 0, st, reinterpret_cast<float4 *>(d_hits), d_counts, (long long)n, (int)K);
        HIP_TRY(hipGetLastError());
        return GNXR_OK;
    }
    WalkLaunch w;
    if (int rc = w.plan(r, sizeof(int), Knobs::allhits_lds_levels(), std::min<long long>(n, kAllHitsLaunchMax), st)) return rc;
    for (long long base = 0; base < n; base += kAllHitsLaunchMax) {
        const long long cnt = std::min<long long>(n - base, kAllHitsLaunchMax);
        AllHitsArrays qa;
        qa.rays = reinterpret_cast<const float4 *>(d_rays + base);
        qa.hits = K > 0 ? reinterpret_cast<float4 *>(d_hits + base * K) : nullptr;
        qa.counts = d_counts + base;
        qa.K = K;
#define GX_ALLHITS(W, L, C) hipLaunchKernelGGL((k_all_hits<W, L, C>), dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, (long long)cnt, w.lds_entries, w.entries, \
                                               (int *)w.spill, d_work)
#define GX_ALLHITS_WL(C) do { if (w.wide) { if (K > 0) GX_ALLHITS(true, true, C); else GX_ALLHITS(true, false, C); } \
                              else { if (K > 0) GX_ALLHITS(false, true, C); else GX_ALLHITS(false, false, C); } } while (0)
        if (d_work) GX_ALLHITS_WL(true);
        else GX_ALLHITS_WL(false);
#undef GX_ALLHITS_WL
#undef GX_ALLHITS
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

static bool all_hits_max_ok(int32_t max_hits, const void *hits) {
    if (max_hits < 0 || max_hits > GNXR_ALL_HITS_MAX) { set_error("max_hits = %d is outside [0, %d]", max_hits, GNXR_ALL_HITS_MAX); return false; }
    if (max_hits == 0 && hits) { set_error("max_hits == 0 is the count-only form: the hits array must be NULL"); return false; }
    return true;
}

static int trace_all_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, uint64_t *d_work, bool counted,
                            void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_rays || !d_counts || (max_hits > 0 && !d_hits))) || (counted && !d_work)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (!all_hits_max_ok(max_hits, d_hits)) return GNXR_ERR_INVALID;
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_rays & 15u) != 0) { set_error("d_rays is not 16-byte aligned (two dwordx4 loads per ray)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_hits & 15u) != 0) { set_error("d_hits is not 16-byte aligned (one dwordx4 per record)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_counts & 3u) != 0) { set_error("d_counts is not 4-byte aligned"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_work & 7u) != 0) { set_error("d_work is not 8-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_hits, (size_t)n * (size_t)max_hits * sizeof(gnxr_ray_hit), "d_hits"},
                             {d_counts, (size_t)n * sizeof(int32_t), "d_counts"}, {d_work, 3 * sizeof(uint64_t), "d_work"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    return all_hits_launch(r, query_device_scene(r), d_rays, n, max_hits, d_hits, d_counts, reinterpret_cast<unsigned long long *>(d_work), (hipStream_t)hip_stream);
}

extern "C" {

int gnxr_trace_all_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, void *hip_stream) {
    return trace_all_device(s, d_rays, n, max_hits, d_hits, d_counts, nullptr, false, hip_stream);
}
int gnxr_trace_all_counted_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, uint64_t *d_work,
                                  void *hip_stream) {
    return trace_all_device(s, d_rays, n, max_hits, d_hits, d_counts, d_work, true, hip_stream);
}

// host arrays: copy in, the device call's walk on the null stream, copy out
int gnxr_trace_all(gnxr_scene *s, const gnxr_ray *rays, int64_t n, int32_t max_hits, gnxr_ray_hit *hits, int32_t *counts) {
    if (!s || n < 0 || (n > 0 && (!rays || !counts || (max_hits > 0 && !hits)))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (!all_hits_max_ok(max_hits, hits)) return GNXR_ERR_INVALID;
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<gnxr_ray> dr;
    DevBuf<gnxr_ray_hit> dh;
    DevBuf<int32_t> dc;
    int rc;
    if ((rc = dr.upload(rays, (size_t)n)) || (rc = dc.alloc((size_t)n)) || (max_hits > 0 && (rc = dh.alloc((size_t)n * (size_t)max_hits)))) return rc;
    if ((rc = all_hits_launch(s, query_device_scene(s), dr.p, n, max_hits, max_hits > 0 ? dh.p : nullptr, dc.p, nullptr, nullptr)) != GNXR_OK) return rc;
    if (max_hits > 0) HIP_TRY(hipMemcpy(hits, dh.p, (size_t)n * (size_t)max_hits * sizeof(gnxr_ray_hit), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, dc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"
