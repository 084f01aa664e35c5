// api_allhits.hip.h -- all-hits ray queries (allhits_kernel.hip.h): gnxr_trace_all_device on device memory, its counting form for the
// measurement, and gnxr_trace_all for host arrays.  This file holds the entry points' signatures, their array and alignment tables,
// the rule for max_hits and the kernel selection; how the walk is run -- checks, chunks, launches, copies -- is api_walk.hip.h's.  Part
// of api.hip's translation unit.
#pragma once

// work: nullptr, or three device words the counting instantiation adds nodes visited, own-box tests and triangle tests to
struct AllHitsWalk {
    typedef AllHitsArrays Arrays;
    typedef int Spill;
    static constexpr bool kBinnable = false;   // rays are walked in caller order
    const gnxr_ray *rays;
    int32_t K;
    gnxr_ray_hit *hits;
    int32_t *counts;
    unsigned long long *work;
    size_t entry_bytes() const { return sizeof(int); }
    int lds_levels() const { return Knobs::allhits_lds_levels(); }
    Arrays at(long long base) const { return {reinterpret_cast<const float4 *>(rays + base), K > 0 ? reinterpret_cast<float4 *>(hits + base * K) : nullptr, counts + base, K}; }
    auto kernel(bool wide) const {   // [wide][K > 0: a list is kept][counting]
        static constexpr decltype(&k_all_hits<true, true, true>) k[2][2][2] = {{{k_all_hits<false, false, false>, k_all_hits<false, false, true>},
                                                                                {k_all_hits<false, true, false>, k_all_hits<false, true, true>}},
                                                                               {{k_all_hits<true, false, false>, k_all_hits<true, false, true>},
                                                                                {k_all_hits<true, true, false>, k_all_hits<true, true, true>}}};
        return k[wide][K > 0][work != nullptr];
    }
};

static int trace_all_device(const char *name, gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, uint64_t *d_work,
                            bool counted, void *hip_stream) {
    // two dwordx4 loads per ray, one dwordx4 per record
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_hits, (size_t)n * (size_t)max_hits * sizeof(gnxr_ray_hit), "d_hits"},
                             {d_counts, (size_t)n * sizeof(int32_t), "d_counts"}, {d_work, 3 * sizeof(uint64_t), "d_work"}};
    const unsigned align[] = {16, 16, 4, 8};
    return walk_device(name, s, n, (n > 0 && (!d_rays || !d_counts || (max_hits > 0 && !d_hits))) || (counted && !d_work),
                       [&] { return walk_list_ok("max_hits", max_hits, 0, GNXR_ALL_HITS_MAX, "", d_hits, "hits"); }, args, align,
                       AllHitsWalk{d_rays, max_hits, d_hits, d_counts, reinterpret_cast<unsigned long long *>(d_work)}, hip_stream);
}

extern "C" {

int gnxr_trace_all_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, void *hip_stream) {
    return trace_all_device("gnxr_trace_all_device", s, d_rays, n, max_hits, d_hits, d_counts, nullptr, false, hip_stream);
}
int gnxr_trace_all_counted_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts, uint64_t *d_work,
                                  void *hip_stream) {
    return trace_all_device("gnxr_trace_all_counted_device", s, d_rays, n, max_hits, d_hits, d_counts, d_work, true, hip_stream);
}

int gnxr_trace_all(gnxr_scene *s, const gnxr_ray *rays, int64_t n, int32_t max_hits, gnxr_ray_hit *hits, int32_t *counts) {
    const size_t list_bytes = max_hits > 0 ? (size_t)n * (size_t)max_hits * sizeof(gnxr_ray_hit) : 0;
    const HostArray arrays[] = {{rays, nullptr, (size_t)n * sizeof(gnxr_ray)}, {nullptr, hits, list_bytes}, {nullptr, counts, (size_t)n * sizeof(int32_t)}};
    return walk_host(s, n, n > 0 && (!rays || !counts || (max_hits > 0 && !hits)), [&] { return walk_list_ok("max_hits", max_hits, 0, GNXR_ALL_HITS_MAX, "", hits, "hits"); },
                     arrays, [&](char *const *d) {
        return AllHitsWalk{reinterpret_cast<const gnxr_ray *>(d[0]), max_hits, reinterpret_cast<gnxr_ray_hit *>(d[1]), reinterpret_cast<int32_t *>(d[2]), nullptr};
    });
}

}  // extern "C"
