// api_closest.hip.h -- closest-point queries (closest_kernel.hip.h): gnxr_closest_point_device on device memory, its counting form for
// the measurement, and gnxr_closest_point for host arrays.  This file holds the entry points' signatures, their array and alignment
// tables and the kernel selection; how the walk is run -- checks, binning, chunks, launches, copies -- is api_walk.hip.h's.  Part of
// api.hip's translation unit.
#pragma once

// work: nullptr, or two device words the counting instantiation adds nodes visited and triangles tested to
struct ClosestWalk {
    typedef ClosestArrays Arrays;
    typedef uint2 Spill;
    static constexpr bool kBinnable = true;
    const gnxr_point_query *queries;
    struct gnxr_closest_point *out;
    unsigned long long *work;
    size_t entry_bytes() const { return sizeof(uint2); }
    int lds_levels() const { return Knobs::closest_lds_levels(); }
    Arrays at(long long base) const { return {reinterpret_cast<const float4 *>(queries + base), reinterpret_cast<float4 *>(out + base)}; }
    auto kernel(bool wide) const {
        static constexpr decltype(&k_closest_point<true, true>) k[2][2] = {{k_closest_point<false, false>, k_closest_point<false, true>},
                                                                           {k_closest_point<true, false>, k_closest_point<true, true>}};
        return k[wide][work != nullptr];
    }
};

static int closest_point_device(const char *name, gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_counts, bool counted,
                                void *hip_stream) {
    // one dwordx4 load per query, two dwordx4 stores per record
    const QueryArg args[] = {{d_queries, (size_t)n * sizeof(gnxr_point_query), "d_queries"}, {d_out, (size_t)n * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_counts, 2 * sizeof(uint64_t), "d_counts"}};
    const unsigned align[] = {16, 16, 8};
    return walk_device(name, s, n, (n > 0 && (!d_queries || !d_out)) || (counted && !d_counts), [] { return true; }, args, align,
                       ClosestWalk{d_queries, d_out, reinterpret_cast<unsigned long long *>(d_counts)}, hip_stream);
}

extern "C" {

int gnxr_closest_point_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, void *hip_stream) {
    return closest_point_device("gnxr_closest_point_device", s, d_queries, n, d_out, nullptr, false, hip_stream);
}
int gnxr_closest_point_counted_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_counts, void *hip_stream) {
    return closest_point_device("gnxr_closest_point_counted_device", s, d_queries, n, d_out, d_counts, true, hip_stream);
}

int gnxr_closest_point(gnxr_scene *s, const gnxr_point_query *queries, int64_t n, struct gnxr_closest_point *out) {
    const HostArray arrays[] = {{queries, nullptr, (size_t)n * sizeof(gnxr_point_query)}, {nullptr, out, (size_t)n * sizeof(struct gnxr_closest_point)}};
    return walk_host(s, n, !queries || !out, [] { return true; }, arrays, [](char *const *d) {
        return ClosestWalk{reinterpret_cast<const gnxr_point_query *>(d[0]), reinterpret_cast<struct gnxr_closest_point *>(d[1]), nullptr};
    });
}

}  // extern "C"
