// api_near.hip.h -- neighbour queries (near_kernel.hip.h): gnxr_near_device on device memory, its counting form for the measurement, and
// gnxr_near for host arrays.  This file holds the entry points' signatures, their array and alignment tables, the rule for flags and
// max_near and the kernel selection; how the walk is run -- checks, binning, chunks, launches, copies -- is api_walk.hip.h's.  Part of
// api.hip's translation unit.
#pragma once

// work: nullptr, or two device words the counting instantiation adds nodes visited and triangles tested to
struct NearWalk {
    typedef NearArrays Arrays;
    typedef void Spill;   // 8-byte entries in the NEAREST mode, 4-byte ones in ALL
    static constexpr bool kBinnable = true;
    const gnxr_point_query *queries;
    int32_t K;
    uint32_t flags;
    struct gnxr_closest_point *out;
    int32_t *counts;
    unsigned long long *work;
    bool nearest() const { return (flags & GNXR_NEAR_NEAREST) != 0; }
    size_t entry_bytes() const { return nearest() ? sizeof(uint2) : sizeof(int); }
    int lds_levels() const { return Knobs::near_lds_levels(); }
    Arrays at(long long base) const { return {reinterpret_cast<const float4 *>(queries + base), K > 0 ? reinterpret_cast<float4 *>(out + base * K) : nullptr, counts + base, K}; }
    auto kernel(bool wide) const {   // [wide][ALL count-only, ALL with a list, NEAREST][counting]
        static constexpr decltype(&k_near<true, true, true, true>) k[2][3][2] = {{{k_near<false, false, false, false>, k_near<false, false, false, true>},
                                                                                  {k_near<false, false, true, false>, k_near<false, false, true, true>},
                                                                                  {k_near<false, true, true, false>, k_near<false, true, true, true>}},
                                                                                 {{k_near<true, false, false, false>, k_near<true, false, false, true>},
                                                                                  {k_near<true, false, true, false>, k_near<true, false, true, true>},
                                                                                  {k_near<true, true, true, false>, k_near<true, true, true, true>}}};
        return k[wide][nearest() ? 2 : K > 0][work != nullptr];
    }
};

// the mode and its K, and the records that go with it
static bool near_args_ok(int32_t max_near, uint32_t flags, const void *out) {
    if (flags & ~(uint32_t)GNXR_NEAR_NEAREST) { set_error("flags = 0x%x: only GNXR_NEAR_ALL (0) and GNXR_NEAR_NEAREST (1) are defined", flags); return false; }
    const bool nearest = (flags & GNXR_NEAR_NEAREST) != 0;
    return walk_list_ok("max_near", max_near, nearest ? 1 : 0, GNXR_NEAR_MAX, nearest ? " of GNXR_NEAR_NEAREST" : " of GNXR_NEAR_ALL", out, "record");
}

static int near_device(const char *name, gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out,
                       int32_t *d_counts, uint64_t *d_work, bool counted, void *hip_stream) {
    // one dwordx4 load per query, two dwordx4 stores per record
    const QueryArg args[] = {{d_queries, (size_t)n * sizeof(gnxr_point_query), "d_queries"},
                             {d_out, (size_t)n * (size_t)max_near * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_counts, (size_t)n * sizeof(int32_t), "d_counts"}, {d_work, 2 * sizeof(uint64_t), "d_work"}};
    const unsigned align[] = {16, 16, 4, 8};
    return walk_device(name, s, n, (n > 0 && (!d_queries || !d_counts || (max_near > 0 && !d_out))) || (counted && !d_work),
                       [&] { return near_args_ok(max_near, flags, d_out); }, args, align,
                       NearWalk{d_queries, max_near, flags, d_out, d_counts, reinterpret_cast<unsigned long long *>(d_work)}, hip_stream);
}

extern "C" {

int gnxr_near_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out, int32_t *d_counts,
                     void *hip_stream) {
    return near_device("gnxr_near_device", s, d_queries, n, max_near, flags, d_out, d_counts, nullptr, false, hip_stream);
}
int gnxr_near_counted_device(gnxr_scene *s, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *d_out,
                             int32_t *d_counts, uint64_t *d_work, void *hip_stream) {
    return near_device("gnxr_near_counted_device", s, d_queries, n, max_near, flags, d_out, d_counts, d_work, true, hip_stream);
}

int gnxr_near(gnxr_scene *s, const gnxr_point_query *queries, int64_t n, int32_t max_near, uint32_t flags, struct gnxr_closest_point *out, int32_t *counts) {
    const size_t list_bytes = max_near > 0 ? (size_t)n * (size_t)max_near * sizeof(struct gnxr_closest_point) : 0;
    const HostArray arrays[] = {{queries, nullptr, (size_t)n * sizeof(gnxr_point_query)}, {nullptr, out, list_bytes}, {nullptr, counts, (size_t)n * sizeof(int32_t)}};
    return walk_host(s, n, n > 0 && (!queries || !counts || (max_near > 0 && !out)), [&] { return near_args_ok(max_near, flags, out); }, arrays, [&](char *const *d) {
        return NearWalk{reinterpret_cast<const gnxr_point_query *>(d[0]), max_near, flags, reinterpret_cast<struct gnxr_closest_point *>(d[1]), reinterpret_cast<int32_t *>(d[2]),
                        nullptr};
    });
}

}  // extern "C"
