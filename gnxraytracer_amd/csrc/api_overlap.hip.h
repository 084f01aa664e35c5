// api_overlap.hip.h -- box overlap queries (overlap_kernel.hip.h): gnxr_overlap_box_device on device memory, its counting form for the
// measurement, and gnxr_overlap_box for host arrays.  This file holds the entry points' signatures, their array and alignment tables,
// the rule for max_prims and the offsets, and the kernel selection; how the walk is run -- checks, chunks, launches, copies -- is
// api_walk.hip.h's.  Part of api.hip's translation unit.
#pragma once

// work: nullptr, or two device words the counting instantiation adds nodes visited and triangles tested to
struct OverlapWalk {
    typedef OverlapArrays Arrays;
    typedef int Spill;
    static constexpr bool kBinnable = false;   // boxes are walked in caller order
    const gnxr_box_query *boxes;
    int32_t K;                 // rows mode; -1 in CSR mode
    const int64_t *offsets;    // CSR mode, else nullptr
    int32_t *prims;
    int32_t *counts;
    unsigned long long *work;
    bool lists() const { return offsets != nullptr || K > 0; }
    size_t entry_bytes() const { return sizeof(int); }
    int lds_levels() const { return Knobs::overlap_lds_levels(); }
    Arrays at(long long base) const {   // CSR offsets index the whole of prims, so only the offsets move with the chunk
        return {reinterpret_cast<const float4 *>(boxes + base), offsets ? reinterpret_cast<const long long *>(offsets + base) : nullptr,
                offsets ? prims : K > 0 ? prims + base * K : nullptr, counts + base, offsets ? 0 : K};
    }
    auto kernel(bool wide) const {   // [wide][rows are kept][counting]
        static constexpr decltype(&k_overlap_box<true, true, true>) k[2][2][2] = {{{k_overlap_box<false, false, false>, k_overlap_box<false, false, true>},
                                                                                   {k_overlap_box<false, true, false>, k_overlap_box<false, true, true>}},
                                                                                  {{k_overlap_box<true, false, false>, k_overlap_box<true, false, true>},
                                                                                   {k_overlap_box<true, true, false>, k_overlap_box<true, true, true>}}};
        return k[wide][lists()][work != nullptr];
    }
};

// the row layout: max_prims rows, or offsets with max_prims == -1
static bool overlap_args_ok(int32_t max_prims, const void *offsets, const void *prims) {
    if (offsets) {
        if (max_prims != -1) { set_error("max_prims = %d with offsets: the CSR form takes max_prims == -1", max_prims); return false; }
        if (!prims) { set_error("the CSR form writes rows: the prims array must not be NULL"); return false; }
        return true;
    }
    if (max_prims == -1) { set_error("max_prims == -1 is the CSR form: the offsets array must be given"); return false; }
    return walk_list_ok("max_prims", max_prims, 0, GNXR_OVERLAP_MAX, "", prims, "prims");
}

static int overlap_box_device(const char *name, gnxr_scene *s, const gnxr_box_query *d_boxes, int64_t n, int32_t max_prims, const int64_t *d_offsets, int32_t *d_prims,
                              int32_t *d_counts, uint64_t *d_work, bool counted, void *hip_stream) {
    // two dwordx4 loads per box, dword rows; the extent of CSR rows is on the device, so only the start of d_prims is looked at
    const QueryArg args[] = {{d_boxes, (size_t)n * sizeof(gnxr_box_query), "d_boxes"}, {d_offsets, ((size_t)n + 1) * sizeof(int64_t), "d_offsets"},
                             {d_prims, max_prims > 0 ? (size_t)n * (size_t)max_prims * sizeof(int32_t) : 0, "d_prims"}, {d_counts, (size_t)n * sizeof(int32_t), "d_counts"},
                             {d_work, 2 * sizeof(uint64_t), "d_work"}};
    const unsigned align[] = {16, 8, 4, 4, 8};
    return walk_device(name, s, n, (n > 0 && (!d_boxes || !d_counts || (max_prims > 0 && !d_prims))) || (counted && !d_work),
                       [&] { return overlap_args_ok(max_prims, d_offsets, d_prims); }, args, align,
                       OverlapWalk{d_boxes, max_prims, d_offsets, d_prims, d_counts, reinterpret_cast<unsigned long long *>(d_work)}, hip_stream);
}

extern "C" {

int gnxr_overlap_box_device(gnxr_scene *s, const gnxr_box_query *d_boxes, int64_t n, int32_t max_prims, const int64_t *d_offsets, int32_t *d_prims, int32_t *d_counts,
                            void *hip_stream) {
    return overlap_box_device("gnxr_overlap_box_device", s, d_boxes, n, max_prims, d_offsets, d_prims, d_counts, nullptr, false, hip_stream);
}
int gnxr_overlap_box_counted_device(gnxr_scene *s, const gnxr_box_query *d_boxes, int64_t n, int32_t max_prims, const int64_t *d_offsets, int32_t *d_prims, int32_t *d_counts,
                                    uint64_t *d_work, void *hip_stream) {
    return overlap_box_device("gnxr_overlap_box_counted_device", s, d_boxes, n, max_prims, d_offsets, d_prims, d_counts, d_work, true, hip_stream);
}

int gnxr_overlap_box(gnxr_scene *s, const gnxr_box_query *boxes, int64_t n, int32_t max_prims, const int64_t *offsets, int32_t *prims, int32_t *counts) {
    const bool missing = n > 0 && (!boxes || !counts || (max_prims > 0 && !prims));
    size_t list_bytes = max_prims > 0 ? (size_t)n * (size_t)max_prims * sizeof(int32_t) : 0;
    // host offsets can be read: the device copy of prims spans [0, offsets[n]), so the rows must lie inside it
    const auto rule = [&] {
        if (!overlap_args_ok(max_prims, offsets, prims)) return false;
        if (!offsets) return true;
        if (offsets[0] < 0) { set_error("offsets[0] = %lld is negative", (long long)offsets[0]); return false; }
        for (int64_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) { set_error("offsets[%lld] = %lld is below offsets[%lld] = %lld: the offsets must ascend", (long long)(i + 1), (long long)offsets[i + 1], (long long)i, (long long)offsets[i]); return false; }
        list_bytes = (size_t)offsets[n] * sizeof(int32_t);
        return true;
    };
    if (int rc = walk_args(s, n, missing, rule)) return rc;   // here, before the table: the rule sizes the CSR rows
    const bool csr = offsets != nullptr;
    // CSR: prims goes up as well, so that what lies below offsets[0] comes back as it was
    const HostArray arrays[] = {{boxes, nullptr, (size_t)n * sizeof(gnxr_box_query)}, {offsets, nullptr, csr ? ((size_t)n + 1) * sizeof(int64_t) : 0},
                                {csr ? prims : nullptr, prims, list_bytes}, {nullptr, counts, (size_t)n * sizeof(int32_t)}};
    return walk_host(s, n, false, [] { return true; }, arrays, [&](char *const *d) {
        // a CSR call whose rows are all empty has no prims on the device: rows mode's count-only form gives the same counts
        const bool lists = d[2] != nullptr;
        return OverlapWalk{reinterpret_cast<const gnxr_box_query *>(d[0]), lists ? max_prims : 0, lists && csr ? reinterpret_cast<const int64_t *>(d[1]) : nullptr,
                           reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[3]), nullptr};
    });
}

}  // extern "C"
