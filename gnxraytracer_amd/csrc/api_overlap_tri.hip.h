// api_overlap_tri.hip.h -- triangle overlap queries (overlap_tri_kernel.hip.h): gnxr_overlap_tri_device on device memory, its counting
// form for the measurement, and gnxr_overlap_tri for host arrays.  This file holds the entry points' signatures, their array and
// alignment tables, the rule for the flags and the kernel selection; the rule for max_prims and the offsets is api_overlap.hip.h's
// (overlap_args_ok), and how the walk is run -- checks, chunks, launches, copies -- is api_walk.hip.h's.  Part of api.hip's translation
// unit (after api_overlap.hip.h).
#pragma once

// work: nullptr, or two device words the counting instantiation adds nodes visited and triangles tested to
struct OverlapTriWalk {
    typedef OverlapTriArrays Arrays;
    typedef int Spill;
    static constexpr bool kBinnable = false;   // 48-byte records are walked in caller order; SELF walks in leaf order
    const gnxr_tri_query *tris;   // nullptr with GNXR_OVERLAP_TRI_SELF
    uint32_t flags;
    int32_t K;                 // rows mode; -1 in CSR mode
    const int64_t *offsets;    // CSR mode, else nullptr
    int32_t *prims;
    int32_t *counts;
    unsigned long long *work;
    bool self() const { return (flags & GNXR_OVERLAP_TRI_SELF) != 0; }
    bool lists() const { return offsets != nullptr || K > 0; }
    size_t entry_bytes() const { return sizeof(int); }
    int lds_levels() const { return Knobs::overlap_lds_levels(); }
    Arrays at(long long base) const {
        const unsigned skip = (flags & GNXR_OVERLAP_TRI_SKIP_SHARED) ? 1u : 0u;
        // SELF: rows, offsets and counts are indexed by authoring index, so nothing but the first triangle moves with the chunk
        if (self()) return {nullptr, reinterpret_cast<const long long *>(offsets), lists() ? prims : nullptr, counts, offsets ? 0 : K, 1u, base};
        // CSR offsets index the whole of prims, so only the offsets move with the chunk
        return {reinterpret_cast<const float4 *>(tris + base), offsets ? reinterpret_cast<const long long *>(offsets + base) : nullptr,
                offsets ? prims : K > 0 ? prims + base * K : nullptr, counts + base, offsets ? 0 : K, skip, 0};
    }
    auto kernel(bool wide) const {   // [wide][rows are kept][counting][self]
        typedef decltype(&k_overlap_tri<true, true, true, true>) Kernel;
        static constexpr Kernel k[2][2][2][2] = {
            {{{k_overlap_tri<false, false, false, false>, k_overlap_tri<false, false, false, true>}, {k_overlap_tri<false, false, true, false>, k_overlap_tri<false, false, true, true>}},
             {{k_overlap_tri<false, true, false, false>, k_overlap_tri<false, true, false, true>}, {k_overlap_tri<false, true, true, false>, k_overlap_tri<false, true, true, true>}}},
            {{{k_overlap_tri<true, false, false, false>, k_overlap_tri<true, false, false, true>}, {k_overlap_tri<true, false, true, false>, k_overlap_tri<true, false, true, true>}},
             {{k_overlap_tri<true, true, false, false>, k_overlap_tri<true, true, false, true>}, {k_overlap_tri<true, true, true, false>, k_overlap_tri<true, true, true, true>}}}};
        return k[wide][lists()][work != nullptr][self()];
    }
};

// The flags, then the row layout.  Runs after the handle and the arrays were found present; the SELF count is the one thing read from the
// handle, and only once everything that can be refused without it has been.
static bool overlap_tri_args_ok(const gnxr_scene *s, const void *tris, int64_t n, uint32_t flags, int32_t max_prims, const void *offsets, const void *prims) {
    if (flags & ~(GNXR_OVERLAP_TRI_SKIP_SHARED | GNXR_OVERLAP_TRI_SELF)) { set_error("flags = 0x%x: unknown bits (GNXR_OVERLAP_TRI_SKIP_SHARED | GNXR_OVERLAP_TRI_SELF)", flags); return false; }
    const bool self = (flags & GNXR_OVERLAP_TRI_SELF) != 0;
    if (self && tris) { set_error("GNXR_OVERLAP_TRI_SELF takes the scene's own triangles as the queries: the triangle array must be NULL"); return false; }
    if (!overlap_args_ok(max_prims, offsets, prims)) return false;
    if (self && n != s->cs.n_triangles) {
        set_error("GNXR_OVERLAP_TRI_SELF: n = %lld, but the scene holds %d triangles (query i is the triangle with authoring index i)", (long long)n, s->cs.n_triangles);
        return false;
    }
    return true;
}

// a required array is null (with SELF the queries are the scene's)
static bool overlap_tri_missing(const void *tris, int64_t n, uint32_t flags, int32_t max_prims, const void *prims, const void *counts) {
    return n > 0 && ((!tris && !(flags & GNXR_OVERLAP_TRI_SELF)) || !counts || (max_prims > 0 && !prims));
}

static int overlap_tri_device(const char *name, gnxr_scene *s, const gnxr_tri_query *d_tris, int64_t n, uint32_t flags, int32_t max_prims, const int64_t *d_offsets,
                              int32_t *d_prims, int32_t *d_counts, uint64_t *d_work, bool counted, void *hip_stream) {
    // three dwordx4 loads per triangle, dword rows; the extent of CSR rows is on the device, so only the start of d_prims is looked at
    const QueryArg args[] = {{d_tris, (size_t)n * sizeof(gnxr_tri_query), "d_tris"}, {d_offsets, ((size_t)n + 1) * sizeof(int64_t), "d_offsets"},
                             {d_prims, max_prims > 0 ? (size_t)n * (size_t)max_prims * sizeof(int32_t) : 0, "d_prims"}, {d_counts, (size_t)n * sizeof(int32_t), "d_counts"},
                             {d_work, 2 * sizeof(uint64_t), "d_work"}};
    const unsigned align[] = {16, 8, 4, 4, 8};
    return walk_device(name, s, n, overlap_tri_missing(d_tris, n, flags, max_prims, d_prims, d_counts) || (counted && !d_work),
                       [&] { return overlap_tri_args_ok(s, d_tris, n, flags, max_prims, d_offsets, d_prims); }, args, align,
                       OverlapTriWalk{d_tris, flags, max_prims, d_offsets, d_prims, d_counts, reinterpret_cast<unsigned long long *>(d_work)}, hip_stream);
}

extern "C" {

int gnxr_overlap_tri_device(gnxr_scene *s, const gnxr_tri_query *d_tris, int64_t n, uint32_t flags, int32_t max_prims, const int64_t *d_offsets, int32_t *d_prims,
                            int32_t *d_counts, void *hip_stream) {
    return overlap_tri_device("gnxr_overlap_tri_device", s, d_tris, n, flags, max_prims, d_offsets, d_prims, d_counts, nullptr, false, hip_stream);
}
int gnxr_overlap_tri_counted_device(gnxr_scene *s, const gnxr_tri_query *d_tris, int64_t n, uint32_t flags, int32_t max_prims, const int64_t *d_offsets, int32_t *d_prims,
                                    int32_t *d_counts, uint64_t *d_work, void *hip_stream) {
    return overlap_tri_device("gnxr_overlap_tri_counted_device", s, d_tris, n, flags, max_prims, d_offsets, d_prims, d_counts, d_work, true, hip_stream);
}

int gnxr_overlap_tri(gnxr_scene *s, const gnxr_tri_query *tris, int64_t n, uint32_t flags, int32_t max_prims, const int64_t *offsets, int32_t *prims, int32_t *counts) {
    size_t list_bytes = max_prims > 0 ? (size_t)n * (size_t)max_prims * sizeof(int32_t) : 0;
    // host offsets can be read: the device copy of prims spans [0, offsets[n]), so the rows must lie inside it
    const auto rule = [&] {
        if (!overlap_tri_args_ok(s, tris, n, flags, max_prims, offsets, prims)) return false;
        if (!offsets) return true;
        if (offsets[0] < 0) { set_error("offsets[0] = %lld is negative", (long long)offsets[0]); return false; }
        for (int64_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) { set_error("offsets[%lld] = %lld is below offsets[%lld] = %lld: the offsets must ascend", (long long)(i + 1), (long long)offsets[i + 1], (long long)i, (long long)offsets[i]); return false; }
        list_bytes = (size_t)offsets[n] * sizeof(int32_t);
        return true;
    };
    if (int rc = walk_args(s, n, overlap_tri_missing(tris, n, flags, max_prims, prims, counts), rule)) return rc;   // here, before the table: the rule sizes the CSR rows
    const bool csr = offsets != nullptr;
    // CSR: prims goes up as well, so that what lies below offsets[0] comes back as it was; SELF: no queries go up
    const HostArray arrays[] = {{tris, nullptr, tris ? (size_t)n * sizeof(gnxr_tri_query) : 0}, {offsets, nullptr, csr ? ((size_t)n + 1) * sizeof(int64_t) : 0},
                                {csr ? prims : nullptr, prims, list_bytes}, {nullptr, counts, (size_t)n * sizeof(int32_t)}};
    return walk_host(s, n, false, [] { return true; }, arrays, [&](char *const *d) {
        // a CSR call whose rows are all empty has no prims on the device: rows mode's count-only form gives the same counts
        const bool lists = d[2] != nullptr;
        return OverlapTriWalk{reinterpret_cast<const gnxr_tri_query *>(d[0]), flags, lists ? max_prims : 0, lists && csr ? reinterpret_cast<const int64_t *>(d[1]) : nullptr,
                              reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[3]), nullptr};
    });
}

}  // extern "C"
