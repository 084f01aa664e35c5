// api_spherecast.hip.h -- sphere casts (spherecast_kernel.hip.h): gnxr_sphere_cast_device on device memory, its counting form for the
// measurement, and gnxr_sphere_cast for host arrays.  This file holds the entry points' signatures, their array and alignment tables
// and the kernel selection; how the walk is run -- checks, chunks, launches, copies -- is api_walk.hip.h's.  Part of api.hip's
// translation unit.
#pragma once

// work: nullptr, or two device words the counting instantiation adds nodes visited and triangles tested to
struct SphereCastWalk {
    typedef SphereCastArrays Arrays;
    typedef uint2 Spill;
    static constexpr bool kBinnable = false;   // casts are walked in caller order: QueryBinning takes 16-byte records
    const struct gnxr_sphere_cast *casts;
    struct gnxr_closest_point *out;
    unsigned long long *work;
    size_t entry_bytes() const { return sizeof(uint2); }
    int lds_levels() const { return Knobs::spherecast_lds_levels(); }
    Arrays at(long long base) const { return {reinterpret_cast<const float4 *>(casts + base), reinterpret_cast<float4 *>(out + base)}; }
    auto kernel(bool wide) const {
        static constexpr decltype(&k_sphere_cast<true, true>) k[2][2] = {{k_sphere_cast<false, false>, k_sphere_cast<false, true>},
                                                                         {k_sphere_cast<true, false>, k_sphere_cast<true, true>}};
        return k[wide][work != nullptr];
    }
};

static int sphere_cast_device(const char *name, gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_work,
                              bool counted, void *hip_stream) {
    // two dwordx4 loads per cast, two dwordx4 stores per record
    const QueryArg args[] = {{d_casts, (size_t)n * sizeof(struct gnxr_sphere_cast), "d_casts"}, {d_out, (size_t)n * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_work, 2 * sizeof(uint64_t), "d_work"}};
    const unsigned align[] = {16, 16, 8};
    return walk_device(name, s, n, (n > 0 && (!d_casts || !d_out)) || (counted && !d_work), [] { return true; }, args, align,
                       SphereCastWalk{d_casts, d_out, reinterpret_cast<unsigned long long *>(d_work)}, hip_stream);
}

extern "C" {

int gnxr_sphere_cast_device(gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, void *hip_stream) {
    return sphere_cast_device("gnxr_sphere_cast_device", s, d_casts, n, d_out, nullptr, false, hip_stream);
}
int gnxr_sphere_cast_counted_device(gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_work, void *hip_stream) {
    return sphere_cast_device("gnxr_sphere_cast_counted_device", s, d_casts, n, d_out, d_work, true, hip_stream);
}

int gnxr_sphere_cast(gnxr_scene *s, const struct gnxr_sphere_cast *casts, int64_t n, struct gnxr_closest_point *out) {
    const HostArray arrays[] = {{casts, nullptr, (size_t)n * sizeof(struct gnxr_sphere_cast)}, {nullptr, out, (size_t)n * sizeof(struct gnxr_closest_point)}};
    return walk_host(s, n, !casts || !out, [] { return true; }, arrays, [](char *const *d) {
        return SphereCastWalk{reinterpret_cast<const struct gnxr_sphere_cast *>(d[0]), reinterpret_cast<struct gnxr_closest_point *>(d[1]), nullptr};
    });
}

}  // extern "C"
