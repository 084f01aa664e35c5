// api_spherecast.hip.h -- sphere casts (spherecast_kernel.hip.h): gnxr_sphere_cast_device on device memory, its counting form for the
// measurement, and gnxr_sphere_cast for host arrays.  Part of api.hip's translation unit (after api_near.hip.h: the front end is its
// siblings' -- the same checks, DeviceCall, query_device_scene, WalkLaunch, scratch from the stream-ordered allocator on the caller's
// stream).  Casts are walked in caller order: QueryBinning takes 16-byte records.
#pragma once

// casts of one launch: the kernel indexes casts in 64 bits, a thread's spill column by its number in the grid
static const long long kSphereCastLaunchMax = 1ll << 30;

// The walk over n casts on `st`.  d_work: nullptr, or two device words the counting instantiation adds nodes visited and triangles
// tested to.
static int sphere_cast_launch(gnxr_scene *r, const DScene &sc, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, unsigned long long *d_work,
                              hipStream_t st) {
    if (r->cs.n_triangles == 0) {
        hipLaunchKernelGGL(k_sphere_cast_none, dim3(grid_for(n)), dim3(kBlock), 0, st, reinterpret_cast<float4 *>(d_out), (long long)n);
        HIP_TRY(hipGetLastError());
        return GNXR_OK;
    }
    const long long per_launch = kSphereCastLaunchMax;
    const long long most = std::min<long long>(n, per_launch);   // casts of one launch
    WalkLaunch w;
    if (int rc = w.plan(r, sizeof(uint2), Knobs::spherecast_lds_levels(), most, st)) return rc;
    for (long long base = 0; base < n; base += per_launch) {
        const long long cnt = std::min<long long>(n - base, per_launch);
        SphereCastArrays qa;
        qa.casts = reinterpret_cast<const float4 *>(d_casts + base);
        qa.out = reinterpret_cast<float4 *>(d_out + base);
#define GX_SPHERECAST(W, C) hipLaunchKernelGGL((k_sphere_cast<W, C>), dim3(w.grid(cnt)), dim3(kBlock), w.lds, st, sc, qa, (long long)cnt, w.lds_entries, w.entries, \
                                               (uint2 *)w.spill, d_work)
        if (d_work) { if (w.wide) GX_SPHERECAST(true, true); else GX_SPHERECAST(false, true); }
        else { if (w.wide) GX_SPHERECAST(true, false); else GX_SPHERECAST(false, false); }
#undef GX_SPHERECAST
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

static int sphere_cast_device(gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_work, bool counted, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_casts || !d_out)) || (counted && !d_work)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_casts & 15u) != 0) { set_error("d_casts is not 16-byte aligned (two dwordx4 loads per cast)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_out & 15u) != 0) { set_error("d_out is not 16-byte aligned (two dwordx4 stores per record)"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_work & 7u) != 0) { set_error("d_work is not 8-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_casts, (size_t)n * sizeof(struct gnxr_sphere_cast), "d_casts"}, {d_out, (size_t)n * sizeof(struct gnxr_closest_point), "d_out"},
                             {d_work, 2 * sizeof(uint64_t), "d_work"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    return sphere_cast_launch(r, query_device_scene(r), d_casts, n, d_out, reinterpret_cast<unsigned long long *>(d_work), (hipStream_t)hip_stream);
}

extern "C" {

int gnxr_sphere_cast_device(gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, void *hip_stream) {
    return sphere_cast_device(s, d_casts, n, d_out, nullptr, false, hip_stream);
}
int gnxr_sphere_cast_counted_device(gnxr_scene *s, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out, uint64_t *d_work, void *hip_stream) {
    return sphere_cast_device(s, d_casts, n, d_out, d_work, true, hip_stream);
}

// host arrays: copy in, the device call's walk on the null stream, copy out
int gnxr_sphere_cast(gnxr_scene *s, const struct gnxr_sphere_cast *casts, int64_t n, struct gnxr_closest_point *out) {
    if (!s || !casts || !out || n < 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<struct gnxr_sphere_cast> dq;
    DevBuf<struct gnxr_closest_point> dout;
    int rc;
    if ((rc = dq.upload(casts, (size_t)n)) || (rc = dout.alloc((size_t)n))) return rc;
    if ((rc = sphere_cast_launch(s, query_device_scene(s), dq.p, n, dout.p, nullptr, nullptr)) != GNXR_OK) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(struct gnxr_closest_point), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"
