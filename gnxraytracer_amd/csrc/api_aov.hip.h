// api_aov.hip.h -- first-hit feature buffers on device memory: gnxr_render_aov_device (aov_kernel.hip.h).
// Part of api.hip's translation unit (after api_query.hip.h: the call's traversal is closest_hit_codes; its front end is api_device_call.hip.h).
#pragma once

// largest share of the free device memory, and largest amount at all, that the rays of one sub-pass may take when samples_per_pass is 0
static const size_t kAovFreeShare = 4, kAovRayBytesMax = (size_t)1 << 30;

extern "C" {

int gnxr_render_aov_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_camera *cameras, const int32_t *camera_media, int32_t n_views,
                           const gnxr_aov_buffers *out, void *hip_stream, gnxr_stats *stats) {
    if (!s || !p || !out) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (n_views < 0 || (!cameras && n_views > 1)) { set_error("feature buffers: n_views = %d with %s cameras", n_views, cameras ? "these" : "null"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "feature buffers", "a caller that shards splits the list of views")) return rc;
    if (!image_and_samples_ok(*p) || p->samples_per_pass < 0) return invalid_render_params();
    if (!out->d_albedo && !out->d_normal && !out->d_shading_normal && !out->d_depth && !out->d_ids) { set_error("feature buffers: no channel requested"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)out->d_albedo | (uintptr_t)out->d_normal | (uintptr_t)out->d_shading_normal) & 15u) != 0) {
        set_error("d_albedo, d_normal and d_shading_normal must be 16-byte aligned");
        return GNXR_ERR_INVALID;
    }
    if ((((uintptr_t)out->d_depth | (uintptr_t)out->d_ids) & 3u) != 0) { set_error("d_depth and d_ids must be 4-byte aligned"); return GNXR_ERR_INVALID; }
    // a sample slot is sample * (n_views * W * H) + pixel, traced by the kernel of the views call: its limit
    long long total = 0;
    if (int rc = check_view_pixels(p->width, p->height, n_views, "feature buffers", &total)) return rc;
    if (!cameras) camera_media = nullptr;   // the scene's own camera sits in the scene's camera medium
    if (int rc = check_view_media(s, camera_media, n_views, "feature buffers")) return rc;
    if (n_views == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }
    if (int rc = ensure_device()) return rc;
    const size_t npx = (size_t)total;
    const QueryArg args[] = {{out->d_albedo, npx * 16, "d_albedo"}, {out->d_normal, npx * 16, "d_normal"}, {out->d_shading_normal, npx * 16, "d_shading_normal"},
                             {out->d_depth, npx * 4, "d_depth"}, {out->d_ids, npx * 8, "d_ids"}};
    DeviceCall call;
    int rc = call.bind(s, args);
    if (rc) return rc;
    gnxr_scene *r = call.r;
    // ids alone come from the lowest sample of the range: nothing else is traced then
    const bool ids_only = !out->d_albedo && !out->d_normal && !out->d_shading_normal && !out->d_depth;
    const int W = p->width, H = p->height, s_begin = p->spp_begin, s_end = ids_only ? p->spp_begin + 1 : (p->spp_end > 0 ? p->spp_end : p->spp), ns = s_end - s_begin;

    std::lock_guard<std::recursive_mutex> lock(r->render_mutex);   // as render_one: one render, Li, views or feature-buffer call per handle at a time
    const auto t_start = std::chrono::steady_clock::now();
    hipStream_t st = (hipStream_t)hip_stream;
    DScene sc = query_device_scene(r);
    sc.st.perms = r->perms.p; sc.st.primes = r->primes.p; sc.st.prime_sums = r->prime_sums.p; sc.st.prime_magic = r->prime_magic.p;
    sc.st.h = make_halton(W, H);
    if ((rc = halton_index_bound(&sc.st.h, p->spp, 1)) != GNXR_OK) return rc;   // (the camera dimensions alone: no array samples)

    std::vector<DCamera> h_cams((size_t)n_views);
    if (cameras) make_view_cameras(cameras, camera_media, n_views, W, H, h_cams.data());
    else h_cams[0] = make_camera(r->cs.camera, W, H, r->cs.camera_medium);

    // ---- plan: k samples of every pixel per sub-pass, 32 bytes each; auto: what a share of the free memory holds
    const int mask = (out->d_albedo ? kAovAlbedo : 0) | (out->d_normal ? kAovNormal : 0) | (out->d_shading_normal ? kAovShading : 0);
    long long k = p->samples_per_pass;
    if (k <= 0) {
        size_t free_b = 0, total_b = 0;
        size_t budget = (size_t)256 << 20;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(free_b / kAovFreeShare, kAovRayBytesMax);
        k = (long long)(budget / (sizeof(gnxr_ray) * npx));
    }
    k = std::max<long long>(1, std::min<long long>(k, ns));
    auto pad256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t cam_bytes = pad256((size_t)n_views * sizeof(DCamera)), ray_bytes = pad256((size_t)k * npx * sizeof(gnxr_ray)), acc_bytes = pad256(npx * sizeof(float4));
    const bool accA = out->d_albedo != nullptr, accN = out->d_normal || out->d_depth, accS = out->d_shading_normal != nullptr;
    const size_t sums_bytes = acc_bytes * ((accA ? 1 : 0) + (accN ? 1 : 0) + (accS ? 1 : 0));
    StreamScratch scratch;
    {
        const hipError_t e = scratch.alloc(cam_bytes + ray_bytes + sums_bytes, st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("feature buffers: %zu bytes of scratch (%lld samples of %zu pixels per sub-pass) could not be allocated: %s", cam_bytes + ray_bytes + sums_bytes, k, npx, hipGetErrorString(e));
            return hip_status(e);
        }
    }
    DCamera *d_cams = reinterpret_cast<DCamera *>(scratch.p);
    gnxr_ray *d_rays = reinterpret_cast<gnxr_ray *>(scratch.p + cam_bytes);
    char *sums = scratch.p + cam_bytes + ray_bytes;
    AovAccum acc = {nullptr, nullptr, nullptr};
    if (accA) { acc.albedo = reinterpret_cast<float4 *>(sums); sums += acc_bytes; }
    if (accN) { acc.normal = reinterpret_cast<float4 *>(sums); sums += acc_bytes; }
    if (accS) { acc.shading = reinterpret_cast<float4 *>(sums); sums += acc_bytes; }
    // every ray's leaf code lives in that ray's pad word: the traversal's one-int-per-32-bytes result array starts at ray 0's
    static_assert(sizeof(gnxr_ray) == sizeof(gnxr_hit) && offsetof(gnxr_hit, prim) == 0 && offsetof(gnxr_ray, _pad) == 28, "the leaf code overlays gnxr_ray::_pad");
    gnxr_hit *d_codes = reinterpret_cast<gnxr_hit *>(reinterpret_cast<char *>(d_rays) + offsetof(gnxr_ray, _pad));

    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, st));
    // (h_cams outlives the copy: the call returns after the stream has drained)
    HIP_TRY(hipMemcpyAsync(d_cams, h_cams.data(), (size_t)n_views * sizeof(DCamera), hipMemcpyHostToDevice, st));
    if (sums_bytes) HIP_TRY(hipMemsetAsync(scratch.p + cam_bytes + ray_bytes, 0, sums_bytes, st));
    DRender rr;
    memset(&rr, 0, sizeof(rr));
    rr.cam = h_cams[0];   // read by no kernel of this call
    rr.W = W; rr.H = H; rr.spp = p->spp; rr.shard_count = 1; rr.shard_rows = 1; rr.npix = (int)total;
    AovTables at;
    at.albedo = reinterpret_cast<const float4 *>(r->aov_albedo.p);
    at.authored = r->material_authored.p;
    at.n_authored = (int)(r->cs.aov_albedo.size() / 4);
    at.n_internal = (int)r->cs.material_authored.size();
    const bool spheres = r->cs.n_spheres > 0;
    unsigned passes = 0, launches = 0;
    for (int s0 = s_begin; s0 < s_end; s0 += (int)k) {
        const int kk = (int)std::min<long long>(k, s_end - s0);
        const long long n = (long long)kk * (long long)npx;
        hipLaunchKernelGGL(k_aov_raygen, dim3(grid_for(n)), dim3(kBlock), 0, st, sc.st, rr, (const DCamera *)d_cams, reinterpret_cast<float4 *>(d_rays), n, s0);
        HIP_TRY(hipGetLastError());
        if ((rc = closest_hit_codes(r, sc, d_rays, n, d_codes, st)) != GNXR_OK) return rc;
        const int first = s0 == s_begin ? 1 : 0, want_depth = out->d_depth ? 1 : 0;
        int2 *ids = reinterpret_cast<int2 *>(out->d_ids);
#define GX_AOV_RESOLVE(M) case M: hipLaunchKernelGGL((k_aov_resolve<M>), dim3(grid_for(total)), dim3(kBlock), 0, st, sc, at, reinterpret_cast<const float4 *>(d_rays), (int)total, kk, first, acc, want_depth, ids); break;
        switch (mask) { GX_AOV_INSTANCES(GX_AOV_RESOLVE) }
#undef GX_AOV_RESOLVE
        HIP_TRY(hipGetLastError());
        ++passes;
        launches += 3;
    }
    if (sums_bytes) {
        AovOut ao;
        ao.albedo = reinterpret_cast<float4 *>(out->d_albedo); ao.normal = reinterpret_cast<float4 *>(out->d_normal); ao.shading = reinterpret_cast<float4 *>(out->d_shading_normal);
        ao.depth = out->d_depth; ao.ids = reinterpret_cast<int2 *>(out->d_ids);
        hipLaunchKernelGGL(k_aov_finish, dim3(grid_for(total)), dim3(kBlock), 0, st, acc, ao, (int)total, (int)p->spp);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));   // the buffers are written when the call returns
    HIP_TRY(hipGetLastError());
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        stats->camera_samples = stats->rays_closest = (uint64_t)ns * (uint64_t)npx;
        stats->passes = passes;
        stats->kernel_launches = launches;
        stats->state_bytes = (uint64_t)k * npx * sizeof(gnxr_ray) + (sums_bytes / acc_bytes) * npx * sizeof(float4);   // rays of a sub-pass + running sums
        stats->seconds_render = ms * 1e-3;
        stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
    return GNXR_OK;
}

}  // extern "C"
