// api_lightprobe.hip.h -- light probes on device memory: gnxr_lightprobe_rays_device, gnxr_sh_project_device, gnxr_sh_irradiance_device and
// gnxr_bake_lightprobes_device (the definition: include/gnxr.h, "Light probes"; the kernels: lightprobe_kernel.hip.h).  The bake is the
// free-space front end of Li, as gnxr_bake_lightmap_device is the texture-space one: sub-batches of probe rays go through render_one's
// caller-ray loops and the projection adds their blocks of 64 samples in order.  Part of api.hip's translation unit (after api_bake.hip.h,
// whose helpers it shares).
#pragma once

// probes of a call: a slot index (probe * 9) and the probe -> pixel map are ints
static const long long kLightprobeMaxProbes = 1ll << 27;
static const int kShBlock = 64;   // samples of a block of the projection's sum: the width of a wave

// a wave per probe, as many blocks as the probes need or the device holds
static int sh_project_grid(long long n_probes) { return grid_for(n_probes * 64); }

extern "C" {

int gnxr_lightprobe_rays_device(gnxr_scene *s, int32_t width, int32_t height, const float *d_pos, const int32_t *d_px, const int32_t *d_py, const int32_t *d_s, int64_t n,
                                int32_t medium, gnxr_ray *d_rays, gnxr_li_sample *d_samples, void *hip_stream) {
    // (what needs no scene comes first: a malformed call is refused whatever else it carries)
    if (n < 0 || width <= 0 || height <= 0) { set_error("gnxr_lightprobe_rays_device: n = %lld must be >= 0 and the image at least 1 x 1, got %d x %d", (long long)n, width, height); return GNXR_ERR_INVALID; }
    if (medium < -1) { set_error("gnxr_lightprobe_rays_device: medium = %d is below -1", medium); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_rays | (uintptr_t)d_samples) & 15u) != 0) { set_error("gnxr_lightprobe_rays_device: d_rays and d_samples must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_pos | (uintptr_t)d_px | (uintptr_t)d_py | (uintptr_t)d_s) & 3u) != 0) {
        set_error("gnxr_lightprobe_rays_device: d_pos, d_px, d_py and d_s must be 4-byte aligned");
        return GNXR_ERR_INVALID;
    }
    if (!s || (n > 0 && (!d_pos || !d_px || !d_py || !d_s || !d_rays || !d_samples))) { set_error("gnxr_lightprobe_rays_device: null argument"); return GNXR_ERR_INVALID; }
    if (medium >= (int32_t)s->cs.media.size()) { set_error("gnxr_lightprobe_rays_device: medium = %d is outside [-1, %d)", medium, (int)s->cs.media.size()); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    const QueryArg args[] = {{d_pos, (size_t)n * 12, "d_pos"}, {d_px, (size_t)n * 4, "d_px"}, {d_py, (size_t)n * 4, "d_py"}, {d_s, (size_t)n * 4, "d_s"},
                             {d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_samples, (size_t)n * sizeof(gnxr_li_sample), "d_samples"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;   // the sampler tables never change after the scene is created: no lock
    hipStream_t stream = (hipStream_t)hip_stream;
    StatusWord status;
    unsigned long long bad = 0;
    if (int rc = status.alloc(stream)) return rc;
    hipLaunchKernelGGL(k_lightprobe_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, bake_sampler_tables(r, width, height), (int)width, (int)height, d_pos, (const int *)d_px,
                       (const int *)d_py, (const int *)d_s, (long long)n, (int)medium, reinterpret_cast<float4 *>(d_rays), reinterpret_cast<int4 *>(d_samples), status.d);
    HIP_TRY(hipGetLastError());
    if (int rc = status.fetch(&bad)) return rc;
    if (bad) {
        set_error("gnxr_lightprobe_rays_device: record %llu is out of range (a finite position, px in [0, %d), py in [0, %d), s >= 0); its ray and sample are 0",
                  (unsigned long long)~bad, width, height);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

// No scene: the device is the one that holds the arrays, as for gnxr_bake_dilate_device.
int gnxr_sh_project_device(const gnxr_ray *d_rays, const float *d_L, int32_t n_probes, int64_t n_samples, float *d_sh_sum, uint32_t flags, void *hip_stream) {
    if (n_probes < 0 || n_samples < 0 || n_probes > kLightprobeMaxProbes) { set_error("gnxr_sh_project_device: n_probes must lie in [0, %lld] and n_samples be >= 0", kLightprobeMaxProbes); return GNXR_ERR_INVALID; }
    if (flags & ~GNXR_SH_CONTINUE) { set_error("gnxr_sh_project_device: unknown flag bits 0x%x", flags & ~GNXR_SH_CONTINUE); return GNXR_ERR_INVALID; }
    if (n_probes == 0) return GNXR_OK;
    if (!d_sh_sum || (n_samples > 0 && (!d_rays || !d_L))) { set_error("gnxr_sh_project_device: null argument"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_rays | (uintptr_t)d_L | (uintptr_t)d_sh_sum) & 15u) != 0) { set_error("gnxr_sh_project_device: d_rays, d_L and d_sh_sum must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    const size_t n = (size_t)n_probes * (size_t)n_samples;
    const QueryArg args[] = {{d_sh_sum, (size_t)n_probes * 9 * sizeof(float4), "d_sh_sum"}, {d_rays, n * sizeof(gnxr_ray), "d_rays"}, {d_L, n * sizeof(float4), "d_L"}};
    DeviceCall call;
    if (int rc = call.bind("gnxr_sh_project_device", args, n_samples > 0 ? 3 : 1)) return rc;
    hipLaunchKernelGGL(k_sh_project, dim3(sh_project_grid(n_probes)), dim3(kBlock), 0, (hipStream_t)hip_stream, reinterpret_cast<const float4 *>(d_rays),
                       reinterpret_cast<const float4 *>(d_L), (int)n_probes, (long long)n_samples, (int)((flags & GNXR_SH_CONTINUE) != 0), reinterpret_cast<float4 *>(d_sh_sum));
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

int gnxr_sh_irradiance_device(const float *d_sh, int32_t n_probes, const int32_t *d_probe, const float *d_normals, int64_t n, float *d_E, void *hip_stream) {
    if (n_probes < 0 || n < 0 || n_probes > kLightprobeMaxProbes) { set_error("gnxr_sh_irradiance_device: n_probes must lie in [0, %lld] and n be >= 0", kLightprobeMaxProbes); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (!d_probe || !d_normals || !d_E || (n_probes > 0 && !d_sh)) { set_error("gnxr_sh_irradiance_device: null argument"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_sh | (uintptr_t)d_E) & 15u) != 0 || (((uintptr_t)d_probe | (uintptr_t)d_normals) & 3u) != 0) {
        set_error("gnxr_sh_irradiance_device: d_sh and d_E must be 16-byte aligned, d_probe and d_normals 4-byte aligned");
        return GNXR_ERR_INVALID;
    }
    if (int rc = ensure_device()) return rc;
    const QueryArg args[] = {{d_E, (size_t)n * sizeof(float4), "d_E"}, {d_probe, (size_t)n * 4, "d_probe"}, {d_normals, (size_t)n * 12, "d_normals"},
                             {d_sh, (size_t)n_probes * 9 * sizeof(float4), "d_sh"}};
    DeviceCall call;
    if (int rc = call.bind("gnxr_sh_irradiance_device", args, n_probes > 0 ? 4 : 3)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    StatusWord status;
    unsigned long long bad = 0;
    if (int rc = status.alloc(stream)) return rc;
    hipLaunchKernelGGL(k_sh_irradiance, dim3(grid_for(n)), dim3(kBlock), 0, stream, reinterpret_cast<const float4 *>(d_sh), (int)n_probes, (const int *)d_probe, d_normals,
                       (long long)n, reinterpret_cast<float4 *>(d_E), status.d);
    HIP_TRY(hipGetLastError());
    if (int rc = status.fetch(&bad)) return rc;
    if (bad) {
        set_error("gnxr_sh_irradiance_device: record %llu names a probe outside [0, %d); its irradiance is 0", (unsigned long long)~bad, n_probes);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

int gnxr_bake_lightprobes_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_lightprobe_params *probe, const float *d_positions, int32_t n_probes,
                                 void *d_sh_out, void *hip_stream, gnxr_stats *stats) {
    // (what needs no scene comes first: a malformed call is refused whatever else it carries)
    if (!p || !probe) { set_error("gnxr_bake_lightprobes_device: null argument"); return GNXR_ERR_INVALID; }
    if (probe->struct_size != (int32_t)sizeof(gnxr_lightprobe_params)) {
        set_error("gnxr_bake_lightprobes_device: struct_size must be sizeof(gnxr_lightprobe_params) = %zu", sizeof(gnxr_lightprobe_params));
        return GNXR_ERR_INVALID;
    }
    if (probe->flags != 0) { set_error("gnxr_bake_lightprobes_device: unknown flag bits 0x%x", probe->flags); return GNXR_ERR_INVALID; }
    if (probe->medium < -1) { set_error("gnxr_bake_lightprobes_device: medium = %d is below -1", probe->medium); return GNXR_ERR_INVALID; }
    if (n_probes < 0 || n_probes > kLightprobeMaxProbes) { set_error("gnxr_bake_lightprobes_device: n_probes = %d is outside [0, %lld]", n_probes, kLightprobeMaxProbes); return GNXR_ERR_INVALID; }
    if (p->width <= 0 || p->height <= 0 || (long long)p->width * p->height < n_probes) {
        set_error("gnxr_bake_lightprobes_device: the %d x %d grid of pixels does not hold %d probes", p->width, p->height, n_probes);
        return GNXR_ERR_INVALID;
    }
    if (p->spp_begin != 0 || p->spp_end != 0) { set_error("gnxr_bake_lightprobes_device: spp_begin and spp_end must be 0 (a bake takes all samples of a probe)"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "gnxr_bake_lightprobes_device", "a caller that shards splits the list of probes")) return rc;
    if (((uintptr_t)d_positions & 3u) != 0 || ((uintptr_t)d_sh_out & 15u) != 0) { set_error("gnxr_bake_lightprobes_device: d_positions must be 4-byte aligned, d_sh_out 16-byte aligned"); return GNXR_ERR_INVALID; }
    if (!s || (n_probes > 0 && (!d_positions || !d_sh_out))) { set_error("gnxr_bake_lightprobes_device: null argument"); return GNXR_ERR_INVALID; }
    if (probe->medium >= (int32_t)s->cs.media.size()) {
        set_error("gnxr_bake_lightprobes_device: medium = %d is outside [-1, %d)", probe->medium, (int)s->cs.media.size());
        return GNXR_ERR_INVALID;
    }
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    {   // the parameters and the support matrix of Li for caller rays, before anything is queued
        const RaySource src{nullptr, nullptr, nullptr, 1};
        RenderPlan pl;
        if (int rc = plan_render(s->cs, &pp, &src, nullptr, nullptr, &pl)) return rc;
        DHalton h = make_halton(pp.width, pp.height);
        if (int rc = halton_index_bound(&h, pp.spp, pl.max_light_samples)) return rc;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_probes == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    const int W = p->width, spp = p->spp;
    const QueryArg args[] = {{d_positions, (size_t)n_probes * 12, "d_positions"}, {d_sh_out, (size_t)n_probes * 9 * sizeof(float4), "d_sh_out"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    std::lock_guard<std::recursive_mutex> lock(r->render_mutex);   // held across the sub-batches: one bake, render or Li call per copy at a time
    hipStream_t stream = (hipStream_t)hip_stream;
    float4 *out = (float4 *)d_sh_out;

    // ---- sub-batches: whole probes while a probe's samples fit a batch, else ranges of whole blocks of one probe
    const long long batch = pp.samples_per_pass > 0 ? (long long)pp.samples_per_pass : kBakeBatchRays;
    const int samples = spp <= batch ? spp : (int)std::max<long long>(kShBlock, batch / kShBlock * kShBlock);
    const int probes = (int)std::max<long long>(1, std::min<long long>(n_probes, batch / samples));
    const size_t cap = (size_t)samples * probes;
    StreamScratch sub;   // [rays | samples | L] of one sub-batch
    HIP_TRY(sub.alloc(cap * (sizeof(gnxr_ray) + sizeof(gnxr_li_sample) + sizeof(float4)), stream));
    gnxr_ray *rays = (gnxr_ray *)sub.p;
    gnxr_li_sample *recs = (gnxr_li_sample *)(sub.p + cap * sizeof(gnxr_ray));
    float *L = (float *)(sub.p + cap * (sizeof(gnxr_ray) + sizeof(gnxr_li_sample)));
    const DSamplerTables st = bake_sampler_tables(r, p->width, p->height);
    for (int k0 = 0; k0 < n_probes; k0 += probes) {
        const int nk = std::min(probes, n_probes - k0);
        for (int s0 = 0; s0 < spp; s0 += samples) {
            const int ns = std::min(samples, spp - s0);
            const long long n = (long long)nk * ns;
            hipLaunchKernelGGL(k_lightprobe_bake_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, st, W, d_positions, k0, s0, ns, n, (int)probe->medium,
                               reinterpret_cast<float4 *>(rays), reinterpret_cast<int4 *>(recs));
            HIP_TRY(hipGetLastError());
            const RaySource src{rays, recs, L, n};
            gnxr_stats t;
            memset(&t, 0, sizeof(t));
            if (int rc = render_one(r, &pp, nullptr, hip_stream, &t, /*reserve_only=*/false, &src)) return rc;
            if (stats) bake_add_stats(stats, t);
            hipLaunchKernelGGL(k_sh_project, dim3(sh_project_grid(nk)), dim3(kBlock), 0, stream, reinterpret_cast<const float4 *>(rays), reinterpret_cast<const float4 *>(L), nk,
                               (long long)ns, (int)(s0 > 0), out + 9 * (size_t)k0);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_lightprobe_finish, dim3(grid_for((long long)n_probes * 9)), dim3(kBlock), 0, stream, d_positions, (long long)n_probes * 9, spp, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));   // back when the coefficients are written, as gnxr_li_device is when d_L is
    return GNXR_OK;
}

}  // extern "C"
