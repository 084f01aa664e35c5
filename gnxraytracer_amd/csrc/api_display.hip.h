// api_display.hip.h -- the display stage on device memory: gnxr_luminance_histogram_device, gnxr_exposure_device and gnxr_tonemap_device
// (validate, queue, return: pure image operations on the device that holds the image).  Once its parameters have passed, each call
// checks overlap, then alignment, returns for an empty call and only then asks the runtime where its arrays live (the pieces:
// api_device_call.hip.h).  The definition: include/gnxr.h; the kernels: display_kernel.hip.h.  Part of api.hip's translation unit.
#pragma once

static bool display_is_finite(float x) { return x - x == 0.f; }

// k_luminance_histogram's grid: every block ends with up to 256 atomic adds on the view's words in memory, and those, not the pixels,
// are what the kernel costs.  1920 x 1080 on an MI355X: 37 us with 8 blocks per CU, 26 with 4, 20 with 2 and with 1
constexpr int kHistogramBlocksPerCU = 2;

template <int CURVE>
static void launch_tonemap(bool srgb, int grid, hipStream_t stream, const float4 *rgba, const float4 *exposure, int npix, int wh, float e, float ww, int round, unsigned int *out) {
    if (srgb) hipLaunchKernelGGL((k_tonemap<CURVE, true>), dim3(grid), dim3(kBlock), 0, stream, rgba, exposure, npix, wh, e, ww, round, out);
    else hipLaunchKernelGGL((k_tonemap<CURVE, false>), dim3(grid), dim3(kBlock), 0, stream, rgba, exposure, npix, wh, e, ww, round, out);
}

extern "C" {

int gnxr_luminance_histogram_device(const gnxr_histogram_params *p, const float *d_rgba, uint32_t *d_hist, void *hip_stream) {
    const char *name = "luminance histogram";
    if (!p || !d_rgba || !d_hist) { set_error("%s: null argument (params, d_rgba and d_hist are required)", name); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_histogram_params)) { set_error("%s: struct_size must be sizeof(gnxr_histogram_params) = %zu", name, sizeof(gnxr_histogram_params)); return GNXR_ERR_INVALID; }
    if (p->width < 1 || p->height < 1 || p->n_views < 0) { set_error("%s: width and height >= 1 and n_views >= 0 are required", name); return GNXR_ERR_INVALID; }
    if (p->min_log2 < -126 || p->min_log2 > 111) { set_error("%s: min_log2 = %d is outside [-126, 111]", name, p->min_log2); return GNXR_ERR_INVALID; }
    long long npix = 0;
    if (int rc = check_view_pixels(p->width, p->height, p->n_views, name, &npix)) return rc;
    const size_t hist_bytes = (size_t)p->n_views * kHistWords * sizeof(uint32_t);
    const QueryArg args[] = {{d_rgba, (size_t)npix * sizeof(float4), "d_rgba"}, {d_hist, hist_bytes, "d_hist"}};
    const unsigned align[] = {16u, 16u};
    if (npix > 0 && ranges_overlap(args[0], args[1])) { set_error("%s: d_hist overlaps d_rgba", name); return GNXR_ERR_INVALID; }
    if (int rc = check_aligned(name, args, align, 2)) return rc;
    if (npix == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind(name, args)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(d_hist, 0, hist_bytes, stream));
    const int bias = (p->min_log2 + 127) << 4;
    const int wh = p->width * p->height;
    hipLaunchKernelGGL(k_luminance_histogram, dim3(grid_for(npix, kHistogramBlocksPerCU)), dim3(kBlock), 0, stream, (const float4 *)d_rgba, (int)npix, wh, bias, (unsigned int *)d_hist);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

int gnxr_exposure_device(const gnxr_exposure_params *p, const uint32_t *d_hist, const float *d_prev_exposure, float *d_exposure, void *hip_stream) {
    const char *name = "exposure";
    if (!p || !d_hist || !d_exposure) { set_error("%s: null argument (params, d_hist and d_exposure are required)", name); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_exposure_params)) { set_error("%s: struct_size must be sizeof(gnxr_exposure_params) = %zu", name, sizeof(gnxr_exposure_params)); return GNXR_ERR_INVALID; }
    if (p->n_views < 0) { set_error("%s: n_views = %d is negative", name, p->n_views); return GNXR_ERR_INVALID; }
    if (p->min_log2 < -126 || p->min_log2 > 111) { set_error("%s: min_log2 = %d is outside [-126, 111]", name, p->min_log2); return GNXR_ERR_INVALID; }
    const float fl[] = {p->key, p->low, p->high, p->rate, p->min_exposure, p->max_exposure};
    for (float x : fl)
        if (!display_is_finite(x)) { set_error("%s: key, low, high, rate, min_exposure and max_exposure must be finite", name); return GNXR_ERR_INVALID; }
    if (!(0.f <= p->low && p->low < p->high && p->high <= 1.f)) { set_error("%s: 0 <= low < high <= 1 is required, got low = %g and high = %g", name, p->low, p->high); return GNXR_ERR_INVALID; }
    if (!(p->key > 0.f)) { set_error("%s: key = %g must be > 0", name, p->key); return GNXR_ERR_INVALID; }
    if (!(p->rate > 0.f && p->rate <= 1.f)) { set_error("%s: rate = %g is outside (0, 1]", name, p->rate); return GNXR_ERR_INVALID; }
    if (!(p->min_exposure > 0.f && p->min_exposure <= p->max_exposure)) {
        set_error("%s: 0 < min_exposure <= max_exposure is required, got %g and %g", name, p->min_exposure, p->max_exposure);
        return GNXR_ERR_INVALID;
    }
    const size_t rec_bytes = (size_t)p->n_views * sizeof(float4);
    const QueryArg args[] = {{d_hist, (size_t)p->n_views * kHistWords * sizeof(uint32_t), "d_hist"}, {d_prev_exposure, rec_bytes, "d_prev_exposure"}, {d_exposure, rec_bytes, "d_exposure"}};
    const unsigned align[] = {16u, 16u, 16u};
    if (p->n_views > 0) {
        if (ranges_overlap(args[2], args[0])) { set_error("%s: d_exposure overlaps d_hist", name); return GNXR_ERR_INVALID; }
        if ((const void *)d_prev_exposure != (const void *)d_exposure && ranges_overlap(args[2], args[1])) {
            set_error("%s: d_exposure overlaps d_prev_exposure at an offset (in place means the same address)", name);
            return GNXR_ERR_INVALID;
        }
    }
    if (int rc = check_aligned(name, args, align, 3)) return rc;
    if (p->n_views == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind(name, args)) return rc;
    ExposureParams ep;
    ep.min_log2 = p->min_log2;
    ep.key = p->key; ep.low = p->low; ep.high = p->high; ep.rate = p->rate; ep.min_exposure = p->min_exposure; ep.max_exposure = p->max_exposure;
    hipLaunchKernelGGL(k_exposure, dim3(grid_for((long long)p->n_views * kBlock)), dim3(kExposureBlock), 0, (hipStream_t)hip_stream, (const unsigned int *)d_hist, (const float4 *)d_prev_exposure,
                       (float4 *)d_exposure, (int)p->n_views, ep);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

int gnxr_tonemap_device(const gnxr_tonemap_params *p, const float *d_rgba, const float *d_exposure, uint8_t *d_rgba8_out, void *hip_stream) {
    const char *name = "tonemap";
    if (!p || !d_rgba || !d_rgba8_out) { set_error("%s: null argument (params, d_rgba and d_rgba8_out are required)", name); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_tonemap_params)) { set_error("%s: struct_size must be sizeof(gnxr_tonemap_params) = %zu", name, sizeof(gnxr_tonemap_params)); return GNXR_ERR_INVALID; }
    if (p->width < 1 || p->height < 1 || p->n_views < 0) { set_error("%s: width and height >= 1 and n_views >= 0 are required", name); return GNXR_ERR_INVALID; }
    if (p->curve < GNXR_TONEMAP_LINEAR || p->curve > GNXR_TONEMAP_ACES) { set_error("%s: curve = %d is none of GNXR_TONEMAP_LINEAR, _REFERENCE, _REINHARD, _ACES", name, p->curve); return GNXR_ERR_INVALID; }
    if ((p->flags & ~(uint32_t)(GNXR_TONEMAP_SRGB | GNXR_TONEMAP_ROUND)) != 0) { set_error("%s: flags = 0x%x holds unknown bits", name, p->flags); return GNXR_ERR_INVALID; }
    if (!display_is_finite(p->exposure) || !(p->exposure >= 0.f)) { set_error("%s: exposure = %g must be finite and >= 0", name, p->exposure); return GNXR_ERR_INVALID; }
    if (!(p->white >= 1e-3f && p->white <= 65504.f)) { set_error("%s: white = %g is outside [1e-3, 65504]", name, p->white); return GNXR_ERR_INVALID; }
    long long npix = 0;
    if (int rc = check_view_pixels(p->width, p->height, p->n_views, name, &npix)) return rc;
    const QueryArg args[] = {{d_rgba, (size_t)npix * sizeof(float4), "d_rgba"}, {d_exposure, (size_t)p->n_views * sizeof(float4), "d_exposure"},
                             {d_rgba8_out, (size_t)npix * 4, "d_rgba8_out"}};
    const unsigned align[] = {16u, 16u, 4u};
    if (npix > 0) {
        for (int i = 0; i < 2; ++i)
            if (ranges_overlap(args[2], args[i])) { set_error("%s: d_rgba8_out overlaps %s", name, args[i].what); return GNXR_ERR_INVALID; }
    }
    if (int rc = check_aligned(name, args, align, 3)) return rc;
    if (npix == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind(name, args)) return rc;
    const bool srgb = (p->flags & GNXR_TONEMAP_SRGB) != 0;
    const int round = (p->flags & GNXR_TONEMAP_ROUND) ? 1 : 0, grid = grid_for(npix), wh = p->width * p->height;
    const float ww = p->white * p->white;
    hipStream_t stream = (hipStream_t)hip_stream;
    const float4 *in = (const float4 *)d_rgba, *ex = (const float4 *)d_exposure;
    unsigned int *out = (unsigned int *)d_rgba8_out;
    switch (p->curve) {
    case GNXR_TONEMAP_LINEAR: launch_tonemap<kToneLinear>(srgb, grid, stream, in, ex, (int)npix, wh, p->exposure, ww, round, out); break;
    case GNXR_TONEMAP_REFERENCE: launch_tonemap<kToneReference>(srgb, grid, stream, in, ex, (int)npix, wh, p->exposure, ww, round, out); break;
    case GNXR_TONEMAP_REINHARD: launch_tonemap<kToneReinhard>(srgb, grid, stream, in, ex, (int)npix, wh, p->exposure, ww, round, out); break;
    default: launch_tonemap<kToneAces>(srgb, grid, stream, in, ex, (int)npix, wh, p->exposure, ww, round, out); break;
    }
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

}  // extern "C"
