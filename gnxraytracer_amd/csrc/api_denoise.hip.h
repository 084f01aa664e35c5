// api_denoise.hip.h -- gnxr_denoise_device: the edge-avoiding a-trous filter on device memory, guided by the feature buffers (the
// definition: include/gnxr.h; the kernels: denoise_kernel.hip.h).  No scene: the device is the one that holds the arrays
// (DeviceCall::bind(name, args), api_device_call.hip.h).  Part of api.hip's translation unit.
#pragma once

template <bool B, bool N, bool Z>
static void launch_denoise_atrous(int grid, hipStream_t stream, const DenoiseImage &im, const DenoiseStep &st, const float4 *src, const float4 *guide, float4 *dst,
                                  const gnxr_denoise_buffers &in, float4 *out) {
    const float4 *a = (const float4 *)in.d_color, *b = (const float4 *)in.d_color_b, *albedo = (const float4 *)in.d_albedo;
    // steps 1 and 2 keep their tile in LDS; a wider step's tile would not fit beside a useful number of waves
    if (st.step == 1) hipLaunchKernelGGL((k_denoise_atrous<B, N, Z, 1>), dim3(grid), dim3(kBlock), 0, stream, im, st, src, guide, dst, a, b, albedo, out);
    else if (st.step == 2) hipLaunchKernelGGL((k_denoise_atrous<B, N, Z, 2>), dim3(grid), dim3(kBlock), 0, stream, im, st, src, guide, dst, a, b, albedo, out);
    else hipLaunchKernelGGL((k_denoise_atrous<B, N, Z, 0>), dim3(grid), dim3(kBlock), 0, stream, im, st, src, guide, dst, a, b, albedo, out);
}

extern "C" {

int gnxr_denoise_device(const gnxr_denoise_params *p, const gnxr_denoise_buffers *in, float *d_rgba_out, void *hip_stream) {
    if (!p || !in || !d_rgba_out) { set_error("denoise: null argument"); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_denoise_params) || in->struct_size != (int32_t)sizeof(gnxr_denoise_buffers)) {
        set_error("denoise: struct_size must be sizeof(gnxr_denoise_params) = %zu and sizeof(gnxr_denoise_buffers) = %zu", sizeof(gnxr_denoise_params), sizeof(gnxr_denoise_buffers));
        return GNXR_ERR_INVALID;
    }
    if (!in->d_color) { set_error("denoise: d_color is null"); return GNXR_ERR_INVALID; }
    if (p->width < 1 || p->height < 1 || p->n_views < 0) { set_error("denoise: width and height >= 1 and n_views >= 0 are required"); return GNXR_ERR_INVALID; }
    if (p->iterations < 1 || p->iterations > 8) { set_error("denoise: iterations = %d is outside [1, 8]", p->iterations); return GNXR_ERR_INVALID; }
    if (!(p->sigma_color >= 0.f) || !(p->sigma_normal >= 0.f) || !(p->sigma_depth >= 0.f)) { set_error("denoise: the sigmas must be >= 0 (no NaN)"); return GNXR_ERR_INVALID; }
    long long npix = 0;
    if (int rc = check_view_pixels(p->width, p->height, p->n_views, "denoise", &npix)) return rc;
    const size_t n4 = (size_t)npix * sizeof(float4), n1 = (size_t)npix * sizeof(float);
    const QueryArg args[] = {{in->d_color, n4, "d_color"}, {in->d_color_b, n4, "d_color_b"}, {in->d_albedo, n4, "d_albedo"}, {in->d_normal, n4, "d_normal"},
                             {in->d_depth, n1, "d_depth"}, {d_rgba_out, n4, "d_rgba_out"}};
    const unsigned align[] = {16u, 16u, 16u, 16u, 4u, 16u};   // d_depth: one float per pixel
    if (int rc = check_aligned("denoise", args, align, 6)) return rc;
    if (npix == 0) return GNXR_OK;
    for (int i = 0; i < 5; ++i) {   // the output may BE a colour share (every lane reads its own pixel before it writes it); it overlaps nothing else
        if (i < 2 && args[i].p == (const void *)d_rgba_out) continue;
        if (ranges_overlap(args[i], args[5])) {
            set_error(i < 2 ? "denoise: d_rgba_out overlaps %s at an offset (in place means the same address)" : "denoise: d_rgba_out overlaps %s", args[i].what);
            return GNXR_ERR_INVALID;
        }
    }
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind("denoise", args)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamScratch scratch;   // two ping-pong work records and one guide record per pixel
    HIP_TRY(scratch.alloc(3 * n4, stream));
    float4 *work[2] = {(float4 *)scratch.p, (float4 *)scratch.p + npix}, *guide = (float4 *)scratch.p + 2 * npix;
    const bool B = in->d_color_b != nullptr, N = in->d_normal && p->sigma_normal > 0.f, Z = in->d_depth && p->sigma_depth > 0.f;
    hipLaunchKernelGGL(k_denoise_prepare, dim3(grid_for(npix)), dim3(kBlock), 0, stream, (const float4 *)in->d_color, (const float4 *)in->d_color_b, (const float4 *)in->d_albedo,
                       (const float4 *)in->d_normal, in->d_depth, npix, work[0], guide);
    DenoiseImage im;
    im.W = p->width; im.H = p->height;
    im.tiles_x = (p->width + kDenoiseTileW - 1) / kDenoiseTileW;
    im.tiles_y = (p->height + kDenoiseTileH - 1) / kDenoiseTileH;
    im.n_tiles = (long long)p->n_views * im.tiles_y * im.tiles_x;
    const int grid = grid_for(im.n_tiles * kBlock, 32);
    const float inv_sc = 1.f / (p->sigma_color * p->sigma_color);
    for (int i = 0; i < p->iterations; ++i) {
        DenoiseStep st;
        st.step = 1 << i;
        st.use_color = p->sigma_color > 0.f;
        st.last = i == p->iterations - 1;
        st.sigma_color = p->sigma_color;
        st.inv_sc_i = inv_sc * (float)(1 << (2 * i));
        st.inv_sn = 1.f / (p->sigma_normal * p->sigma_normal);
        st.sigma_z_step = p->sigma_depth * (float)st.step;
        const float4 *src = work[i & 1];
        float4 *dst = work[1 - (i & 1)];
        switch ((B ? 4 : 0) | (N ? 2 : 0) | (Z ? 1 : 0)) {
        case 0: launch_denoise_atrous<false, false, false>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 1: launch_denoise_atrous<false, false, true>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 2: launch_denoise_atrous<false, true, false>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 3: launch_denoise_atrous<false, true, true>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 4: launch_denoise_atrous<true, false, false>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 5: launch_denoise_atrous<true, false, true>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        case 6: launch_denoise_atrous<true, true, false>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        default: launch_denoise_atrous<true, true, true>(grid, stream, im, st, src, guide, dst, *in, (float4 *)d_rgba_out); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

}  // extern "C"
