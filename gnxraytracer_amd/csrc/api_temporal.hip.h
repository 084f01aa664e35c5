// api_temporal.hip.h -- temporal accumulation on device memory: gnxr_motion_device (a pixel-centre G-buffer and where each pixel was one frame
// ago; around closest_hit_codes, the front end of the feature buffers) and gnxr_temporal_accumulate_device (validate, gather and blend: a
// pure image operation on the device that holds its arrays, found by api_device_call.hip.h's walk).  The definition: include/gnxr.h; the kernels:
// temporal_kernel.hip.h; gnxr_camera_matrices lives with make_camera (scene_compile.cpp).  Part of api.hip's translation unit.
#pragma once

extern "C" {

int gnxr_motion_device(gnxr_scene *s, const gnxr_motion_params *p, const gnxr_camera *cameras, const gnxr_camera *prev_cameras, const float *d_prev_vertices,
                       const gnxr_motion_buffers *out, void *hip_stream) {
    if (!s || !p || !prev_cameras || !out) { set_error("motion: null argument"); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_motion_params) || out->struct_size != (int32_t)sizeof(gnxr_motion_buffers)) {
        set_error("motion: struct_size must be sizeof(gnxr_motion_params) = %zu and sizeof(gnxr_motion_buffers) = %zu", sizeof(gnxr_motion_params), sizeof(gnxr_motion_buffers));
        return GNXR_ERR_INVALID;
    }
    if (p->width < 1 || p->height < 1 || p->n_views < 0) { set_error("motion: width and height >= 1 and n_views >= 0 are required"); return GNXR_ERR_INVALID; }
    if (!cameras && p->n_views > 1) { set_error("motion: n_views = %d with null cameras (the scene's own camera is one view)", p->n_views); return GNXR_ERR_INVALID; }
    if (!out->d_motion && !out->d_guide && !out->d_prim) { set_error("motion: no channel requested"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)out->d_motion | (uintptr_t)out->d_guide) & 15u) != 0) { set_error("motion: d_motion and d_guide must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)out->d_prim | (uintptr_t)d_prev_vertices) & 3u) != 0) { set_error("motion: d_prim and d_prev_vertices must be 4-byte aligned"); return GNXR_ERR_INVALID; }
    long long total = 0;
    if (int rc = check_view_pixels(p->width, p->height, p->n_views, "motion", &total)) return rc;
    if (p->n_views == 0) return GNXR_OK;
    if (int rc = ensure_device()) return rc;
    const size_t npx = (size_t)total;
    const QueryArg args[] = {{out->d_motion, npx * 16, "d_motion"}, {out->d_guide, npx * 16, "d_guide"}, {out->d_prim, npx * 4, "d_prim"},
                             {d_prev_vertices, (size_t)s->cs.n_vertices * 12, "d_prev_vertices"}};
    DeviceCall call;
    int rc = call.bind(s, args);
    if (rc) return rc;
    gnxr_scene *r = call.r;
    const int W = p->width, H = p->height, V = p->n_views;

    std::lock_guard<std::recursive_mutex> lock(r->render_mutex);   // as the feature buffers: one render, Li, views or feature-buffer call per handle at a time
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_prev_vertices && (rc = refit_tables(r)) != GNXR_OK) return rc;   // the corner -> vertex table, uploaded as the refit uploads it
    const DScene sc = query_device_scene(r);

    std::vector<MotionView> h_views((size_t)V);
    for (int v = 0; v < V; ++v) {
        MotionView &mv = h_views[(size_t)v];
        mv.cam = cameras ? make_camera(cameras[v], W, H, -1) : make_camera(r->cs.camera, W, H, r->cs.camera_medium);
        mv.cam.lens_radius = 0.f;   // the centre ray is a pinhole's, whatever the camera says
        const DCamera prev = make_camera(prev_cameras[v], W, H, -1);
        camera_world_to_raster(prev_cameras[v], W, H, mv.w2r);
        mv.eye[0] = prev.c2w[3]; mv.eye[1] = prev.c2w[7]; mv.eye[2] = prev.c2w[11];
        mv.prev_ortho = prev.ortho;
    }
    auto pad256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t view_bytes = pad256((size_t)V * sizeof(MotionView)), ray_bytes = npx * sizeof(gnxr_ray);
    StreamScratch scratch;   // one ray per pixel: the hit's leaf code lives in the ray's pad word
    {
        const hipError_t e = scratch.alloc(view_bytes + ray_bytes, st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("motion: %zu bytes of scratch (a ray for each of %zu pixels) could not be allocated: %s", view_bytes + ray_bytes, npx, hipGetErrorString(e));
            return hip_status(e);
        }
    }
    MotionView *d_views = reinterpret_cast<MotionView *>(scratch.p);
    gnxr_ray *d_rays = reinterpret_cast<gnxr_ray *>(scratch.p + view_bytes);
    // the traversal's one-int-per-32-bytes result array starts at ray 0's pad word (api_aov.hip.h asserts the layout)
    gnxr_hit *d_codes = reinterpret_cast<gnxr_hit *>(reinterpret_cast<char *>(d_rays) + offsetof(gnxr_ray, _pad));
    // (h_views outlives the copy: the call returns after the stream has drained)
    HIP_TRY(hipMemcpyAsync(d_views, h_views.data(), (size_t)V * sizeof(MotionView), hipMemcpyHostToDevice, st));
    MotionOut mo;
    mo.motion = reinterpret_cast<float4 *>(out->d_motion); mo.guide = reinterpret_cast<float4 *>(out->d_guide); mo.prim = out->d_prim;
    const int *corner = d_prev_vertices ? (const int *)r->upd_corner.p : nullptr;
    hipLaunchKernelGGL((k_motion<0>), dim3(grid_for(total)), dim3(kBlock), 0, st, sc, (const MotionView *)d_views, W, H, (int)total, reinterpret_cast<float4 *>(d_rays),
                       corner, d_prev_vertices, mo);
    HIP_TRY(hipGetLastError());
    if ((rc = closest_hit_codes(r, sc, d_rays, total, d_codes, st)) != GNXR_OK) return rc;
    hipLaunchKernelGGL((k_motion<1>), dim3(grid_for(total)), dim3(kBlock), 0, st, sc, (const MotionView *)d_views, W, H, (int)total, reinterpret_cast<float4 *>(d_rays),
                       corner, d_prev_vertices, mo);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // the buffers are written when the call returns
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

int gnxr_temporal_accumulate_device(const gnxr_temporal_params *p, const gnxr_temporal_buffers *io, void *hip_stream) {
    if (!p || !io) { set_error("temporal accumulate: null argument"); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_temporal_params) || io->struct_size != (int32_t)sizeof(gnxr_temporal_buffers)) {
        set_error("temporal accumulate: struct_size must be sizeof(gnxr_temporal_params) = %zu and sizeof(gnxr_temporal_buffers) = %zu", sizeof(gnxr_temporal_params),
                  sizeof(gnxr_temporal_buffers));
        return GNXR_ERR_INVALID;
    }
    if (!io->d_color || !io->d_motion || !io->d_guide || !io->d_prim || !io->d_out_color || !io->d_out_stat) {
        set_error("temporal accumulate: d_color, d_motion, d_guide, d_prim, d_out_color and d_out_stat are required");
        return GNXR_ERR_INVALID;
    }
    const int n_hist = (io->d_hist_color ? 1 : 0) + (io->d_hist_stat ? 1 : 0) + (io->d_hist_guide ? 1 : 0) + (io->d_hist_prim ? 1 : 0);
    if (n_hist != 0 && n_hist != 4) { set_error("temporal accumulate: the four history pointers are all set or all null (the first frame), %d are set", n_hist); return GNXR_ERR_INVALID; }
    if (p->width < 1 || p->height < 1 || p->n_views < 0) { set_error("temporal accumulate: width and height >= 1 and n_views >= 0 are required"); return GNXR_ERR_INVALID; }
    if (p->max_history < 1) { set_error("temporal accumulate: max_history = %d is below 1", p->max_history); return GNXR_ERR_INVALID; }
    if (!(p->depth_tol >= 0.f) || p->normal_cos != p->normal_cos) { set_error("temporal accumulate: depth_tol must be >= 0 and normal_cos a number (no NaN)"); return GNXR_ERR_INVALID; }
    long long npix = 0;
    if (int rc = check_view_pixels(p->width, p->height, p->n_views, "temporal accumulate", &npix)) return rc;
    const size_t n4 = (size_t)npix * sizeof(float4), n1 = (size_t)npix * sizeof(int32_t);
    const int kArgs = 10, kInputs = 8;   // the two outputs come last
    const QueryArg args[kArgs] = {{io->d_color, n4, "d_color"}, {io->d_motion, n4, "d_motion"}, {io->d_guide, n4, "d_guide"}, {io->d_prim, n1, "d_prim"},
                                  {io->d_hist_color, n4, "d_hist_color"}, {io->d_hist_stat, n4, "d_hist_stat"}, {io->d_hist_guide, n4, "d_hist_guide"}, {io->d_hist_prim, n1, "d_hist_prim"},
                                  {io->d_out_color, n4, "d_out_color"}, {io->d_out_stat, n4, "d_out_stat"}};
    const unsigned align[kArgs] = {16u, 16u, 16u, 4u, 16u, 16u, 16u, 4u, 16u, 16u};   // the primitive ids: one int per pixel
    if (int rc = check_aligned("temporal accumulate", args, align, kArgs)) return rc;
    if (npix == 0) return GNXR_OK;
    for (int o = kInputs; o < kArgs; ++o)   // the gather reads neighbours: an output overlaps no input, nor the other output
        for (int i = 0; i < o; ++i)
            if (ranges_overlap(args[i], args[o])) { set_error("temporal accumulate: %s overlaps %s", args[o].what, args[i].what); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind("temporal accumulate", args)) return rc;
    TemporalArrays a;
    a.color = (const float4 *)io->d_color; a.motion = (const float4 *)io->d_motion; a.guide = (const float4 *)io->d_guide; a.prim = io->d_prim;
    a.hist_color = (const float4 *)io->d_hist_color; a.hist_stat = (const float4 *)io->d_hist_stat; a.hist_guide = (const float4 *)io->d_hist_guide; a.hist_prim = io->d_hist_prim;
    a.out_color = (float4 *)io->d_out_color; a.out_stat = (float4 *)io->d_out_stat;
    TemporalParams tp;
    tp.W = p->width; tp.H = p->height; tp.npix = npix;
    tp.max_history = (float)p->max_history;
    tp.depth_tol = p->depth_tol; tp.normal_cos = p->normal_cos;
    hipLaunchKernelGGL(k_temporal_accumulate, dim3(grid_for(npix)), dim3(kBlock), 0, (hipStream_t)hip_stream, a, tp);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

}  // extern "C"
