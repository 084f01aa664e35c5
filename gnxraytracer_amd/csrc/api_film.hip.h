// api_film.hip.h -- the film on device memory: gnxr_film_filter_table (host), gnxr_film_add_device, gnxr_film_resolve_device and
// gnxr_render_filtered_device (the definition: include/gnxr.h; the kernels: film_kernel.hip.h; the render path's film stages:
// RenderRun::resolve and render_one, api_render.hip.h).  Part of api.hip's translation unit (after api_query.hip.h).
#pragma once

// ---- the filter: checks and the 16 x 16 table (host code, no device) ----

static int film_check_filter(const gnxr_film_filter *f, const char *call) {
    if (!f) { set_error("%s: null filter", call); return GNXR_ERR_INVALID; }
    if (f->struct_size != (int32_t)sizeof(gnxr_film_filter)) { set_error("%s: filter.struct_size must be sizeof(gnxr_film_filter) = %zu", call, sizeof(gnxr_film_filter)); return GNXR_ERR_INVALID; }
    if (f->kind < GNXR_FILTER_BOX || f->kind > GNXR_FILTER_TABLE) { set_error("%s: unknown filter kind %d", call, f->kind); return GNXR_ERR_INVALID; }
    if (!(f->radius_x >= 0.5f && f->radius_x <= 4.f) || !(f->radius_y >= 0.5f && f->radius_y <= 4.f)) {
        set_error("%s: the filter radii must lie in [0.5, 4] (no NaN), got %g x %g", call, (double)f->radius_x, (double)f->radius_y);
        return GNXR_ERR_INVALID;
    }
    if (f->kind == GNXR_FILTER_TABLE && !f->table) { set_error("%s: GNXR_FILTER_TABLE with a null table", call); return GNXR_ERR_INVALID; }
    return GNXR_OK;
}

// pbrt-v3's Mitchell1D (filters/mitchell.h), every operation rounded on its own in the order gnxr.h writes
static float film_mitchell_1d(float t, float B, float C) {
    const float x = fabsf(2.f * t);
    if (x > 1.f) {
        const float c3 = -B - 6.f * C, c2 = 6.f * B + 30.f * C, c1 = -12.f * B - 48.f * C, c0 = 8.f * B + 24.f * C;
        return (((((c3 * x) * x) * x + ((c2 * x) * x)) + (c1 * x)) + c0) * (1.f / 6.f);
    }
    const float d3 = (12.f - 9.f * B) - 6.f * C, d2 = (-18.f + 12.f * B) + 6.f * C, d0 = 6.f - 2.f * B;
    return (((((d3 * x) * x) * x) + ((d2 * x) * x)) + d0) * (1.f / 6.f);
}
// GaussianFilter::Gaussian (GaussianFilter.h:28-32)
static float film_gaussian_1d(float d, float alpha, float e) {
    const float g = expf(((-alpha) * d) * d) - e;
    return g > 0.f ? g : 0.f;
}
static void film_table(const gnxr_film_filter &f, float *out) {
    const float rx = f.radius_x, ry = f.radius_y;
    const float expX = f.kind == GNXR_FILTER_GAUSSIAN ? expf(((-f.a) * rx) * rx) : 0.f, expY = f.kind == GNXR_FILTER_GAUSSIAN ? expf(((-f.a) * ry) * ry) : 0.f;
    for (int y = 0; y < 16; ++y) {
        for (int x = 0; x < 16; ++x) {
            const float px = (((float)x + 0.5f) * rx) / 16.f, py = (((float)y + 0.5f) * ry) / 16.f;
            float v = 1.f;
            switch (f.kind) {
            case GNXR_FILTER_TRIANGLE: {
                const float tx = rx - fabsf(px), ty = ry - fabsf(py);
                v = (tx > 0.f ? tx : 0.f) * (ty > 0.f ? ty : 0.f);
                break;
            }
            case GNXR_FILTER_GAUSSIAN: v = film_gaussian_1d(px, f.a, expX) * film_gaussian_1d(py, f.a, expY); break;
            case GNXR_FILTER_MITCHELL: v = film_mitchell_1d(px / rx, f.a, f.b) * film_mitchell_1d(py / ry, f.a, f.b); break;
            case GNXR_FILTER_TABLE: v = f.table[y * 16 + x]; break;
            default: break;
            }
            out[y * 16 + x] = v;
        }
    }
}
// what the kernels take: the radii, their reciprocals, the halo and the table
static void film_make(const gnxr_film_filter &f, FilmFilter *ff, FilmTable *tab) {
    ff->rx = f.radius_x; ff->ry = f.radius_y;
    ff->inv_rx = 1.f / f.radius_x; ff->inv_ry = 1.f / f.radius_y;
    // a sample of source pixel q sits within 0.5 of q's centre line and reaches r beyond itself: |q - p| <= ceil(r + 0.5)
    ff->hx = std::min(kFilmMaxHalo, (int)ceilf(f.radius_x + 0.5f)); ff->hy = std::min(kFilmMaxHalo, (int)ceilf(f.radius_y + 0.5f));
    film_table(f, tab->v);
}
// The arrays of a film call without a scene: each given and aligned, then -- the first step that needs the runtime -- all on one device,
// which `dc` binds
static int film_check_buffers(const char *call, const QueryArg *args, const unsigned *align, int n_args, DeviceCall *dc) {
    for (int i = 0; i < n_args; ++i) {
        if (!args[i].p) { set_error("%s: %s is null", call, args[i].what); return GNXR_ERR_INVALID; }
        if (int rc = check_aligned(call, args + i, align + i, 1)) return rc;
    }
    if (int rc = ensure_device()) return rc;
    return dc->bind(call, args, n_args);
}
static int film_check_size(const char *call, int32_t width, int32_t height, int32_t n_views, long long *npix) {
    if (width < 1 || height < 1 || n_views < 0) { set_error("%s: width and height >= 1 and n_views >= 0 are required", call); return GNXR_ERR_INVALID; }
    return check_view_pixels(width, height, n_views, call, npix);
}

extern "C" {

int gnxr_film_filter_table(const gnxr_film_filter *filter, float out[256]) {
    if (int rc = film_check_filter(filter, "film_filter_table")) return rc;
    if (!out) { set_error("film_filter_table: null out"); return GNXR_ERR_INVALID; }
    film_table(*filter, out);
    return GNXR_OK;
}

int gnxr_film_add_device(const gnxr_film_filter *filter, int32_t width, int32_t height, int32_t n_views, int32_t n_layers, const float *d_L, const float *d_offsets,
                         float *d_accum, void *hip_stream) {
    if (int rc = film_check_filter(filter, "film_add")) return rc;
    if (n_layers < 0) { set_error("film_add: n_layers = %d is negative", n_layers); return GNXR_ERR_INVALID; }
    long long npix = 0;
    if (int rc = film_check_size("film_add", width, height, n_views, &npix)) return rc;
    if (npix == 0 || n_layers == 0) return GNXR_OK;
    const size_t n = (size_t)n_layers * (size_t)npix;
    const QueryArg args[] = {{d_accum, (size_t)npix * sizeof(float4), "d_accum"}, {d_L, n * sizeof(float4), "d_L"}, {d_offsets, n * sizeof(float2), "d_offsets"}};
    const unsigned align[] = {16u, 16u, 8u};
    DeviceCall call;
    if (int rc = film_check_buffers("film_add", args, align, 3, &call)) return rc;
    for (int i = 1; i < 3; ++i)   // the accumulator is read and written while the samples are read
        if (ranges_overlap(args[0], args[i])) { set_error("film_add: d_accum overlaps %s", args[i].what); return GNXR_ERR_INVALID; }
    FilmFilter ff;
    FilmTable tab;
    film_make(*filter, &ff, &tab);
    const FilmImage im = film_image(width, height, n_views);
    DSamplerTables none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(k_film_add<false>, dim3(film_grid(im)), dim3(kBlock), 0, (hipStream_t)hip_stream, im, ff, tab, (const float4 *)d_L, (const float2 *)d_offsets, none, 0,
                       (int)n_layers, (float4 *)d_accum);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

int gnxr_film_resolve_device(int32_t width, int32_t height, int32_t n_views, const float *d_accum, float *d_rgba_out, void *hip_stream) {
    long long npix = 0;
    if (int rc = film_check_size("film_resolve", width, height, n_views, &npix)) return rc;
    if (npix == 0) return GNXR_OK;
    const size_t n4 = (size_t)npix * sizeof(float4);
    const QueryArg args[] = {{d_accum, n4, "d_accum"}, {d_rgba_out, n4, "d_rgba_out"}};
    const unsigned align[] = {16u, 16u};
    DeviceCall call;
    if (int rc = film_check_buffers("film_resolve", args, align, 2, &call)) return rc;
    if ((const void *)d_accum != (const void *)d_rgba_out && ranges_overlap(args[0], args[1])) {
        set_error("film_resolve: d_rgba_out overlaps d_accum at an offset (in place means the same address)");
        return GNXR_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_film_resolve, dim3(grid_for(npix)), dim3(kBlock), 0, (hipStream_t)hip_stream, (const float4 *)d_accum, npix, (float4 *)d_rgba_out);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

// render_one's loops with a FilmSource in place of k_resolve / k_finish, through the scene's own camera or a ViewSource
int gnxr_render_filtered_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_film_filter *filter, const gnxr_camera *cameras, const int32_t *camera_media,
                                int32_t n_views, void *d_rgba_out, float *d_accum, uint32_t flags, void *hip_stream, gnxr_stats *stats) {
    if (!s || !p) { set_error("render_filtered: null scene or params"); return GNXR_ERR_INVALID; }
    if (int rc = film_check_filter(filter, "render_filtered")) return rc;
    if (n_views < 0 || (!cameras && n_views > 1)) { set_error("render_filtered: n_views = %d with %s cameras", n_views, cameras ? "these" : "null"); return GNXR_ERR_INVALID; }
    if (flags & ~GNXR_FILM_CONTINUE) { set_error("render_filtered: unknown flag bits 0x%x", flags & ~GNXR_FILM_CONTINUE); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "render_filtered", "a filter reads its neighbours' samples: a caller that shards splits the views")) return rc;
    if (!image_and_samples_ok(*p) || p->max_depth < 0 || p->max_depth > 250) return invalid_render_params();
    if (n_views == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }
    if (!d_rgba_out && !d_accum) { set_error("render_filtered: d_rgba_out and d_accum are both null"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_rgba_out | (uintptr_t)d_accum) & 15u) != 0) { set_error("render_filtered: d_rgba_out and d_accum must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    long long total = 0;
    if (int rc = check_view_pixels(p->width, p->height, n_views, "render_filtered", &total)) return rc;
    if (int rc = ensure_device()) return rc;
    if (!cameras) camera_media = nullptr;   // the scene's own camera sits in the scene's camera medium
    if (int rc = check_view_media(s, camera_media, n_views, "render_filtered")) return rc;
    const size_t n4 = (size_t)total * sizeof(float4);
    const QueryArg args[] = {{d_rgba_out, n4, "d_rgba_out"}, {d_accum, n4, "d_accum"}};
    if (ranges_overlap(args[0], args[1])) { set_error("render_filtered: d_rgba_out overlaps d_accum"); return GNXR_ERR_INVALID; }
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    FilmSource film;
    film_make(*filter, &film.f, &film.tab);
    film.accum = reinterpret_cast<float4 *>(d_accum);
    film.keep = d_accum && (flags & GNXR_FILM_CONTINUE) != 0;
    const ViewSource vs{cameras, camera_media, (int)n_views};
    return render_one(call.r, &pp, d_rgba_out, hip_stream, stats, /*reserve_only=*/false, nullptr, cameras ? &vs : nullptr, nullptr, &film);
}

}  // extern "C"
