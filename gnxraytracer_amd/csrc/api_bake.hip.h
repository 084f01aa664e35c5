// api_bake.hip.h -- lightmap baking on device memory: gnxr_bake_texels_device, gnxr_surface_rays_device, gnxr_bake_dilate_device and
// gnxr_bake_lightmap_device (the definition: include/gnxr.h; the kernels: bake_kernel.hip.h).  The bake is the texture-space front end of
// Li: it rasterises the atlas, lists the covered texels and feeds sub-batches of surface rays through render_one's caller-ray loops
// (api_render.hip.h), as gnxr_li_device does.  Part of api.hip's translation unit (after api_query.hip.h).
#pragma once

// texels of an atlas: a texel index and the covered-texel list are ints
static const long long kBakeMaxTexels = 1ll << 30;
// Rays of an automatic sub-batch of a bake: Li's own automatic sub-pass (64 bytes of scratch each: ray, sample record, L; 4 GB at the
// most).  A sub-batch is one Li call, which drains before the next starts; measured on cfg 3 (1024^2 x 64 spp, 66.9 M paths,
// profiles/README.md): 16 M per batch costs 9 % over one Li call on the same rays, everything around Li 1.3 %.
static const long long kBakeBatchRays = kSubPassPaths;

static int bake_atlas_ok(const char *call, int32_t width, int32_t height) {
    if (width > 0 && height > 0 && (long long)width * height <= kBakeMaxTexels) return GNXR_OK;
    set_error("%s: the atlas must be at least 1 x 1 and at most %lld texels, got %d x %d", call, kBakeMaxTexels, width, height);
    return GNXR_ERR_INVALID;
}

// the sampler tables of a copy of the scene for a HaltonSampler over [0, W) x [0, H) (they never change after the scene is created)
static DSamplerTables bake_sampler_tables(const gnxr_scene *r, int W, int H) {
    DSamplerTables st;
    st.perms = r->perms.p; st.primes = r->primes.p; st.prime_sums = r->prime_sums.p; st.prime_magic = r->prime_magic.p;
    st.h = make_halton(W, H);
    return st;
}

// rasterisation on `st`: texel_tri (n_texels ints) and, when wanted, bary (n_texels float2)
static int bake_rasterise(const float *d_lm_uv, int n_tris, int W, int H, int *texel_tri, float2 *bary, hipStream_t st) {
    const long long n_texels = (long long)W * H;
    HIP_TRY(hipMemsetAsync(texel_tri, 0xff, (size_t)n_texels * sizeof(int), st));
    if (n_tris > 0) hipLaunchKernelGGL(k_bake_raster, dim3(grid_for((long long)n_tris * 64)), dim3(kBlock), 0, st, d_lm_uv, n_tris, W, H, (unsigned int *)texel_tri);
    if (bary) hipLaunchKernelGGL(k_bake_bary, dim3(grid_for(n_texels)), dim3(kBlock), 0, st, d_lm_uv, (const int *)texel_tri, W, n_texels, bary);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

// authoring index -> leaf index, from the triangles on the (bound) device
static int bake_leaf_of(const gnxr_scene *r, int n_tris, int *leaf_of, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(leaf_of, 0, (size_t)std::max(1, n_tris) * sizeof(int), st));
    if (n_tris > 0) hipLaunchKernelGGL(k_bake_leaf_of, dim3(grid_for(n_tris)), dim3(kBlock), 0, st, (const DTri *)r->tris.p, n_tris, leaf_of);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

// `iterations` dilation passes over img (n_texels float4) on `st`; scratch: a second image and two byte masks
static int bake_dilate(float4 *img, int W, int H, int iterations, hipStream_t st) {
    if (iterations <= 0) return GNXR_OK;
    const long long n_texels = (long long)W * H;
    const size_t mask_bytes = ((size_t)n_texels + 15) & ~(size_t)15;
    StreamScratch scratch;
    HIP_TRY(scratch.alloc((size_t)n_texels * sizeof(float4) + 2 * mask_bytes, st));
    float4 *image[2] = {img, (float4 *)scratch.p};
    unsigned char *mask[2] = {(unsigned char *)scratch.p + (size_t)n_texels * sizeof(float4), (unsigned char *)scratch.p + (size_t)n_texels * sizeof(float4) + mask_bytes};
    const int grid = grid_for(n_texels);
    hipLaunchKernelGGL(k_bake_mask, dim3(grid), dim3(kBlock), 0, st, (const float4 *)img, n_texels, mask[0]);
    for (int i = 0; i < iterations; ++i)
        hipLaunchKernelGGL(k_bake_dilate, dim3(grid), dim3(kBlock), 0, st, (const float4 *)image[i & 1], (const unsigned char *)mask[i & 1], W, H, image[1 - (i & 1)], mask[1 - (i & 1)]);
    HIP_TRY(hipGetLastError());
    if (iterations & 1) HIP_TRY(hipMemcpyAsync(img, image[1], (size_t)n_texels * sizeof(float4), hipMemcpyDeviceToDevice, st));
    return GNXR_OK;
}

// the counters of a bake's Li calls, added up
static void bake_add_stats(gnxr_stats *sum, const gnxr_stats &t) {
    sum->rays_closest += t.rays_closest; sum->rays_any += t.rays_any; sum->camera_samples += t.camera_samples;
    sum->nodes_visited += t.nodes_visited; sum->tris_tested += t.tris_tested; sum->kernel_launches += t.kernel_launches;
    sum->rays_closest_nee += t.rays_closest_nee; sum->media_segments += t.media_segments; sum->media_steps += t.media_steps; sum->leaf_retests += t.leaf_retests;
    sum->nodes_from_memory += t.nodes_from_memory;
    sum->seconds_render += t.seconds_render; sum->seconds_total += t.seconds_total;
    sum->seconds_closest += t.seconds_closest; sum->seconds_nee += t.seconds_nee; sum->seconds_shade += t.seconds_shade; sum->seconds_trace += t.seconds_trace;
    sum->launches_closest += t.launches_closest; sum->launches_nee += t.launches_nee;
    sum->passes += t.passes; sum->loop_iterations += t.loop_iterations;
    sum->passes_in_flight = std::max(sum->passes_in_flight, t.passes_in_flight);
    sum->state_bytes = std::max(sum->state_bytes, t.state_bytes);
}

extern "C" {

int gnxr_bake_texels_device(gnxr_scene *s, const float *d_tri_lm_uv, int32_t width, int32_t height, int32_t *d_texel_tri, float *d_texel_bary, void *hip_stream) {
    if (!s || !d_tri_lm_uv || !d_texel_tri) { set_error("gnxr_bake_texels_device: null argument"); return GNXR_ERR_INVALID; }
    if (int rc = bake_atlas_ok("gnxr_bake_texels_device", width, height)) return rc;
    if ((((uintptr_t)d_tri_lm_uv | (uintptr_t)d_texel_tri) & 3u) != 0 || ((uintptr_t)d_texel_bary & 7u) != 0) {
        set_error("gnxr_bake_texels_device: d_tri_lm_uv and d_texel_tri must be 4-byte aligned, d_texel_bary 8-byte aligned");
        return GNXR_ERR_INVALID;
    }
    if (int rc = ensure_device()) return rc;
    const int n_tris = (int)s->cs.n_triangles;
    const size_t n_texels = (size_t)width * height;
    const QueryArg args[] = {{d_tri_lm_uv, (size_t)std::max(1, n_tris) * 24, "d_tri_lm_uv"}, {d_texel_tri, n_texels * 4, "d_texel_tri"}, {d_texel_bary, n_texels * 8, "d_texel_bary"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    return bake_rasterise(d_tri_lm_uv, n_tris, width, height, d_texel_tri, (float2 *)d_texel_bary, (hipStream_t)hip_stream);
}

int gnxr_surface_rays_device(gnxr_scene *s, int32_t width, int32_t height, const int32_t *d_tri, const float *d_bary, const int32_t *d_px, const int32_t *d_py,
                             const int32_t *d_s, int64_t n, uint32_t flags, int32_t medium, gnxr_ray *d_rays, gnxr_li_sample *d_samples, float *d_pn, void *hip_stream) {
    if (!s || n < 0 || width <= 0 || height <= 0 || (n > 0 && (!d_tri || !d_bary || !d_px || !d_py || !d_s || !d_rays || !d_samples))) {
        set_error("gnxr_surface_rays_device: bad argument");
        return GNXR_ERR_INVALID;
    }
    if (flags & ~GNXR_BAKE_FLIP_NORMALS) { set_error("gnxr_surface_rays_device: unknown flag bits 0x%x", flags & ~GNXR_BAKE_FLIP_NORMALS); return GNXR_ERR_INVALID; }
    if (medium < -1 || medium >= (int32_t)s->cs.media.size()) { set_error("gnxr_surface_rays_device: medium = %d is outside [-1, %d)", medium, (int)s->cs.media.size()); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if ((((uintptr_t)d_rays | (uintptr_t)d_samples | (uintptr_t)d_pn) & 15u) != 0) { set_error("gnxr_surface_rays_device: d_rays, d_samples and d_pn must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_bary & 7u) != 0 || (((uintptr_t)d_tri | (uintptr_t)d_px | (uintptr_t)d_py | (uintptr_t)d_s) & 3u) != 0) {
        set_error("gnxr_surface_rays_device: d_bary must be 8-byte aligned, d_tri, d_px, d_py and d_s 4-byte aligned");
        return GNXR_ERR_INVALID;
    }
    if (int rc = ensure_device()) return rc;
    const QueryArg args[] = {{d_tri, (size_t)n * 4, "d_tri"}, {d_bary, (size_t)n * 8, "d_bary"}, {d_px, (size_t)n * 4, "d_px"}, {d_py, (size_t)n * 4, "d_py"}, {d_s, (size_t)n * 4, "d_s"},
                             {d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_samples, (size_t)n * sizeof(gnxr_li_sample), "d_samples"}, {d_pn, (size_t)n * 32, "d_pn"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    std::lock_guard<std::recursive_mutex> lock(r->render_mutex);   // the triangles are what the editing calls and the rebuild rewrite
    const int n_tris = (int)r->cs.n_triangles;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamScratch scratch;   // [status word | pad to 16 B | leaf_of]
    HIP_TRY(scratch.alloc(16 + (size_t)std::max(1, n_tris) * sizeof(int), stream));
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(scratch.p), bad = 0;
    int *leaf_of = reinterpret_cast<int *>(scratch.p + 16);
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), stream));
    if (int rc = bake_leaf_of(r, n_tris, leaf_of, stream)) return rc;
    hipLaunchKernelGGL(k_surface_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, (const DTri *)r->tris.p, (const int *)leaf_of, n_tris, bake_sampler_tables(r, width, height),
                       (int)width, (int)height, (const int *)d_tri, (const float2 *)d_bary, (const int *)d_px, (const int *)d_py, (const int *)d_s, (long long)n,
                       (int)((flags & GNXR_BAKE_FLIP_NORMALS) != 0), (int)medium, reinterpret_cast<float4 *>(d_rays), reinterpret_cast<int4 *>(d_samples),
                       reinterpret_cast<float4 *>(d_pn), d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // only the status word has to come back: the records are on the stream
    if (bad) {
        set_error("gnxr_surface_rays_device: record %llu is out of range (triangle in [0, %d), px in [0, %d), py in [0, %d), s >= 0); its ray and sample are 0",
                  (unsigned long long)~bad, n_tris, width, height);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

// No scene: the device is the one that holds the image, as for gnxr_denoise_device.
int gnxr_bake_dilate_device(int32_t width, int32_t height, int32_t iterations, float *d_rgba, void *hip_stream) {
    if (!d_rgba || iterations < 0) { set_error("gnxr_bake_dilate_device: null image or iterations < 0"); return GNXR_ERR_INVALID; }
    if (int rc = bake_atlas_ok("gnxr_bake_dilate_device", width, height)) return rc;
    if (((uintptr_t)d_rgba & 15u) != 0) { set_error("gnxr_bake_dilate_device: d_rgba is not 16-byte aligned"); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    const QueryArg args[] = {{d_rgba, (size_t)width * height * sizeof(float4), "d_rgba"}};
    DeviceCall call;
    if (int rc = call.bind("gnxr_bake_dilate_device", args)) return rc;
    return bake_dilate((float4 *)d_rgba, width, height, iterations, (hipStream_t)hip_stream);
}

int gnxr_bake_lightmap_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_bake_params *bake, const float *d_tri_lm_uv, void *d_rgba_out, void *hip_stream,
                              gnxr_stats *stats) {
    if (!s || !p || !bake || !d_tri_lm_uv || !d_rgba_out) { set_error("gnxr_bake_lightmap_device: null argument"); return GNXR_ERR_INVALID; }
    if (bake->struct_size != (int32_t)sizeof(gnxr_bake_params)) { set_error("gnxr_bake_lightmap_device: struct_size must be sizeof(gnxr_bake_params) = %zu", sizeof(gnxr_bake_params)); return GNXR_ERR_INVALID; }
    if (bake->flags & ~GNXR_BAKE_FLIP_NORMALS) { set_error("gnxr_bake_lightmap_device: unknown flag bits 0x%x", bake->flags & ~GNXR_BAKE_FLIP_NORMALS); return GNXR_ERR_INVALID; }
    if (bake->dilate < 0) { set_error("gnxr_bake_lightmap_device: dilate = %d is negative", bake->dilate); return GNXR_ERR_INVALID; }
    if (bake->medium < -1 || bake->medium >= (int32_t)s->cs.media.size()) { set_error("gnxr_bake_lightmap_device: medium = %d is outside [-1, %d)", bake->medium, (int)s->cs.media.size()); return GNXR_ERR_INVALID; }
    if (int rc = bake_atlas_ok("gnxr_bake_lightmap_device", p->width, p->height)) return rc;
    if (p->spp_begin != 0 || p->spp_end != 0) { set_error("gnxr_bake_lightmap_device: spp_begin and spp_end must be 0 (a bake takes all samples of a texel)"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "gnxr_bake_lightmap_device", "a caller that shards splits the atlas")) return rc;
    if (((uintptr_t)d_tri_lm_uv & 3u) != 0 || ((uintptr_t)d_rgba_out & 15u) != 0) { set_error("gnxr_bake_lightmap_device: d_tri_lm_uv must be 4-byte aligned, d_rgba_out 16-byte aligned"); return GNXR_ERR_INVALID; }
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    {   // the parameters and the support matrix of Li for caller rays, before anything is queued
        const RaySource probe{nullptr, nullptr, nullptr, 1};
        RenderPlan pl;
        if (int rc = plan_render(s->cs, &pp, &probe, nullptr, nullptr, &pl)) return rc;
        DHalton h = make_halton(pp.width, pp.height);
        if (int rc = halton_index_bound(&h, pp.spp, pl.max_light_samples)) return rc;
    }
    if (int rc = ensure_device()) return rc;
    const int W = p->width, H = p->height, spp = p->spp;
    const long long n_texels = (long long)W * H;
    const int n_tris = (int)s->cs.n_triangles;
    const QueryArg args[] = {{d_tri_lm_uv, (size_t)std::max(1, n_tris) * 24, "d_tri_lm_uv"}, {d_rgba_out, (size_t)n_texels * sizeof(float4), "d_rgba_out"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_scene *r = call.r;
    std::lock_guard<std::recursive_mutex> lock(r->render_mutex);   // held across the sub-batches: one bake, render or Li call per copy at a time
    hipStream_t stream = (hipStream_t)hip_stream;
    float4 *out = (float4 *)d_rgba_out;
    if (stats) memset(stats, 0, sizeof(*stats));

    // ---- the atlas: winner and barycentrics per texel, the covered texels in texel order
    const int n_tiles = (int)((n_texels + kBlock - 1) / kBlock);
    const size_t texel_bytes = ((size_t)n_texels * sizeof(int) + 15) & ~(size_t)15, tile_bytes = ((size_t)(n_tiles + 1) * sizeof(int) + 15) & ~(size_t)15;
    const size_t tri_bytes = ((size_t)std::max(1, n_tris) * sizeof(int) + 15) & ~(size_t)15;
    StreamScratch atlas;   // [texel_tri | bary | list | counts | offsets | leaf_of]
    HIP_TRY(atlas.alloc(4 * texel_bytes + 2 * tile_bytes + tri_bytes, stream));
    int *texel_tri = (int *)atlas.p, *list = (int *)(atlas.p + 3 * texel_bytes);
    float2 *bary = (float2 *)(atlas.p + texel_bytes);
    int *counts = (int *)(atlas.p + 4 * texel_bytes), *offsets = (int *)(atlas.p + 4 * texel_bytes + tile_bytes), *leaf_of = (int *)(atlas.p + 4 * texel_bytes + 2 * tile_bytes);
    if (int rc = bake_rasterise(d_tri_lm_uv, n_tris, W, H, texel_tri, bary, stream)) return rc;
    if (int rc = bake_leaf_of(r, n_tris, leaf_of, stream)) return rc;
    const int tile_grid = (int)std::min<long long>(n_tiles, (long long)g_num_cus * g_grid_bpc);
    hipLaunchKernelGGL(k_bake_count, dim3(tile_grid), dim3(kBlock), 0, stream, (const int *)texel_tri, n_texels, n_tiles, counts);
    hipLaunchKernelGGL(k_bake_scan, dim3(1), dim3(kBlock), 0, stream, (const int *)counts, n_tiles, offsets);
    hipLaunchKernelGGL(k_bake_scatter, dim3(tile_grid), dim3(kBlock), 0, stream, (const int *)texel_tri, n_texels, n_tiles, (const int *)offsets, list);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_texels * sizeof(float4), stream));
    int n_covered = 0;
    HIP_TRY(hipMemcpyAsync(&n_covered, offsets + n_tiles, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the sub-batches are sized by the number of covered texels

    // ---- Li in sub-batches: whole layers of samples while a layer fits a batch, else ranges of one layer's texels
    if (n_covered > 0) {
        const long long batch = pp.samples_per_pass > 0 ? (long long)pp.samples_per_pass : kBakeBatchRays;
        const int layers = (int)std::max<long long>(1, std::min<long long>(spp, batch / n_covered));
        const int texels = (int)std::min<long long>(n_covered, batch);
        const size_t cap = (size_t)layers * texels;
        StreamScratch sub;   // [rays | samples | L] of one sub-batch
        HIP_TRY(sub.alloc(cap * (sizeof(gnxr_ray) + sizeof(gnxr_li_sample) + sizeof(float4)), stream));
        gnxr_ray *rays = (gnxr_ray *)sub.p;
        gnxr_li_sample *samples = (gnxr_li_sample *)(sub.p + cap * sizeof(gnxr_ray));
        float *L = (float *)(sub.p + cap * (sizeof(gnxr_ray) + sizeof(gnxr_li_sample)));
        const DSamplerTables st = bake_sampler_tables(r, W, H);
        const int flip = (bake->flags & GNXR_BAKE_FLIP_NORMALS) != 0;
        for (int s0 = 0; s0 < spp; s0 += layers) {
            const int ns = std::min(layers, spp - s0);
            for (int k0 = 0; k0 < n_covered; k0 += texels) {
                const int nk = std::min(texels, n_covered - k0);
                const long long n = (long long)ns * nk;
                hipLaunchKernelGGL(k_bake_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, (const DTri *)r->tris.p, (const int *)leaf_of, st, W, (const int *)texel_tri,
                                   (const float2 *)bary, (const int *)list, k0, nk, s0, n, flip, (int)bake->medium, reinterpret_cast<float4 *>(rays), reinterpret_cast<int4 *>(samples));
                HIP_TRY(hipGetLastError());
                const RaySource src{rays, samples, L, n};
                gnxr_stats t;
                memset(&t, 0, sizeof(t));
                if (int rc = render_one(r, &pp, nullptr, hip_stream, &t, /*reserve_only=*/false, &src)) return rc;
                if (stats) bake_add_stats(stats, t);
                hipLaunchKernelGGL(k_bake_accum, dim3(grid_for(nk)), dim3(kBlock), 0, stream, (const float4 *)L, reinterpret_cast<const float4 *>(rays), (const int *)list, k0, nk,
                                   ns, out);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    hipLaunchKernelGGL(k_bake_finish, dim3(grid_for(n_texels)), dim3(kBlock), 0, stream, (const int *)texel_tri, n_texels, spp, out);
    HIP_TRY(hipGetLastError());
    if (int rc = bake_dilate(out, W, H, bake->dilate, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(stream));   // back when the lightmap is written, as gnxr_li_device is when d_L is
    return GNXR_OK;
}

}  // extern "C"
