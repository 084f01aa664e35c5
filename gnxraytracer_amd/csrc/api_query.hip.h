// api_query.hip.h -- the entry points on device memory: batched ray queries, Li for caller rays, views, shading queries.
// Part of api.hip's translation unit (after api_render.hip.h; the calls' front end -- replica choice, scratch, parameter checks -- is api_device_call.hip.h).
#pragma once

extern "C" {

// ---- batched queries on device memory: gnxr_trace_closest_device / gnxr_trace_any_device ----
// k_trace4 in its query modes (query_kernel.hip.h) on the caller's stream.  Nothing of the handle's render state is touched: the chunk
// cursor and the global part of the traversal stack come from the stream-ordered allocator on the caller's stream (allocated, used and
// freed in stream order; their size depends on the scene and the grid, never on n), so queries on several streams and a render in
// flight on another stream never share scratch.

// work items per k_trace4 launch: the kernel counts them in 32 bits (chunk_plan / chunk_range) and keeps a ray's index in an int
static const long long kQueryLaunchMax = 1ll << 30;

// the tables the walk, the hit record and a BSDF read (device_scene() would also read the light and sampler state, which a render may be rebuilding)
static DScene query_device_scene(gnxr_scene *r) {
    const SceneFacts &cs = r->cs;
    DScene sc = {};
    sc.nodes = reinterpret_cast<const float4 *>(r->nodes.p);
    sc.nodes4 = reinterpret_cast<const float4 *>(r->nodes4.p);
    sc.root4 = cs.root4;
    sc.tris = r->tris.p;
    sc.leaf_box = reinterpret_cast<const float4 *>(r->leaf_boxes.p);
    sc.leaf1_from_verts = (cs.leaf1_from_verts && !Knobs::leaf_box_table()) ? 1 : 0;   // as device_scene()
    sc.spheres = r->spheres.p;
    sc.n_spheres = cs.n_spheres;
    sc.materials = r->materials.p + 1;
    return sc;
}

// k_trace4 in a query mode over n rays on `st`, with the call's own scratch.  any == false: the leaf code of every ray's closest hit into
// hits[i].prim (kT4QueryClosest); any == true: occluded[i].  Scenes on the 4-wide tree only (r->wide_ok).
static int query_trace4(gnxr_scene *r, const DScene &sc, const gnxr_ray *d_rays, int64_t n, gnxr_hit *hits, unsigned char *occluded, bool any, hipStream_t st) {
    const bool spheres = r->cs.n_spheres > 0;
    // scratch of this call: [cursor | pad to 256 B | spill columns of the grid the largest launch uses]
    const TraceLaunch tl = trace_launch(r, true, spheres, std::min<long long>(n, kQueryLaunchMax));
    const size_t spill_ints = tl.spill_needed ? (size_t)(tl.entries - tl.lds_entries) * (size_t)tl.blocks * kBlock : 0;
    StreamScratch scratch;
    HIP_TRY(scratch.alloc(256 + spill_ints * sizeof(int), st));
    unsigned int *cursor = reinterpret_cast<unsigned int *>(scratch.p);
    int *spill = reinterpret_cast<int *>(scratch.p + 256);
    for (long long base = 0; base < n; base += kQueryLaunchMax) {
        const long long cnt = std::min<long long>(n - base, kQueryLaunchMax);
        const TraceLaunch t = trace_launch(r, true, spheres, cnt);
        QueryArrays qa;
        qa.rays = reinterpret_cast<const float4 *>(d_rays + base);
        qa.hits = any ? nullptr : hits + base;
        qa.occluded = any ? occluded + base : nullptr;
        TraceWork w = {};
        w.n_closest = (int)cnt;
        HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(unsigned int), st));
#define GX_QUERY4(S, P, Q) hipLaunchKernelGGL((k_trace4<false, S, P, Q>), dim3(t.blocks), dim3(kBlock), t.lds, st, sc, qa, w, cursor, (Counters *)nullptr, t.lds_entries, spill, kTraceChunk, t.n_top, t.hot_bytes)
#define GX_QUERY4_SP(Q) do { if (spheres) { if (t.spill_needed) GX_QUERY4(true, true, Q); else GX_QUERY4(true, false, Q); } \
                             else { if (t.spill_needed) GX_QUERY4(false, true, Q); else GX_QUERY4(false, false, Q); } } while (0)
        if (any) GX_QUERY4_SP(kT4QueryAny);
        else GX_QUERY4_SP(kT4QueryClosest);
#undef GX_QUERY4_SP
#undef GX_QUERY4
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

// The leaf code of every ray's closest hit into codes[i].prim, for the calls that shade what the rays hit: k_trace4's closest-hit query
// on the 4-wide tree, else the binary walk (64 stack entries at 2 blocks per CU, 32 at 5).
static int closest_hit_codes(gnxr_scene *r, const DScene &sc, const gnxr_ray *d_rays, long long n, gnxr_hit *codes, hipStream_t st) {
    if (r->wide_ok) return query_trace4(r, sc, d_rays, n, codes, nullptr, false, st);
    if (r->stack_size > 32) hipLaunchKernelGGL((k_trace_closest_code<64>), dim3(grid_for(n, 2)), dim3(kBlock), 0, st, sc, d_rays, n, codes);
    else hipLaunchKernelGGL((k_trace_closest_code<32>), dim3(grid_for(n, 5)), dim3(kBlock), 0, st, sc, d_rays, n, codes);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

// any == false: Scene::Intersect, out = gnxr_hit[n]; any == true: Scene::IntersectP, out = uint8_t[n]
static int trace_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, void *out, void *hip_stream, bool any) {
    if (!s || n < 0 || (n > 0 && (!d_rays || !out))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_rays & 15u) != 0) { set_error("d_rays is not 16-byte aligned (two dwordx4 loads per ray)"); return GNXR_ERR_INVALID; }
    if (!any && ((uintptr_t)out & 3u) != 0) { set_error("d_hits is not 4-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {out, (size_t)n * (!any ? sizeof(gnxr_hit) : 1), !any ? "d_hits" : "d_occluded"}};
    DeviceCall call;
    int rc = call.bind(s, args);
    if (rc) return rc;
    gnxr_scene *r = call.r;
    hipStream_t st = (hipStream_t)hip_stream;
    const DScene sc = query_device_scene(r);
    if (!r->wide_ok) return binary_trace_api(r, sc, d_rays, n, out, any, st);   // same results
    if ((rc = query_trace4(r, sc, d_rays, n, any ? nullptr : (gnxr_hit *)out, any ? (unsigned char *)out : nullptr, any, st)) != GNXR_OK) return rc;
    if (!any) {
        hipLaunchKernelGGL(k_query_finish, dim3(grid_for(n)), dim3(kBlock), 0, st, sc, reinterpret_cast<const float4 *>(d_rays), (long long)n, (gnxr_hit *)out);
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}
int gnxr_trace_closest_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, gnxr_hit *d_hits, void *hip_stream) {
    return trace_device(s, d_rays, n, d_hits, hip_stream, false);
}
int gnxr_trace_any_device(gnxr_scene *s, const gnxr_ray *d_rays, int64_t n, uint8_t *d_occluded, void *hip_stream) {
    return trace_device(s, d_rays, n, d_occluded, hip_stream, true);
}

// ---- SamplerIntegrator::Li for caller rays on device memory: gnxr_li_device ----
// render_one's loops (api_render.hip.h) with a RaySource in place of the camera and the image (li_kernel.hip.h), on the copy of the scene that holds the arrays.
int gnxr_li_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_ray *d_rays, const gnxr_li_sample *d_samples, int64_t n, float *d_L, void *hip_stream,
                   gnxr_stats *stats) {
    if (int rc = ensure_device()) return rc;
    if (!s || !p || n < 0 || (n > 0 && (!d_rays || !d_samples || !d_L))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (p->spp_begin != 0 || p->spp_end != 0) { set_error("Li for caller rays: spp_begin and spp_end must be 0 (the records name each ray's sample)"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "Li for caller rays", "the records name each ray's sample")) return rc;
    if (n == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }
    if ((((uintptr_t)d_rays | (uintptr_t)d_samples | (uintptr_t)d_L) & 15u) != 0) { set_error("d_rays, d_samples and d_L must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_samples, (size_t)n * sizeof(gnxr_li_sample), "d_samples"}, {d_L, (size_t)n * 4 * sizeof(float), "d_L"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    const RaySource src{d_rays, d_samples, d_L, (long long)n};
    return render_one(call.r, &pp, nullptr, hip_stream, stats, /*reserve_only=*/false, &src);
}

// ---- many cameras in one render on device memory: gnxr_render_views_device ----
// render_one's loops (api_render.hip.h) with a ViewSource in place of the scene's camera (views_kernel.hip.h), on the copy of the scene that holds the images.
int gnxr_render_views_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_camera *cameras, const int32_t *camera_media, int32_t n_views, void *d_rgba_out,
                             void *hip_stream, gnxr_stats *stats) {
    if (!s || !p || n_views < 0 || (n_views > 0 && !cameras)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "views", "a caller that shards splits the list of views")) return rc;
    if (!image_and_samples_ok(*p) || p->max_depth < 0 || p->max_depth > 250) return invalid_render_params();
    if (n_views == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }
    if (!d_rgba_out || ((uintptr_t)d_rgba_out & 15u) != 0) { set_error("d_rgba_out is null or not 16-byte aligned"); return GNXR_ERR_INVALID; }
    long long total = 0;
    if (int rc = check_view_pixels(p->width, p->height, n_views, "views", &total)) return rc;
    if (int rc = ensure_device()) return rc;
    if (int rc = check_view_media(s, camera_media, n_views, "views")) return rc;
    const QueryArg args[] = {{d_rgba_out, (size_t)total * sizeof(float4), "d_rgba_out"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    const ViewSource vs{cameras, camera_media, (int)n_views};
    return render_one(call.r, &pp, d_rgba_out, hip_stream, stats, /*reserve_only=*/false, nullptr, &vs);
}

// ---- shading queries on device memory: gnxr_bsdf_device / gnxr_light_sample_device / gnxr_light_le_device (shade_query_kernel.hip.h) ----

// rays of one traversal + k_bsdf_query round: bounds the call's scratch (one gnxr_hit per ray for the leaf codes) at 128 MB whatever n is
static const long long kBsdfQueryChunk = 1ll << 22;

int gnxr_bsdf_device(gnxr_scene *s, const gnxr_ray *d_rays, const float *d_wi, const float *d_u, const float *d_differentials, int64_t n, int32_t flags,
                     gnxr_bsdf_result *d_out, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_rays || !d_wi || !d_u || !d_out))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (flags < 0 || flags > 31) { set_error("flags = %d is not a BxDFType mask (0 .. BSDF_ALL = 31)", flags); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if ((((uintptr_t)d_rays | (uintptr_t)d_out) & 15u) != 0) { set_error("d_rays and d_out must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_wi | (uintptr_t)d_u | (uintptr_t)d_differentials) & 3u) != 0) { set_error("d_wi, d_u and d_differentials must be 4-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_wi, (size_t)n * 12, "d_wi"}, {d_u, (size_t)n * 8, "d_u"},
                             {d_differentials, (size_t)n * 48, "d_differentials"}, {d_out, (size_t)n * sizeof(gnxr_bsdf_result), "d_out"}};
    if (int drc = ensure_device()) return drc;
    DeviceCall call;
    int rc = call.bind(s, args);
    if (rc) return rc;
    gnxr_scene *r = call.r;
    hipStream_t st = (hipStream_t)hip_stream;
    const DScene sc = query_device_scene(r);
    StreamScratch scratch;
    HIP_TRY(scratch.alloc((size_t)std::min<long long>(n, kBsdfQueryChunk) * sizeof(gnxr_hit), st));
    gnxr_hit *codes = reinterpret_cast<gnxr_hit *>(scratch.p);
    for (long long base = 0; base < n; base += kBsdfQueryChunk) {
        const long long cnt = std::min<long long>(n - base, kBsdfQueryChunk);
        if ((rc = closest_hit_codes(r, sc, d_rays + base, cnt, codes, st)) != GNXR_OK) return rc;
        BsdfQueryArrays q;
        q.rays = reinterpret_cast<const float4 *>(d_rays + base);
        q.codes = codes;
        q.wi = d_wi + 3 * base;
        q.u = d_u + 2 * base;
        q.diffs = d_differentials ? d_differentials + 12 * base : nullptr;
        q.out = reinterpret_cast<float4 *>(d_out + base);
        hipLaunchKernelGGL((k_bsdf_query<LM_ALL>), dim3(grid_for(cnt)), dim3(kBlock), 0, st, sc, q, cnt, (int)flags);
        HIP_TRY(hipGetLastError());
    }
    return GNXR_OK;
}

// the light tables of `r` with the selection table of `strategy`: the render's cache (ensure_grid), under the render lock
static int query_light_tables(gnxr_scene *r, int32_t strategy, DLightTables *lt) {
    if (int rc = r->ensure_grid(strategy)) return rc;
    *lt = r->device_scene(1, 1).lt;
    return GNXR_OK;
}

int gnxr_light_sample_device(gnxr_scene *s, const float *d_queries, int64_t n, int32_t strategy, gnxr_light_result *d_out, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_queries || !d_out))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (strategy != GNXR_LIGHTS_SPATIAL && strategy != GNXR_LIGHTS_UNIFORM && strategy != GNXR_LIGHTS_POWER) {
        set_error("strategy = %d is not a gnxr_light_strategy", strategy);
        return GNXR_ERR_INVALID;
    }
    if (n == 0) return GNXR_OK;
    if ((((uintptr_t)d_queries | (uintptr_t)d_out) & 15u) != 0) { set_error("d_queries and d_out must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_queries, (size_t)n * 48, "d_queries"}, {d_out, (size_t)n * sizeof(gnxr_light_result), "d_out"}};
    if (int drc = ensure_device()) return drc;
    DeviceCall call;
    int rc = call.bind(s, args);
    if (rc) return rc;
    gnxr_scene *r = call.r;
    // the selection table belongs to the renders of the copy it lives on: both locks, in DeviceCall's order
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    std::lock_guard<std::recursive_mutex> lock_r(r->render_mutex);
    hipStream_t st = (hipStream_t)hip_stream;
    DLightTables lt;
    if ((rc = query_light_tables(r, strategy, &lt)) != GNXR_OK) return rc;
    StatusWord status;
    unsigned long long bad = 0;
    if ((rc = status.alloc(st)) != GNXR_OK) return rc;
    hipLaunchKernelGGL((k_light_sample_query<LT_ALL>), dim3(grid_for(n)), dim3(kBlock), 0, st, lt, reinterpret_cast<const float4 *>(d_queries), (long long)n,
                       reinterpret_cast<float4 *>(d_out), status.d);
    HIP_TRY(hipGetLastError());
    if ((rc = status.fetch(&bad)) != GNXR_OK) return rc;
    if (bad) {
        set_error("gnxr_light_sample_device: query %llu names a light outside [0, %d); its record is 0", (unsigned long long)~bad, lt.n_lights);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

int gnxr_light_le_device(gnxr_scene *s, int32_t light, const gnxr_ray *d_rays, int64_t n, float *d_le, void *hip_stream) {
    if (!s || n < 0 || (n > 0 && (!d_rays || !d_le))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (light < 0 || light >= (int32_t)s->cs.desc_lights.size()) { set_error("light = %d is outside [0, %d)", light, (int)s->cs.desc_lights.size()); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_le & 3u) != 0) { set_error("d_rays must be 16-byte aligned, d_le 4-byte aligned"); return GNXR_ERR_INVALID; }
    const QueryArg args[] = {{d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"}, {d_le, (size_t)n * 12, "d_le"}};
    if (int drc = ensure_device()) return drc;
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    const gnxr_scene *r = call.r;
    // Le reads the lights and the environment map, not the selection table: nothing here that a render rebuilds, so no lock
    const DLightTables lt = r->light_tables_static();
    hipLaunchKernelGGL((k_light_le_query<LT_ALL>), dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, lt, (int)light, reinterpret_cast<const float4 *>(d_rays),
                       (long long)n, d_le);
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}

}  // extern "C"
