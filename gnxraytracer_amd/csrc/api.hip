// api.hip -- C ABI of libgnxr.so (include/gnxr.h): one translation unit.  This file keeps initialisation, scene creation, the render entry
// points and the host-memory probes (gnxr_scene_create compiles into a local CompiledScene, uploads it and leaves the handle its facts:
// host_scene.h); the rest lives in the api_*.hip.h headers included below (shared pieces, gnxr_scene, the HLBVH build
// driver, the peak probes, the front end of the calls on device memory, the render path, the editing calls, the in-place BVH rebuild, the
// light list's replacement, the environment light's rebuild, the media edit, the texture edit, the entry points on device memory, adaptive sampling, the denoiser, the film, lightmap baking, mesh deformation, closest-point queries, all-hits ray queries, neighbour queries, sphere casts).  One process drives one GPU (gnxr_init), or several behind every handle (gnxr_init_devices).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_scene.h"
#include "kernels.hip.h"
#include "trace4_kernel.hip.h"
#include "hlbvh_build.hip.h"
#include "refit_kernel.hip.h"
#include "material_kernel.hip.h"
#include "rebuild_kernel.hip.h"
#include "geometry_kernel.hip.h"
#include "lights_kernel.hip.h"
#include "env_build_kernel.hip.h"
#include "media_kernel.hip.h"
#include "texture_build_kernel.hip.h"
#include "li_kernel.hip.h"
#include "views_kernel.hip.h"
#include "shade_query_kernel.hip.h"
#include "aov_kernel.hip.h"
#include "adaptive_kernel.hip.h"
#include "denoise_kernel.hip.h"
#include "film_kernel.hip.h"
#include "bake_kernel.hip.h"
#include "lightprobe_kernel.hip.h"
#include "temporal_kernel.hip.h"
#include "display_kernel.hip.h"
#include "deform_kernel.hip.h"
#include "closest_kernel.hip.h"
#include "allhits_kernel.hip.h"
#include "near_kernel.hip.h"
#include "spherecast_kernel.hip.h"
#include "overlap_kernel.hip.h"
#include "overlap_tri_kernel.hip.h"
#include "kernel_instances.h"

using namespace gnxr;

// compiled in inst_whitted.hip / inst_whitted_tex.hip / inst_vol.hip
#define X(M, L, S, T) extern template GX_WHITTED_SIGNATURE(M, L, S, T)
GX_WHITTED_INSTANCES(X)
#undef X
#define X(M, L, ST, T) extern template GX_VOL_SIGNATURE(M, L, ST, T)
GX_VOL_INSTANCES(X)
#undef X
// compiled in inst_shade_kinds.hip
#define X(M, L) extern template GX_SHADE_KIND_SIGNATURE(M, L)
GX_SHADE_KIND_INSTANCES(X)
#undef X
#define X(M, L, S) extern template GX_SHADE_MIS_SIGNATURE(M, L, S)
GX_SHADE_MIS_INSTANCES(X)
#undef X
// compiled in inst_shade_query.hip
extern template GX_BSDF_QUERY_SIGNATURE(LM_ALL)
extern template GX_LIGHT_SAMPLE_QUERY_SIGNATURE(LT_ALL)
extern template GX_LIGHT_LE_QUERY_SIGNATURE(LT_ALL)
extern template GX_TRACE_CLOSEST_CODE_SIGNATURE(32)
extern template GX_TRACE_CLOSEST_CODE_SIGNATURE(64)
// compiled in inst_aov.hip
#define X(M) extern template GX_AOV_RESOLVE_SIGNATURE(M)
GX_AOV_INSTANCES(X)
#undef X

#include "api_common.hip.h"
#include "api_scene.hip.h"
#include "api_hlbvh.hip.h"
#include "api_probes.hip.h"
#include "api_device_call.hip.h"
#include "api_render.hip.h"

extern "C" {

int gnxr_init(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_error("no HIP device available; libgnxr has no CPU fallback"); return GNXR_ERR_NO_DEVICE; }
    if (device_id < 0 || device_id >= n) { set_error("device %d out of range (%d visible)", device_id, n); return GNXR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(device_id));
    g_device = -1;
    g_devices.assign(1, device_id);
    g_peer_ok.assign(1, 1);
    return ensure_device();
}
int gnxr_init_devices(int32_t n_devices, const int32_t *device_ids) {
    if (n_devices <= 0 || n_devices > 64 || !device_ids) { set_error("bad device list"); return GNXR_ERR_INVALID; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_error("no HIP device available; libgnxr has no CPU fallback"); return GNXR_ERR_NO_DEVICE; }
    for (int i = 0; i < n_devices; ++i)
        if (device_ids[i] < 0 || device_ids[i] >= n) { set_error("device %d out of range (%d visible)", device_ids[i], n); return GNXR_ERR_INVALID; }
    int rc = gnxr_init(device_ids[0]);
    if (rc) return rc;
    g_devices.assign(device_ids, device_ids + n_devices);
    // Peer access between the primary and the others (assembling the image).  Whether it was granted is RECORDED per device: a pair
    // without it assembles its rows through a pinned host buffer (render_sharded), it is never assumed.
    g_peer_ok.assign(n_devices, 1);
    for (int i = 1; i < n_devices; ++i) {
        if (device_ids[i] == device_ids[0]) continue;   // the same card listed twice: plain device-to-device copies
        int can01 = 0, can10 = 0;
        bool ok = hipDeviceCanAccessPeer(&can01, device_ids[0], device_ids[i]) == hipSuccess && can01 &&
                  hipDeviceCanAccessPeer(&can10, device_ids[i], device_ids[0]) == hipSuccess && can10;
        if (ok) {
            hipError_t e0 = hipSetDevice(device_ids[0]) == hipSuccess ? hipDeviceEnablePeerAccess(device_ids[i], 0) : hipErrorInvalidDevice;
            hipError_t e1 = hipSetDevice(device_ids[i]) == hipSuccess ? hipDeviceEnablePeerAccess(device_ids[0], 0) : hipErrorInvalidDevice;
            ok = (e0 == hipSuccess || e0 == hipErrorPeerAccessAlreadyEnabled) && (e1 == hipSuccess || e1 == hipErrorPeerAccessAlreadyEnabled);
        }
        g_peer_ok[i] = ok ? 1 : 0;
        if (getenv("GNXR_VERBOSE")) fprintf(stderr, "[gnxr] device %d <-> %d: %s\n", device_ids[0], device_ids[i], ok ? "peer access" : "no peer access: rows are staged through the host");
    }
    (void)hipGetLastError();
    if (getenv("GNXR_NO_PEER")) for (int i = 1; i < n_devices; ++i) g_peer_ok[i] = 0;   // test switch: take the host-staged route everywhere
    HIP_TRY(hipSetDevice(device_ids[0]));
    return GNXR_OK;
}
void gnxr_shutdown(void) { g_device = -1; g_devices.clear(); g_peer_ok.clear(); }
int gnxr_set_profiling(int flags) { g_profiling = flags; return GNXR_OK; }
#ifdef GX_SHADE_STATS
// development builds only (-DGX_SHADE_STATS): wave-time per section of k_shade
int gnxr_debug_shade_stats(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_shade_stats), 16 * sizeof(unsigned long long)) != hipSuccess) return GNXR_ERR_INVALID;
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_shade_stats), z, sizeof(z)); }
    return GNXR_OK;
}
#endif
#ifdef GX_TRACE_STATS
// development builds only (-DGX_TRACE_STATS): wave-level occupancy statistics of k_trace
int gnxr_debug_trace_stats(unsigned long long *out16, int reset) {   // 24 slots
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_trace_stats), 24 * sizeof(unsigned long long)) != hipSuccess) return GNXR_ERR_INVALID;
    if (reset) { unsigned long long z[24] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace_stats), z, sizeof(z)); }
    return GNXR_OK;
}
#endif
#ifdef GX_TAIL_STAMP
// development builds only (-DGX_TAIL_STAMP): what of the k_trace4 launches lay behind the end of their work lists (g_tail, trace_kernel.hip.h)
int gnxr_debug_tail_stamp(unsigned long long *out12, int reset) {
    if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_tail), 12 * sizeof(unsigned long long)) != hipSuccess) return GNXR_ERR_INVALID;
    if (reset) { unsigned long long z[12] = {~0ull, 0ull, ~0ull, 0ull}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tail), z, sizeof(z)); }
    return GNXR_OK;
}
#endif

// device side of gnxr_scene_create: everything compile_scene produced goes to the copy's (bound) device -- the upload tables from the
// caller's (they end with gnxr_scene_create), the tables among the facts from the handle's host scene
static int upload_scene(gnxr_scene *s, const SceneUploadTables &up) {
    const SceneFacts &cs = s->cs;
    int rc;
    if (cs.bvh_max_depth + 1 > 64) { set_error("BVH depth %d exceeds the 64-entry traversal stack (BVHAccel.cpp:661)", cs.bvh_max_depth); return GNXR_ERR_UNSUPPORTED; }
    s->set_traversal(std::any_of(up.nodes.begin(), up.nodes.end(), [](const DNode &n) { return (n.meta & 0xffffu) > 127; }));
#define UP(from, field) if ((rc = s->field.upload(from.field)) != GNXR_OK) return rc;
    UP(up, nodes) UP(up, nodes4) UP(up, tris) UP(up, leaf_boxes) UP(up, tri_class) UP(cs, lights) UP(cs, perms) UP(cs, primes) UP(cs, prime_sums) UP(cs, prime_magic)
    UP(cs, dmedia) UP(up, grid_density) UP(up, tri_media) UP(cs, spheres) UP(cs, textures) UP(up, tex_texels) UP(up, ewa_lut) UP(up, tri_uv) UP(up, tri_n) UP(up, tri_s)
    UP(cs, aov_albedo)
    UP(cs, env_texels4) UP(cs, env_cond_func) UP(cs, env_cond_cdf) UP(cs, env_cond_int) UP(cs, env_marg_func) UP(cs, env_marg_cdf) UP(cs, env_marg_guide) UP(cs, env_cond_guide)
#undef UP
    {   // materials, preceded by one record that carries the texture tables.  A material edit may give every authored material an attribute
        // copy: the buffers are sized for that once, so that no edit reallocates them under queries in flight
        const size_t worst = 2 * cs.desc_materials.size();
        if ((rc = s->material_authored.alloc(worst)) || (rc = s->materials.alloc(1 + worst)) || (rc = s->materials_single.alloc(1 + worst))) return rc;
        if ((rc = s->material_authored.upload(cs.material_authored)) != GNXR_OK) return rc;
        const DTexTables at = s->tex_tables(s->tri_uv.p, s->tri_n.p, s->tri_s.p);   // (an empty upload still allocates: absent tables are null here)
        if ((rc = s->write_material_tables(cs.materials, cs.materials_single, at.tri_uv, at.tri_n, at.tri_s)) != GNXR_OK) return rc;
    }
    if ((rc = s->infinite.upload(cs.infinite_lights)) != GNXR_OK) return rc;
    if ((rc = s->counters.alloc(1)) != GNXR_OK) return rc;
    if (hipHostMalloc((void **)&s->h_counters, sizeof(Counters)) != hipSuccess) { set_error("hipHostMalloc failed"); return GNXR_ERR_OOM; }
    if (hipHostMalloc((void **)&s->h_ring, sizeof(Counters) * gnxr_scene::kRing) != hipSuccess) { set_error("hipHostMalloc failed"); return GNXR_ERR_OOM; }
    for (hipEvent_t &e : s->ring_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipStream_t &a : s->aux_stream) HIP_TRY(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
    for (hipEvent_t &e : s->ev_join) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return GNXR_OK;
}

int gnxr_scene_create(const gnxr_scene_desc *desc, gnxr_scene **out) {
    if (!desc || !out) { set_error("null argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    gnxr_scene *s = new (std::nothrow) gnxr_scene(g_device);
    if (!s) return GNXR_ERR_OOM;
    // the whole compiled scene lives in this call: its facts move into the handle (with the refit's seeds, which go to a device at the
    // first edit), its upload tables go to the devices and end here
    CompiledScene compiled;
    if (!compile_scene(desc, &compiled, device_hlbvh_build)) { delete s; return GNXR_ERR_INVALID; }
    s->cs = std::move(static_cast<SceneFacts &>(compiled));
    s->cs.refit_seeds = std::move(static_cast<RefitSeeds &>(compiled));
    // gnxr_init_devices: a copy on every other device of the list, sharing the host scene; then the same tables on every device
    for (size_t i = 1; i < g_devices.size(); ++i) s->replicas.push_back(std::make_unique<gnxr_scene>(g_devices[i], s->host));
    s->host->copies_awaiting_seeds = s->n_copies();
    if ((rc = s->each_copy([&](gnxr_scene *c, size_t) { return upload_scene(c, compiled); })) != GNXR_OK) { delete s; return rc; }
    const SceneFacts &cs = s->cs;
    if (getenv("GNXR_VERBOSE"))
        fprintf(stderr, "[gnxr] scene: %zu tris, %zu nodes (depth %d), %zu 4-wide nodes (stack %d), wide=%d, %zu device(s)\n", cs.n_triangles, cs.n_nodes, cs.bvh_max_depth,
                cs.n_nodes4, cs.stack4_need, (int)s->wide_ok, s->n_copies());
    *out = s;
    return GNXR_OK;
}
void gnxr_scene_destroy(gnxr_scene *s) { delete s; }

int gnxr_scene_info(const gnxr_scene *s, int32_t *n_nodes, int32_t *max_depth, int32_t *n_vox) {
    if (!s) return GNXR_ERR_INVALID;
    if (n_nodes) *n_nodes = (int32_t)s->cs.n_nodes;
    if (max_depth) *max_depth = s->cs.bvh_max_depth;
    if (n_vox) *n_vox = s->grid_strategy >= 0 ? s->grid.nvox[0] * s->grid.nvox[1] * s->grid.nvox[2] : 0;
    return GNXR_OK;
}

// Who added the light estimates of the handle's last PathIntegrator render (Counters::nee_applied_*), summed over its devices.  A call of
// its own: gnxr_stats keeps its layout.
int gnxr_scene_nee_apply_counts(gnxr_scene *s, uint64_t *in_trace, uint64_t *by_sweep) {
    if (!s) { set_error("null argument"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    uint64_t t = 0, w = 0;
    for (size_t i = 0; i <= s->replicas.size(); ++i) {
        const Counters *c = s->copy(i)->h_counters;
        if (c) { t += c->nee_applied_trace; w += c->nee_applied_sweep; }
    }
    if (in_trace) *in_trace = t;
    if (by_sweep) *by_sweep = w;
    return GNXR_OK;
}

// What k_trace4<COUNT> counted in the handle's last render (Counters::tris_hot / tris), summed over its devices.
int gnxr_scene_hot_leaf_counts(gnxr_scene *s, uint64_t *tris_from_lds, uint64_t *tris_loaded) {
    if (!s) { set_error("null argument"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    uint64_t h = 0, t = 0;
    for (size_t i = 0; i <= s->replicas.size(); ++i) {
        const Counters *c = s->copy(i)->h_counters;
        if (c) { h += c->tris_hot; t += c->tris; }
    }
    if (tris_from_lds) *tris_from_lds = h;
    if (tris_loaded) *tris_loaded = t;
    return GNXR_OK;
}

// The launch shape trace_launch gives a render's timed traversal launches on this scene (a launch of `total` work items): what a test pins.
int gnxr_scene_trace_plan(const gnxr_scene *s, int64_t total, gnxr_trace_plan *out) {
    if (!s || !out || total < 0) { set_error("null argument"); return GNXR_ERR_INVALID; }
    const TraceLaunch t = trace_launch(s, s->wide_ok, s->cs.n_spheres > 0, total);
    out->wide = s->wide_ok ? 1 : 0;
    out->stack_entries = t.entries; out->lds_entries = t.lds_entries;
    out->lds_bytes = (int64_t)t.lds;
    out->n_top = t.n_top; out->hot_bytes = t.hot_bytes;
    out->blocks = t.blocks; out->blocks_per_cu = g_trace_blocks_per_cu;
    return GNXR_OK;
}

int gnxr_render_device(gnxr_scene *s, const gnxr_render_params *pin, void *d_rgba_out, void *hip_stream, gnxr_stats *stats) {
    return render_sharded(s, pin, d_rgba_out, hip_stream, stats);
}

// Allocates the path state a render with these parameters needs (on every device of the handle) without rendering: a caller that times
// its renders -- or a viewer that must not stall in its first frame -- pays for the allocation up front.  State only ever grows.
int gnxr_render_reserve(gnxr_scene *s, const gnxr_render_params *pin) {
    if (!s || !pin) { set_error("null argument"); return GNXR_ERR_INVALID; }
    int dummy = 0;   // never written: render_one returns before anything touches the output
    return render_sharded(s, pin, &dummy, nullptr, nullptr, /*reserve_only=*/true);
}

int gnxr_render(gnxr_scene *s, const gnxr_render_params *p, float *rgba_out, gnxr_stats *stats) {
    if (!s || !p || !rgba_out) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (p->width <= 0 || p->height <= 0) { set_error("invalid image size"); return GNXR_ERR_INVALID; }
    size_t npx = (size_t)p->width * p->height;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);   // s->out is shared by every gnxr_render on this handle
    if (int brc = s->bind()) return brc;
    const bool grew = !(s->out.p && npx <= s->out.n);
    int rc = s->out.alloc(npx);
    if (rc) return rc;
    HIP_TRY(hipMemset(s->out.p, 0, npx * sizeof(float4)));
    rc = render_sharded(s, p, s->out.p, nullptr, stats);
    // a refused call (render_one: plan_render / size_passes run before RenderState::reserve) leaves device memory as it found it:
    // the image this call grew for it goes too
    if (rc) { if (grew) s->out.release(); return rc; }
    // copy back only the rows this shard owns
    int sc = p->shard_count > 0 ? p->shard_count : 1, sr = p->shard_rows > 0 ? p->shard_rows : 1;
    if (sc == 1) {
        HIP_TRY(hipMemcpy(rgba_out, s->out.p, npx * sizeof(float4), hipMemcpyDeviceToHost));
    } else {
        for (int y = 0; y < p->height; ++y)
            if ((y / sr) % sc == p->shard_index)
                HIP_TRY(hipMemcpy(rgba_out + (size_t)y * p->width * 4, s->out.p + (size_t)y * p->width, (size_t)p->width * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return GNXR_OK;
}

int gnxr_scene_bvh(const gnxr_scene *sc, float *bounds6, int32_t *meta3, int32_t *ordered, int64_t node_capacity, int64_t *n_nodes) {
    if (!sc || !n_nodes) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    // const for the caller (the scene does not change); the tables are read from the first device, as gnxr_scene_bvh4 reads them
    gnxr_scene *s = const_cast<gnxr_scene *>(sc);
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    *n_nodes = (int64_t)s->cs.n_nodes;
    if (!bounds6 || !meta3 || !ordered || node_capacity < *n_nodes) return GNXR_OK;
    if (int rc = s->bind()) return rc;
    std::vector<DNode> nodes(s->cs.n_nodes);
    std::vector<DTri> tris(s->cs.n_triangles);
    HIP_TRY(hipMemcpy(nodes.data(), s->nodes.p, nodes.size() * sizeof(DNode), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tris.data(), s->tris.p, tris.size() * sizeof(DTri), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nodes.size(); ++i) {
        const DNode &n = nodes[i];
        bounds6[6 * i + 0] = n.lo[0]; bounds6[6 * i + 1] = n.lo[1]; bounds6[6 * i + 2] = n.lo[2];
        bounds6[6 * i + 3] = n.hi0; bounds6[6 * i + 4] = n.hi1; bounds6[6 * i + 5] = n.hi2;
        const int nPrims = (int)(n.meta & 0xffffu);
        meta3[3 * i + 0] = n.offset; meta3[3 * i + 1] = nPrims; meta3[3 * i + 2] = nPrims ? 0 : (int)(n.meta >> 16);
    }
    for (size_t i = 0; i < tris.size(); ++i) ordered[i] = tris[i].prim;
    return GNXR_OK;
}

int gnxr_trace_closest(gnxr_scene *s, const gnxr_ray *rays, int64_t n, gnxr_hit *hits) {
    if (!s || !rays || !hits || n < 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<gnxr_ray> dr;
    DevBuf<gnxr_hit> dh;
    int rc;
    if ((rc = dr.upload(rays, (size_t)n)) || (rc = dh.alloc((size_t)n))) return rc;
    DScene sc = s->device_scene(1, 1);
    if ((rc = binary_trace_api(s, sc, dr.p, n, dh.p, /*any=*/false, nullptr)) != GNXR_OK) return rc;
    HIP_TRY(hipMemcpy(hits, dh.p, (size_t)n * sizeof(gnxr_hit), hipMemcpyDeviceToHost));
    return GNXR_OK;
}
int gnxr_trace_any(gnxr_scene *s, const gnxr_ray *rays, int64_t n, uint8_t *occluded) {
    if (!s || !rays || !occluded || n < 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if (int brc = s->bind()) return brc;
    DevBuf<gnxr_ray> dr;
    DevBuf<unsigned char> dob;
    int rc;
    if ((rc = dr.upload(rays, (size_t)n)) || (rc = dob.alloc((size_t)n))) return rc;
    DScene sc = s->device_scene(1, 1);
    if ((rc = binary_trace_api(s, sc, dr.p, n, dob.p, /*any=*/true, nullptr)) != GNXR_OK) return rc;
    HIP_TRY(hipMemcpy(occluded, dob.p, (size_t)n, hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"

#include "api_edit.hip.h"
#include "api_rebuild.hip.h"
#include "api_geometry.hip.h"
#include "api_lights.hip.h"
#include "api_env.hip.h"
#include "api_media.hip.h"
#include "api_textures.hip.h"
#include "api_query.hip.h"
#include "api_walk.hip.h"
#include "api_closest.hip.h"
#include "api_allhits.hip.h"
#include "api_near.hip.h"
#include "api_spherecast.hip.h"
#include "api_overlap.hip.h"
#include "api_overlap_tri.hip.h"
#include "api_aov.hip.h"
#include "api_adaptive.hip.h"
#include "api_denoise.hip.h"
#include "api_film.hip.h"
#include "api_bake.hip.h"
#include "api_lightprobe.hip.h"
#include "api_temporal.hip.h"
#include "api_display.hip.h"
#include "api_deform.hip.h"

extern "C" {

// sampler tables without a scene (probes)
static int probe_tables(CompiledScene *cs, DevBuf<uint16_t> *perms, DevBuf<int32_t> *primes, DevBuf<int32_t> *sums, DevBuf<uint32_t> *magic, DSamplerTables *st,
                        int W, int H) {
    // a one-triangle scene is the cheapest way to reuse the table builder
    float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    int32_t idx[3] = {0, 1, 2}, mat[1] = {-1}, lt[1] = {-1};
    gnxr_scene_desc d;
    memset(&d, 0, sizeof(d));
    d.abi_version = GNXR_ABI_VERSION; d.n_vertices = 3; d.n_triangles = 1; d.vertices = v; d.indices = idx; d.tri_material = mat; d.tri_light = lt;
    if (!compile_scene(&d, cs)) return GNXR_ERR_INVALID;
    int rc;
    if ((rc = perms->upload(cs->perms)) || (rc = primes->upload(cs->primes)) || (rc = sums->upload(cs->prime_sums)) || (rc = magic->upload(cs->prime_magic))) return rc;
    st->perms = perms->p; st->primes = primes->p; st->prime_sums = sums->p; st->prime_magic = magic->p;
    st->h = make_halton(W, H);
    return GNXR_OK;
}

int gnxr_sample_halton(int32_t width, int32_t height, const int32_t *px, const int32_t *py, const int64_t *sidx, const int32_t *dim, int64_t n, float *out) {
    if (!px || !py || !sidx || !dim || !out || n < 0 || width <= 0 || height <= 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return GNXR_OK;
    CompiledScene cs;
    DevBuf<uint16_t> perms; DevBuf<int32_t> primes, sums; DevBuf<uint32_t> magic;
    DSamplerTables st;
    if ((rc = probe_tables(&cs, &perms, &primes, &sums, &magic, &st, width, height))) return rc;
    DevBuf<int32_t> dpx, dpy, ddim; DevBuf<long long> ds; DevBuf<float> dout;
    if ((rc = dpx.upload(px, n)) || (rc = dpy.upload(py, n)) || (rc = ddim.upload(dim, n)) || (rc = ds.upload((const long long *)sidx, n)) || (rc = dout.alloc(n))) return rc;
    {   // the probe takes the render path's 32-bit accumulator wherever its indices allow it
        unsigned long long smax = 0;
        for (int64_t i = 0; i < n; ++i) smax = std::max<unsigned long long>(smax, (unsigned long long)std::max<int64_t>(0, sidx[i]));
        const unsigned long long bound = (unsigned long long)st.h.stride * (smax + 2);
        st.h.base32_max = bound >= (1ull << 32) ? 0 : (int32_t)std::min<unsigned long long>(0x7fffffffull, 0xffffffffull / bound);
    }
    hipLaunchKernelGGL(k_halton_probe, dim3(grid_for(n)), dim3(kBlock), 0, 0, st, (const int *)dpx.p, (const int *)dpy.p, (const long long *)ds.p, (const int *)ddim.p, (long long)n, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

int gnxr_camera_rays(const gnxr_camera *cam, int32_t width, int32_t height, const int32_t *px, const int32_t *py, const int64_t *sidx, int64_t n, float *o_out,
                     float *d_out) {
    if (!cam || !px || !py || !sidx || !o_out || !d_out || n < 0 || width <= 0 || height <= 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return GNXR_OK;
    CompiledScene cs;
    DevBuf<uint16_t> perms; DevBuf<int32_t> primes, sums; DevBuf<uint32_t> magic;
    DSamplerTables st;
    if ((rc = probe_tables(&cs, &perms, &primes, &sums, &magic, &st, width, height))) return rc;
    DCamera dc = make_camera(*cam, width, height, -1);
    DevBuf<int32_t> dpx, dpy; DevBuf<long long> ds; DevBuf<float> dob, dd;
    if ((rc = dpx.upload(px, n)) || (rc = dpy.upload(py, n)) || (rc = ds.upload((const long long *)sidx, n)) || (rc = dob.alloc(3 * n)) || (rc = dd.alloc(3 * n))) return rc;
    hipLaunchKernelGGL(k_camera_probe, dim3(grid_for(n)), dim3(kBlock), 0, 0, st, dc, (const int *)dpx.p, (const int *)dpy.p, (const long long *)ds.p, (long long)n, dob.p, dd.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(o_out, dob.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(d_out, dd.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

// The sampler tables of probe_tables on `device`, uploaded once per device and kept until the process ends (never freed: the runtime may
// be gone when static destructors run).  h of the returned tables is the caller's to set (make_halton).
static int device_probe_tables(int device, DSamplerTables *st) {
    struct Set { CompiledScene cs; DevBuf<uint16_t> perms; DevBuf<int32_t> primes, sums; DevBuf<uint32_t> magic; DSamplerTables st; };
    static std::mutex m;
    static std::vector<std::pair<int, Set *>> sets;
    std::lock_guard<std::mutex> lock(m);
    for (auto &e : sets) if (e.first == device) { *st = e.second->st; return GNXR_OK; }
    std::unique_ptr<Set> set(new (std::nothrow) Set());
    if (!set) return GNXR_ERR_OOM;
    if (int rc = probe_tables(&set->cs, &set->perms, &set->primes, &set->sums, &set->magic, &set->st, 1, 1)) return rc;
    *st = set->st;
    sets.emplace_back(device, set.release());
    return GNXR_OK;
}

// The device-memory form of gnxr_camera_rays: rays and sample records for gnxr_li_device, written on the caller's stream.  No scene: the
// sampler tables are cached per device, the camera travels as a kernel argument, and the only allocation is the 8-byte status word.
int gnxr_camera_rays_device(const gnxr_camera *cam, int32_t camera_medium, int32_t width, int32_t height, const int32_t *d_px, const int32_t *d_py, const int32_t *d_s,
                            int64_t n, gnxr_ray *d_rays, gnxr_li_sample *d_samples, void *hip_stream) {
    if (!cam || n < 0 || width <= 0 || height <= 0 || camera_medium < -1 || (n > 0 && (!d_px || !d_py || !d_s || !d_rays || !d_samples))) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (n == 0) return GNXR_OK;
    if ((((uintptr_t)d_rays | (uintptr_t)d_samples) & 15u) != 0) { set_error("d_rays and d_samples must be 16-byte aligned"); return GNXR_ERR_INVALID; }
    if ((((uintptr_t)d_px | (uintptr_t)d_py | (uintptr_t)d_s) & 3u) != 0) { set_error("d_px, d_py and d_s must be 4-byte aligned"); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    const QueryArg args[] = {{d_px, (size_t)n * 4, "d_px"}, {d_py, (size_t)n * 4, "d_py"}, {d_s, (size_t)n * 4, "d_s"}, {d_rays, (size_t)n * sizeof(gnxr_ray), "d_rays"},
                             {d_samples, (size_t)n * sizeof(gnxr_li_sample), "d_samples"}};
    DeviceCall call;
    if (int rc = call.bind("", args, " (host arrays go through gnxr_camera_rays)")) return rc;
    DSamplerTables st;
    if (int rc = device_probe_tables(call.device, &st)) return rc;
    st.h = make_halton(width, height);
    const DCamera dc = make_camera(*cam, width, height, camera_medium);
    hipStream_t stream = (hipStream_t)hip_stream;
    StatusWord status;
    unsigned long long bad = 0;
    if (int rc = status.alloc(stream)) return rc;
    hipLaunchKernelGGL(k_camera_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, st, dc, (int)width, (int)height, (const int *)d_px, (const int *)d_py, (const int *)d_s,
                       (long long)n, reinterpret_cast<float4 *>(d_rays), reinterpret_cast<int4 *>(d_samples), status.d);
    HIP_TRY(hipGetLastError());
    if (int rc = status.fetch(&bad)) return rc;
    if (bad) {
        set_error("gnxr_camera_rays_device: record %llu is out of range (px in [0, %d), py in [0, %d), s >= 0); its ray and sample are 0", (unsigned long long)~bad, width, height);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

int gnxr_light_grid_table(gnxr_scene *s, int32_t strategy, int32_t on_host, float *out, int64_t capacity, int64_t *n_floats) {
    if (!s || !n_floats) { set_error("null argument"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    if (int brc = s->bind()) return brc;
    int rc = s->ensure_grid(strategy, on_host != 0);
    if (rc) return rc;
    const int64_t n = (int64_t)s->grid.nvox[0] * s->grid.nvox[1] * s->grid.nvox[2] * s->grid.stride;
    *n_floats = n;
    if (out && capacity >= n) HIP_TRY(hipMemcpy(out, s->grid_table.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

int gnxr_eval_libm(int32_t fn, const float *x, const float *x2, int64_t n, float *out) {
    if (!x || !out || n < 0 || fn < 0 || fn > 8 || (fn >= 7 && !x2)) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return GNXR_OK;
    DevBuf<float> dx, dx2, dout;
    if ((rc = dx.upload(x, (size_t)n)) || (rc = dout.alloc((size_t)n))) return rc;
    if (x2 && (rc = dx2.upload(x2, (size_t)n))) return rc;
    hipLaunchKernelGGL(k_libm_probe, dim3(grid_for(n)), dim3(kBlock), 0, 0, (int)fn, (const float *)dx.p, (const float *)(x2 ? dx2.p : nullptr), (long long)n, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

int gnxr_eval_libm_f64(int32_t fn, const float *x, int64_t n, double *out) {
    if (!x || !out || n < 0 || fn < 0 || fn > 3) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return GNXR_OK;
    DevBuf<float> dx;
    DevBuf<double> dout;
    if ((rc = dx.upload(x, (size_t)n)) || (rc = dout.alloc((size_t)n))) return rc;
    hipLaunchKernelGGL(k_libm_probe_f64, dim3(grid_for(n)), dim3(kBlock), 0, 0, (int)fn, (const float *)dx.p, (long long)n, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

int gnxr_framebuffer_update(float *running_mean_rgba, const float *frame_rgba, int32_t width, int32_t height, int32_t frame_count, uint8_t *rgba8_out) {
    if (!running_mean_rgba || !frame_rgba || !rgba8_out || width <= 0 || height <= 0 || frame_count <= 0) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    size_t nv = (size_t)width * height * 4;
    DevBuf<float> dm, df;
    DevBuf<unsigned char> du;
    if ((rc = dm.upload(running_mean_rgba, nv)) || (rc = df.upload(frame_rgba, nv)) || (rc = du.alloc(nv))) return rc;
    hipLaunchKernelGGL(k_framebuffer_update, dim3(grid_for((long long)nv)), dim3(kBlock), 0, 0, dm.p, (const float *)df.p, (long long)nv, frame_count, du.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(running_mean_rgba, dm.p, nv * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rgba8_out, du.p, nv, hipMemcpyDeviceToHost));
    return GNXR_OK;
}

}  // extern "C"

