// api_lights.hip.h -- gnxr_scene_set_lights: the light list of a live scene replaced (lights_kernel.hip.h), and the test hook
// gnxr_scene_light_tables.  Part of api.hip's translation unit (after api_rebuild.hip.h, whose swap_buf it uses).
//
// The host compiles and checks the whole list first (compile_light_list, scene_compile.cpp).  Every device of the handle then takes the
// records into a FRESH buffer (the count changes, and the old records must survive a failure), binds the AREA_TRI records to their
// leaf-order triangles (k_lights_scatter, k_lights_bind: the device holds the only leaf order) and lets k_refit_lights
// compute corners, area and normal.  DTri::light is the one thing written in place: a failure on any copy puts the old values, which the
// still unchanged host scene describes, back on every copy.  Only then does the host scene change, once, and the copies swap buffers.
// What crosses to the host: the finished records (gnxr_scene_update_lights and the power table read them) and one flag.
#pragma once

static_assert(sizeof(DLight) == 112, "gnxr_scene_light_tables documents 28 words per record");

namespace {

struct LightsBuilt {
    DevBuf<DLight> lights;
    DevBuf<int32_t> infinite;
    std::vector<DLight> h_lights;
};

// DTri::light of every leaf-order triangle of the (bound) device from an authoring-order table in host memory; nothing else is written
int lights_bind_back(gnxr_scene *s, const std::vector<int32_t> &light_of_prim) {
    const int nt = (int)light_of_prim.size();
    DevBuf<int32_t> lop;
    if (int rc = lop.upload(light_of_prim)) return rc;
    hipLaunchKernelGGL(lightedit::k_lights_bind, dim3(grid_for(nt)), dim3(refit::kB), 0, 0, s->tris.p, nt, (const int *)lop.p, (DLight *)nullptr, 0, (const float *)nullptr,
                       (const float *)nullptr, (int *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return GNXR_OK;
}

// One copy's share on its (bound) device: `recs` (compile_light_list's, max(1, n) of them) and `infinite` into fresh buffers, DTri::light
// in place, the finished records into out->h_lights.  Everything is queued on st and waited for.
int lights_on_device(gnxr_scene *s, const std::vector<DLight> &recs, int n_lights, const std::vector<int32_t> &infinite, hipStream_t st, LightsBuilt *out) {
    const SceneFacts &cs = s->cs;
    const int nt = (int)cs.tri_material.size();
    DevBuf<int32_t> lop;
    DevBuf<int> flag;
    int rc;
    if ((rc = out->lights.alloc(recs.size())) || (rc = out->infinite.alloc(infinite.size())) || (rc = lop.alloc(nt)) || (rc = flag.alloc(1))) return rc;
    if (s->tris.n < (size_t)nt) { set_error("set_lights: the device holds %zu triangles, the host scene %d (internal error)", s->tris.n, nt); return GNXR_ERR_RUNTIME; }
    HIP_TRY(hipMemcpyAsync(out->lights.p, recs.data(), recs.size() * sizeof(DLight), hipMemcpyHostToDevice, st));
    if (!infinite.empty()) HIP_TRY(hipMemcpyAsync(out->infinite.p, infinite.data(), infinite.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(lop.p, 0xff, (size_t)nt * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    if (n_lights > 0) hipLaunchKernelGGL(lightedit::k_lights_scatter, dim3(grid_for(n_lights)), dim3(refit::kB), 0, st, (const DLight *)out->lights.p, n_lights, lop.p, nt);
    hipLaunchKernelGGL(lightedit::k_lights_bind, dim3(grid_for(nt)), dim3(refit::kB), 0, st, s->tris.p, nt, (const int *)lop.p, out->lights.p, n_lights,
                       cs.has_tri_n ? (const float *)s->tri_n.p : (const float *)nullptr, cs.has_tri_s ? (const float *)s->tri_s.p : (const float *)nullptr, flag.p);
    if (n_lights > 0) hipLaunchKernelGGL(refit::k_refit_lights, dim3(grid_for(n_lights)), dim3(refit::kB), 0, st, out->lights.p, n_lights, (const DTri *)s->tris.p, nt);
    HIP_TRY(hipGetLastError());
    int h_flag = 0;
    out->h_lights.resize(recs.size());
    HIP_TRY(hipMemcpyAsync(out->h_lights.data(), out->lights.p, recs.size() * sizeof(DLight), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_flag, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flag) { set_error("set_lights: per-vertex normals or tangents on an emissive triangle are not supported"); return GNXR_ERR_INVALID; }
    return GNXR_OK;
}

}  // namespace

extern "C" int gnxr_scene_set_lights(gnxr_scene *s, const gnxr_light *lights, int32_t n_lights, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_lights < 0) { set_error("set_lights: %d lights", n_lights); return GNXR_ERR_INVALID; }
    if (n_lights > 0 && !lights) { set_error("null light array"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    SceneFacts &cs = s->cs;
    // 1. the whole list, compiled and checked on the host: a refusal has touched nothing
    std::vector<DLight> recs;
    std::vector<int32_t> infinite, light_of_prim;
    int rc = compile_light_list(cs, lights, n_lights, &recs, &infinite, &light_of_prim);
    if (rc) return rc;
    if ((rc = s->bind()) != GNXR_OK) return rc;
    // 2. every device (the primary on the caller's stream); all must finish with the same records
    std::vector<LightsBuilt> built(s->n_copies());
    rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int { return lights_on_device(c, recs, n_lights, infinite, i == 0 ? (hipStream_t)hip_stream : nullptr, &built[i]); });
    for (size_t i = 1; i < built.size() && rc == GNXR_OK; ++i)
        if (memcmp(built[i].h_lights.data(), built[0].h_lights.data(), recs.size() * sizeof(DLight)) != 0) { set_error("set_lights: the devices disagree (internal error)"); rc = GNXR_ERR_RUNTIME; }
    if (rc) {
        // DTri::light was written in place: the old values, from the list the host scene still holds, back on every copy
        std::vector<int32_t> old(light_of_prim.size(), -1);
        for (size_t l = 0; l < cs.desc_lights.size(); ++l)
            if (cs.desc_lights[l].type == GNXR_LIGHT_AREA_TRI && (size_t)cs.desc_lights[l].tri < old.size()) old[cs.desc_lights[l].tri] = (int32_t)l;
        return s->put_back_after(rc, [&](gnxr_scene *c, size_t) -> int { (void)lights_bind_back(c, old); (void)hipGetLastError(); return GNXR_OK; });
    }
    // 3. the host scene, once ...
    cs.lights = std::move(built[0].h_lights);
    cs.desc_lights.assign(lights, lights + n_lights);
    cs.infinite_lights = std::move(infinite);
    // ... then every copy: pointer swaps, and a new light-selection table at the next render
    for (size_t i = 0; i < s->n_copies(); ++i) {
        gnxr_scene *c = s->copy(i);
        swap_buf(c->lights, built[i].lights);
        swap_buf(c->infinite, built[i].infinite);
        c->grid_strategy = -1;
    }
    // the old records are released with `built` (hipFree waits for what still reads them)
    return GNXR_OK;
}

// test hook: the DLight records of the first device (which 0; n_lights records, none for a scene without lights), or DTri::light of every
// triangle in authoring order (which 1)
extern "C" int gnxr_scene_light_tables(gnxr_scene *s, int32_t which, void *out, int64_t capacity_bytes, int64_t *n_bytes) {
    if (!s || !n_bytes) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (which < 0 || which > 1) { set_error("light table %d outside [0, 2)", which); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    const int nt = (int)cs.tri_material.size();
    const size_t bytes = which == 0 ? cs.desc_lights.size() * sizeof(DLight) : (size_t)nt * sizeof(int32_t);
    *n_bytes = (int64_t)bytes;
    if (!out || capacity_bytes < (int64_t)bytes || bytes == 0) return GNXR_OK;
    if (int rc = s->bind()) return rc;
    if (which == 0) {
        HIP_TRY(hipMemcpy(out, s->lights.p, bytes, hipMemcpyDeviceToHost));
        return GNXR_OK;
    }
    DevBuf<int32_t> d_light;
    if (int rc = d_light.alloc(nt)) return rc;
    HIP_TRY(hipMemset(d_light.p, 0xff, bytes));
    hipLaunchKernelGGL(lightedit::k_lights_gather, dim3(grid_for(nt)), dim3(refit::kB), 0, 0, (const DTri *)s->tris.p, nt, d_light.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_light.p, bytes, hipMemcpyDeviceToHost));
    return GNXR_OK;
}
