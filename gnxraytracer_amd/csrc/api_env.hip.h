// api_env.hip.h -- gnxr_scene_update_environment: host driver of the environment light's rebuild on the device (env_build_kernel.hip.h), and
// the test hook gnxr_scene_env_tables.  Part of api.hip's translation unit (after api_rebuild.hip.h, whose structure it follows and whose
// swap_buf it uses).
//
// Every device of the handle builds the tables into FRESH buffers from the raw map (env_build_on_device); only when all of them have built,
// and agree on the scalars, are the light records written (the one device write that could still fail; a failure puts the host's records,
// still the old ones, back), the host scene told once and the buffers swapped into the copies (pointer swaps only), so a refused or failed
// call leaves the scene as it was.  What crosses to the host: the at most 21 texels of the pyramid's top three levels (InfiniteAreaLight::
// Power's lookup runs over them on the host, in the code gnxr_scene_create runs) and the marginal's funcInt; what crosses to the device
// besides the map: the Lanczos weights (px + py records, computed by the host's resample_weights) and the light records.  The host copies
// of the tables (SceneFacts::env_*) are marked stale and fetched when the host-built spatial light table asks for them (sync_host_env).
#pragma once

namespace {

struct EnvBuilt {
    DevBuf<float> texels4, cond_func, cond_cdf, cond_int, marg_func, marg_cdf;
    DevBuf<uint16_t> marg_guide, cond_guide;
    int rx = 0, ry = 0;
    float marg_func_int = 0.f, power[3] = {0.f, 0.f, 0.f};
    // the scalars the host scene records.  Every device builds the same ones.
    bool same(const EnvBuilt &o) const { return rx == o.rx && ry == o.ry && memcmp(&marg_func_int, &o.marg_func_int, 4) == 0 && memcmp(power, o.power, 12) == 0; }
};

// the environment tables of the w x h map d_rgb (memory of the bound device, complete in stream order on st) into `r`; nothing of `s` changes
int env_build_on_device(gnxr_scene *s, const float *d_rgb, int w, int h, bool flip_y, const float le[3], hipStream_t st, EnvBuilt *r) {
    using namespace envb;
    int rc;
    const bool resample = (w & (w - 1)) || (h & (h - 1));
    const int rx = resample ? env_round_up_pow2(w) : w, ry = resample ? env_round_up_pow2(h) : h;
    const int W2 = 2 * rx, H2 = 2 * ry;
    const size_t n_tex = (size_t)rx * ry;
    if ((rc = r->texels4.alloc(4 * n_tex)) || (rc = r->cond_func.alloc((size_t)W2 * H2)) || (rc = r->cond_cdf.alloc((size_t)(W2 + 1) * H2)) || (rc = r->cond_int.alloc(H2)) ||
        (rc = r->marg_func.alloc(H2)) || (rc = r->marg_cdf.alloc((size_t)H2 + 1)) || (rc = r->marg_guide.alloc(kEnvGuideMarg + 1)) ||
        (rc = r->cond_guide.alloc((size_t)H2 * (kEnvGuideCond + 1))))
        return rc;
    float4 *tex = reinterpret_cast<float4 *>(r->texels4.p);
    // ---- texels, resampled to powers of two when a side is not one
    DevBuf<float4> raw_tex, res_s;
    DevBuf<DResampleWeight> d_sw, d_tw;
    if (!resample) {
        hipLaunchKernelGGL(k_env_texels, dim3(grid_for((long long)w * h)), dim3(kB), 0, st, d_rgb, w, h, flip_y ? 1 : 0, le[0], le[1], le[2], tex);
    } else {
        static_assert(sizeof(DResampleWeight) == sizeof(EnvResampleWeight), "the device reads the host's weight records");
        const std::vector<EnvResampleWeight> sw = env_resample_weights(w, rx), tw = env_resample_weights(h, ry);
        if ((rc = raw_tex.alloc((size_t)w * h)) || (rc = res_s.alloc((size_t)h * rx)) || (rc = d_sw.upload(reinterpret_cast<const DResampleWeight *>(sw.data()), sw.size())) ||
            (rc = d_tw.upload(reinterpret_cast<const DResampleWeight *>(tw.data()), tw.size())))
            return rc;
        hipLaunchKernelGGL(k_env_texels, dim3(grid_for((long long)w * h)), dim3(kB), 0, st, d_rgb, w, h, flip_y ? 1 : 0, le[0], le[1], le[2], raw_tex.p);
        hipLaunchKernelGGL(k_env_resample_s, dim3(grid_for((long long)h * rx)), dim3(kB), 0, st, (const float4 *)raw_tex.p, w, h, rx, (const DResampleWeight *)d_sw.p, res_s.p);
        hipLaunchKernelGGL(k_env_resample_t, dim3(grid_for((long long)n_tex)), dim3(kB), 0, st, (const float4 *)res_s.p, rx, h, ry, (const DResampleWeight *)d_tw.p, tex);
    }
    HIP_TRY(hipGetLastError());
    // ---- the pyramid above level 0 (one buffer, level after level), of which the top three levels come back for the Power lookup
    std::vector<int> lw, lh;
    env_pyramid_sizes(rx, ry, &lw, &lh);
    const int n_levels = (int)lw.size();
    std::vector<size_t> off(n_levels, 0);
    size_t n_pyr = 0;
    for (int i = 1; i < n_levels; ++i) { off[i] = n_pyr; n_pyr += (size_t)lw[i] * lh[i]; }
    DevBuf<float4> pyr;
    if ((rc = pyr.alloc(n_pyr)) != GNXR_OK) return rc;
    const auto level_ptr = [&](int i) -> const float4 * { return i == 0 ? tex : pyr.p + off[i]; };
    for (int i = 1; i < n_levels; ++i)
        hipLaunchKernelGGL(k_env_pyramid, dim3(grid_for((long long)lw[i] * lh[i])), dim3(kB), 0, st, level_ptr(i - 1), lw[i - 1], lh[i - 1], lw[i], lh[i], pyr.p + off[i]);
    HIP_TRY(hipGetLastError());
    const int first_level = std::max(0, n_levels - 3);
    std::vector<std::vector<float>> top(n_levels - first_level);
    for (int i = first_level; i < n_levels; ++i) {
        top[i - first_level].resize(4 * (size_t)lw[i] * lh[i]);
        HIP_TRY(hipMemcpyAsync(top[i - first_level].data(), level_ptr(i), top[i - first_level].size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    // ---- the sampling image, its Distribution2D and the guide tables
    hipLaunchKernelGGL(k_env_image, dim3(grid_for((long long)W2 * H2)), dim3(kB), 0, st, (const float4 *)tex, rx, ry, r->cond_func.p);
    hipLaunchKernelGGL(k_env_dist1d, dim3(std::min(H2, g_num_cus * 8)), dim3(kB), 0, st, (const float *)r->cond_func.p, W2, H2, r->cond_cdf.p, r->cond_int.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(r->marg_func.p, r->cond_int.p, (size_t)H2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    DevBuf<float> d_mfi;
    if ((rc = d_mfi.alloc(1)) != GNXR_OK) return rc;
    hipLaunchKernelGGL(k_env_dist1d, dim3(1), dim3(kB), 0, st, (const float *)r->marg_func.p, H2, 1, r->marg_cdf.p, d_mfi.p);
    hipLaunchKernelGGL(k_env_guide, dim3(grid_for(kEnvGuideMarg + 1)), dim3(kB), 0, st, (const float *)r->marg_cdf.p, H2 + 1, 1, kEnvGuideMarg, r->marg_guide.p);
    hipLaunchKernelGGL(k_env_guide, dim3(grid_for((long long)H2 * (kEnvGuideCond + 1))), dim3(kB), 0, st, (const float *)r->cond_cdf.p, W2 + 1, H2, kEnvGuideCond, r->cond_guide.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&r->marg_func_int, d_mfi.p, sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    env_power_from_top_levels(rx, ry, first_level, top, r->power);
    r->rx = rx; r->ry = ry;
    return GNXR_OK;
}

// the new tables into a copy: pointer swaps (the old ones are released with `r`), and a new light-selection table at the next render
void env_commit_copy(gnxr_scene *s, EnvBuilt &r) {
    swap_buf(s->env_texels4, r.texels4); swap_buf(s->env_cond_func, r.cond_func); swap_buf(s->env_cond_cdf, r.cond_cdf); swap_buf(s->env_cond_int, r.cond_int);
    swap_buf(s->env_marg_func, r.marg_func); swap_buf(s->env_marg_cdf, r.marg_cdf); swap_buf(s->env_marg_guide, r.marg_guide); swap_buf(s->env_cond_guide, r.cond_guide);
    s->grid_strategy = -1;
}

}  // namespace

extern "C" int gnxr_scene_update_environment(gnxr_scene *s, const gnxr_light *light, const float *rgb, int32_t width, int32_t height, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (!light) { set_error("null light record"); return GNXR_ERR_INVALID; }
    if (light->type != GNXR_LIGHT_INFINITE) { set_error("the record of an environment update must be of type GNXR_LIGHT_INFINITE (got %d)", light->type); return GNXR_ERR_INVALID; }
    if (rgb) {
        if (width <= 0 || height <= 0) { set_error("invalid environment map size %d x %d", width, height); return GNXR_ERR_INVALID; }
        // the guide tables hold cdf indices up to 2 * round_up_pow2(size) + 1 as uint16_t
        if (width > 16384 || height > 16384) {
            set_error("environment map %d x %d: 2 * round_up_pow2(size) + 1 exceeds the 65535 a guide-table entry holds (at most 16384 texels per side)", width, height);
            return GNXR_ERR_INVALID;
        }
    }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    SceneFacts &cs = s->cs;
    int idx = -1;
    for (size_t i = 0; i < cs.desc_lights.size() && idx < 0; ++i)
        if (cs.desc_lights[i].type == GNXR_LIGHT_INFINITE) idx = (int)i;
    if (idx < 0 || !cs.has_env) { set_error("the scene has no INFINITE light, and neither this call nor gnxr_scene_set_lights adds one: create the scene with it"); return GNXR_ERR_UNSUPPORTED; }
    if (!rgb && memcmp(light->le, cs.desc_lights[idx].le, sizeof(light->le)) != 0) {
        set_error("le of the environment light changes its texels: send the map again (the raw map is not retained)");
        return GNXR_ERR_INVALID;
    }
    // the record and the transforms, as compile_scene / build_env make them
    std::vector<DLight> recs = cs.lights;
    if (!compile_light(*light, idx, nullptr, -1, cs.world_bound, &recs[idx])) return GNXR_ERR_INVALID;
    DEnv env = cs.env;   // (the bounding sphere stays: it follows the world bound)
    {
        Mat4 l2w;
        memcpy(l2w.m, light->light_to_world, 64);
        const Mat4 w2l = inverse(l2w);
        memcpy(env.l2w, l2w.m, 64); memcpy(env.w2l, w2l.m, 64);
    }
    int rc = s->bind();
    if (rc) return rc;
    // 1. every device builds into fresh buffers from the raw map: the primary on the caller's stream (one copy path for host and device
    // memory, ordered after what the caller queued there), the others from the primary's staged copy on their null stream
    std::vector<EnvBuilt> built(rgb ? s->n_copies() : 0);
    if (rgb) {
        bool flip_y = false;   // compile_scene's rule: a SKYBOX light earlier in the list has switched the image loader to flipped rows
        for (int k = 0; k < idx; ++k) if (cs.desc_lights[k].type == GNXR_LIGHT_SKYBOX) flip_y = true;
        const size_t nf = (size_t)width * height * 3;
        DevBuf<float> staged;
        rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int {
            int rc_;
            if (i == 0) {
                hipStream_t st = (hipStream_t)hip_stream;
                if ((rc_ = staged.alloc(nf)) != GNXR_OK) return rc_;
                HIP_TRY(hipMemcpyAsync(staged.p, rgb, nf * sizeof(float), hipMemcpyDefault, st));
                return env_build_on_device(c, staged.p, width, height, flip_y, light->le, st, &built[0]);   // (returns with the stream drained)
            }
            DevBuf<float> raw;
            if ((rc_ = raw.alloc(nf)) != GNXR_OK) return rc_;
            HIP_TRY(hipMemcpyPeer(raw.p, c->device, staged.p, s->device, nf * sizeof(float)));
            return env_build_on_device(c, raw.p, width, height, flip_y, light->le, nullptr, &built[i]);
        });
        if (rc) return rc;
        for (size_t i = 1; i < built.size(); ++i)
            if (!built[i].same(built[0])) { set_error("environment update: the devices disagree (internal error)"); return GNXR_ERR_RUNTIME; }
        env.w = built[0].rx; env.h = built[0].ry; env.dw = 2 * built[0].rx; env.dh = 2 * built[0].ry;
        env.marg_func_int = built[0].marg_func_int;
    }
    // 2. the only writes that can still fail: the light records.  A failure puts the host's records, still the old ones, back
    rc = s->apply_or_put_back([&](gnxr_scene *c, size_t) -> int {
        HIP_TRY(hipMemcpy(c->lights.p, recs.data(), recs.size() * sizeof(DLight), hipMemcpyHostToDevice));
        return GNXR_OK;
    }, refit_world);
    if (rc) return rc;
    // 3. the host scene, then the swaps
    cs.lights = std::move(recs);
    cs.desc_lights[idx] = *light;
    cs.env = env;
    if (rgb) {
        memcpy(cs.env_power_lookup, built[0].power, sizeof(cs.env_power_lookup));
        s->host->host_env_stale = true;
    }
    for (size_t i = 0; i < s->n_copies(); ++i) {
        if (rgb) env_commit_copy(s->copy(i), built[i]);
        s->copy(i)->grid_strategy = -1;
    }
    // the old tables are released with `built` (hipFree waits for what still reads them)
    return GNXR_OK;
}

// test hook: one of the environment tables as the first device holds it (which 0 .. 7: env_texels4, env_cond_func, env_cond_cdf,
// env_cond_int, env_marg_func, env_marg_cdf, env_marg_guide, env_cond_guide), the DEnv record renders are given (8) or the Power lookup (9)
extern "C" int gnxr_scene_env_tables(gnxr_scene *s, int32_t which, void *out, int64_t capacity_bytes, int64_t *n_bytes) {
    if (!s || !n_bytes) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (which < 0 || which > 9) { set_error("environment table %d outside [0, 10)", which); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    const DEnv &e = cs.env;
    const size_t W2 = cs.has_env ? e.dw : 0, H2 = cs.has_env ? e.dh : 0, on = cs.has_env ? 1 : 0;
    const void *d_src = nullptr, *h_src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: d_src = s->env_texels4.p; bytes = (size_t)e.w * e.h * on * 16; break;
        case 1: d_src = s->env_cond_func.p; bytes = W2 * H2 * 4; break;
        case 2: d_src = s->env_cond_cdf.p; bytes = (W2 + 1) * H2 * 4; break;
        case 3: d_src = s->env_cond_int.p; bytes = H2 * 4; break;
        case 4: d_src = s->env_marg_func.p; bytes = H2 * 4; break;
        case 5: d_src = s->env_marg_cdf.p; bytes = (H2 + 1) * on * 4; break;
        case 6: d_src = s->env_marg_guide.p; bytes = (size_t)(kEnvGuideMarg + 1) * on * 2; break;
        case 7: d_src = s->env_cond_guide.p; bytes = H2 * (kEnvGuideCond + 1) * 2; break;
        case 8: h_src = &cs.env; bytes = sizeof(DEnv) * on; break;
        default: h_src = cs.env_power_lookup; bytes = sizeof(cs.env_power_lookup) * on; break;
    }
    *n_bytes = (int64_t)bytes;
    if (!out || capacity_bytes < (int64_t)bytes || bytes == 0) return GNXR_OK;
    if (h_src) { memcpy(out, h_src, bytes); return GNXR_OK; }
    if (int rc = s->bind()) return rc;
    HIP_TRY(hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
    return GNXR_OK;
}
