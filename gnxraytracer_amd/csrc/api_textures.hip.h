// api_textures.hip.h -- gnxr_scene_update_textures: host driver of the replacement of image textures of a live scene
// (texture_build_kernel.hip.h), and the test hook gnxr_scene_texture_tables.  Part of api.hip's translation unit (after api_media.hip.h,
// whose structure it follows; swap_buf is api_rebuild.hip.h's).
//
// The records are validated and compiled into a copy first (compile_texture: sizes, levels and offsets of the packed buffer, textures in
// index order, levels 0 .. n - 1 of each in order, no padding -- build_textures' layout).  With new texels every device of the handle then
// builds a FRESH packed texel buffer (tex_build_on_device): the pyramids of the textures the call leaves alone are copied device to
// device, the new ones are built by the kernels.  Only when all devices have built are the DTexture records and the record in front of
// the materials, which holds the buffer's address, written (the device writes that could still fail; a failure puts the old ones back),
// the host scene told once and the buffers swapped into the copies (pointer swaps only), so a refused or failed call leaves the scene as
// it was.  Nothing crosses to the host; what crosses to the device besides the texels: the Lanczos weights of a resampled texture
// (px + py records, computed by the host's resample_weights), the DTexture records and one DTexTables record.  Texels in device memory
// are read where they lie (the replicas take them by peer copy); host memory is staged on the primary once.
#pragma once

namespace {

static_assert(sizeof(DTexture) == 112, "gnxr_scene_texture_tables documents 28 words per record");

// the texels of all levels of a compiled texture
int64_t texture_texels(const DTexture &t) {
    int64_t n = 0;
    for (int i = 0, w = t.w0, h = t.h0; i < t.n_levels; ++i, w = std::max(1, w / 2), h = std::max(1, h / 2)) n += (int64_t)w * h;
    return n;
}

// GNXR_VERBOSE: every kernel launch of the build between two HIP events of its own, reported on stderr once the stream has drained
// (tests/dev_texture_update_time.py reads the lines).  Without the variable nothing is created or recorded.
struct TexLaunchTimes {
    struct Span { hipEvent_t a, b; const char *kernel; int texture; long long texels_out, bytes; };
    std::vector<Span> spans;
    const hipStream_t st;
    const bool on = getenv("GNXR_VERBOSE") != nullptr;
    bool open = false;
    explicit TexLaunchTimes(hipStream_t st_) : st(st_) {}
    ~TexLaunchTimes() { for (Span &e : spans) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); } }
    void begin(const char *kernel, int texture, long long texels_out, long long bytes) {
        Span e{nullptr, nullptr, kernel, texture, texels_out, bytes};
        if (!on || hipEventCreate(&e.a) != hipSuccess) return;
        if (hipEventCreate(&e.b) != hipSuccess) { (void)hipEventDestroy(e.a); return; }
        (void)hipEventRecord(e.a, st);
        spans.push_back(e);
        open = true;
    }
    void end() { if (open) (void)hipEventRecord(spans.back().b, st); open = false; }
    void report(int device) const {
        for (const Span &e : spans) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess)
                fprintf(stderr, "[gnxr] %s: device %d, texture %d, %lld texels, %.1f us, %lld bytes, %.0f GB/s\n", e.kernel, device, e.texture, e.texels_out, ms * 1e3, e.bytes,
                        1e-6 * e.bytes / std::max(ms, 1e-6f));
        }
    }
};

// a kernel templated on the wrap mode, launched for the mode `wrap` (validated: one of the three)
#define GX_TEX_LAUNCH(kernel, wrap, grid, st, ...)                                                                                      \
    do {                                                                                                                                \
        if ((wrap) == GNXR_WRAP_REPEAT) hipLaunchKernelGGL((texb::kernel<GNXR_WRAP_REPEAT>), dim3(grid), dim3(texb::kB), 0, st, __VA_ARGS__); \
        else if ((wrap) == GNXR_WRAP_BLACK) hipLaunchKernelGGL((texb::kernel<GNXR_WRAP_BLACK>), dim3(grid), dim3(texb::kB), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((texb::kernel<GNXR_WRAP_CLAMP>), dim3(grid), dim3(texb::kB), 0, st, __VA_ARGS__);                         \
    } while (0)

// The pyramid of texture `t` (compiled: `rec`, whose level offsets index `packed`) from its raw texels d_rgb (memory of the bound device,
// complete in stream order on st), queued on st.  `temps` keeps the intermediate buffers until the caller has drained the stream.
int tex_build_one(const gnxr_texture &t, int index, const DTexture &rec, const float *d_rgb, float4 *packed, hipStream_t st, std::vector<std::unique_ptr<DevBuf<float4>>> *temps,
                  std::vector<std::unique_ptr<DevBuf<texb::DResampleWeight>>> *weights, TexLaunchTimes *times) {
    using namespace texb;
    int rc;
    const int w = t.width, h = t.height, rx = rec.w0, ry = rec.h0, wrap = t.wrap;
    float4 *level0 = packed + rec.level_offset[0];
    const long long n_raw = (long long)w * h, n0 = (long long)rx * ry;
    if (rx == w && ry == h) {
        times->begin("k_tex_convert", index, n_raw, n_raw * 28);
        hipLaunchKernelGGL(k_tex_convert, dim3(grid_for(n_raw)), dim3(kB), 0, st, d_rgb, w, h, t.scale, t.gamma ? 1 : 0, level0);
        times->end();
    } else {
        static_assert(sizeof(DResampleWeight) == sizeof(EnvResampleWeight), "the device reads the host's weight records");
        const std::vector<EnvResampleWeight> sw = env_resample_weights(w, rx), tw = env_resample_weights(h, ry);
        temps->emplace_back(new DevBuf<float4>()); DevBuf<float4> &raw = *temps->back();
        temps->emplace_back(new DevBuf<float4>()); DevBuf<float4> &res_s = *temps->back();
        weights->emplace_back(new DevBuf<DResampleWeight>()); DevBuf<DResampleWeight> &d_sw = *weights->back();
        weights->emplace_back(new DevBuf<DResampleWeight>()); DevBuf<DResampleWeight> &d_tw = *weights->back();
        if ((rc = raw.alloc((size_t)n_raw)) || (rc = res_s.alloc((size_t)h * rx)) || (rc = d_sw.upload(reinterpret_cast<const DResampleWeight *>(sw.data()), sw.size())) ||
            (rc = d_tw.upload(reinterpret_cast<const DResampleWeight *>(tw.data()), tw.size())))
            return rc;
        times->begin("k_tex_convert", index, n_raw, n_raw * 28);
        hipLaunchKernelGGL(k_tex_convert, dim3(grid_for(n_raw)), dim3(kB), 0, st, d_rgb, w, h, t.scale, t.gamma ? 1 : 0, raw.p);
        times->end();
        times->begin("k_tex_resample_s", index, (long long)h * rx, ((long long)h * rx + n_raw) * 16);
        GX_TEX_LAUNCH(k_tex_resample_s, wrap, grid_for((long long)h * rx), st, (const float4 *)raw.p, w, h, rx, (const DResampleWeight *)d_sw.p, res_s.p);
        times->end();
        times->begin("k_tex_resample_t", index, n0, (n0 + (long long)h * rx) * 16);
        GX_TEX_LAUNCH(k_tex_resample_t, wrap, grid_for(n0), st, (const float4 *)res_s.p, rx, h, ry, (const DResampleWeight *)d_tw.p, level0);
        times->end();
    }
    // the pyramid above level 0: one launch per level while a side exceeds kTailSide, then one launch of one block for the rest
    int lw = rx, lh = ry;
    for (int i = 1; i < rec.n_levels; ++i) {
        const int sres = std::max(1, lw / 2), tres = std::max(1, lh / 2);
        const float4 *below = packed + rec.level_offset[i - 1];
        float4 *lvl = packed + rec.level_offset[i];
        if (std::max(sres, tres) <= kTailSide) {
            times->begin("k_tex_pyramid_tail", index, texture_texels(rec) - (rec.level_offset[i] - rec.level_offset[0]), ((long long)lw * lh + 2ll * sres * tres) * 16);
            GX_TEX_LAUNCH(k_tex_pyramid_tail, wrap, 1, st, below, lw, lh, rec.n_levels - i, lvl);
            times->end();
            break;
        }
        times->begin("k_tex_pyramid", index, (long long)sres * tres, ((long long)lw * lh + (long long)sres * tres) * 16);
        GX_TEX_LAUNCH(k_tex_pyramid, wrap, grid_for((long long)sres * tres), st, below, lw, lh, sres, tres, lvl);
        times->end();
        lw = sres; lh = tres;
    }
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}
#undef GX_TEX_LAUNCH

// The packed texel buffer of the edited texture list (descriptions `descs`, compiled records `recs`, `total` texels) into `r`, on the
// copy's (bound) device: records [first, first + n) are built from d_src + src_off[k] (memory of this device, complete in stream order on
// st), every other texture keeps the pyramid the copy holds.  Returns with the stream drained; nothing of `s` changes.
int tex_build_on_device(gnxr_scene *s, const std::vector<gnxr_texture> &descs, const std::vector<DTexture> &recs, int64_t total, int first, int n, const float *d_src,
                        const std::vector<int64_t> &src_off, hipStream_t st, DevBuf<float> *r) {
    int rc;
    if ((rc = r->alloc(4 * (size_t)total)) != GNXR_OK) return rc;
    float4 *packed = reinterpret_cast<float4 *>(r->p);
    std::vector<std::unique_ptr<DevBuf<float4>>> temps;
    std::vector<std::unique_ptr<DevBuf<texb::DResampleWeight>>> weights;
    TexLaunchTimes times(st);
    for (int i = 0; i < (int)descs.size(); ++i) {
        if (i >= first && i < first + n) {
            if ((rc = tex_build_one(descs[i], i, recs[i], d_src + src_off[i - first], packed, st, &temps, &weights, &times)) != GNXR_OK) return rc;
        } else {
            const DTexture &was = s->cs.textures[i];
            HIP_TRY(hipMemcpyAsync(packed + recs[i].level_offset[0], reinterpret_cast<const float4 *>(s->tex_texels.p) + was.level_offset[0], (size_t)texture_texels(was) * sizeof(float4),
                                   hipMemcpyDeviceToDevice, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    times.report(s->device);
    return GNXR_OK;
}

// One copy's DTexture records and the record in front of its materials, which points at the texel buffer `texels` (an each_copy
// callable's body): towards the buffers the swap will bring in, or back towards what the copy holds
int tex_write_records(gnxr_scene *c, const std::vector<DTexture> &recs, const float *texels) {
    HIP_TRY(hipMemcpy(c->textures.p, recs.data(), recs.size() * sizeof(DTexture), hipMemcpyHostToDevice));
    if (texels == c->tex_texels.p) return GNXR_OK;   // (the buffer stays: so does the record that points at it)
    DTexTables rec = c->tex_tables(c->tri_uv.p, c->tri_n.p, c->tri_s.p);
    rec.texels = reinterpret_cast<const float4 *>(texels);
    HIP_TRY(hipMemcpy(c->materials.p, &rec, sizeof(rec), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->materials_single.p, &rec, sizeof(rec), hipMemcpyHostToDevice));
    return GNXR_OK;
}
// what a failed write puts back: the host scene's records, still the old ones, and the address of the buffer the copy holds
int tex_records_back(gnxr_scene *c, size_t) {
    HIP_TRY(hipMemcpy(c->textures.p, c->cs.textures.data(), c->cs.textures.size() * sizeof(DTexture), hipMemcpyHostToDevice));
    const DTexTables rec = c->tex_tables(c->tri_uv.p, c->tri_n.p, c->tri_s.p);
    HIP_TRY(hipMemcpy(c->materials.p, &rec, sizeof(rec), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->materials_single.p, &rec, sizeof(rec), hipMemcpyHostToDevice));
    return GNXR_OK;
}

}  // namespace

extern "C" int gnxr_scene_update_textures(gnxr_scene *s, int32_t first_texture, int32_t n_textures, const gnxr_texture *textures, const float *texels, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_textures > 0 && !textures) { set_error("null texture array"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    SceneFacts &cs = s->cs;
    const int64_t have = (int64_t)cs.textures.size();   // (the number of textures never changes)
    if (have == 0) { set_error("the scene was created without textures (the texture list of a scene is fixed)"); return GNXR_ERR_UNSUPPORTED; }
    if (first_texture < 0 || n_textures < 0 || (int64_t)first_texture + n_textures > have) {
        set_error("texture range [%d, %lld) outside the scene's %lld textures", first_texture, (long long)first_texture + n_textures, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_textures == 0) return GNXR_OK;
    // 1. the records into a copy, validated as gnxr_scene_create validates them; with texels the whole list is laid out again
    std::vector<gnxr_texture> descs = cs.desc_textures;
    std::vector<DTexture> recs = cs.textures;
    std::vector<int64_t> src_off((size_t)n_textures, 0);
    int64_t src_lo = INT64_MAX, src_hi = 0;   // the floats of `texels` the call reads: [src_lo, src_hi)
    for (int k = 0; k < n_textures; ++k) {
        const int i = first_texture + k;
        const gnxr_texture &t = textures[k];
        int64_t nt = 0;
        DTexture rec;
        if (!compile_texture(t, i, recs[i].level_offset[0], &rec, &nt)) return GNXR_ERR_INVALID;
        if (texels) {
            if (t.texel_offset < 0) { set_error("texture %d: negative texel_offset", i); return GNXR_ERR_INVALID; }
            if (t.texel_offset >= (1ll << 60)) { set_error("texture %d: texel_offset %lld is 2^60 or more", i, (long long)t.texel_offset); return GNXR_ERR_INVALID; }   // (offset + size stays an int64_t)
            src_off[k] = t.texel_offset;
            src_lo = std::min(src_lo, (int64_t)t.texel_offset);
            src_hi = std::max(src_hi, (int64_t)t.texel_offset + (int64_t)t.width * t.height * 3);
        } else {
            const gnxr_texture &was = cs.desc_textures[i];
            if (was.width != t.width || was.height != t.height || was.wrap != t.wrap || (was.gamma != 0) != (t.gamma != 0) || memcmp(&was.scale, &t.scale, sizeof(float)) != 0) {
                set_error("texture %d: width, height, wrap, gamma and scale are baked into the texels and must stay as they are without texels (send the texels)", i);
                return GNXR_ERR_INVALID;
            }
        }
        recs[i] = rec;
        descs[i] = t;
        descs[i].texel_offset = 0;
    }
    int64_t total = 0;
    bool src_on_device = false;
    if (texels) {
        for (size_t i = 0; i < descs.size(); ++i) {
            int64_t nt = 0;
            if (!compile_texture(descs[i], (int)i, total, &recs[i], &nt)) return GNXR_ERR_INVALID;   // (the offsets again, now that every size is known)
            total += nt;
        }
        if (total >= (1ll << 31)) { set_error("the textures of the scene would hold %lld texels (2^31 or more)", (long long)total); return GNXR_ERR_INVALID; }
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, texels);
        (void)hipGetLastError();
        src_on_device = e == hipSuccess && at.type == hipMemoryTypeDevice;
        if (src_on_device && at.device != s->device) { set_error("texels live on device %d, the scene's first device is %d", at.device, s->device); return GNXR_ERR_INVALID; }
    }
    int rc = s->bind();
    if (rc) return rc;
    // 2. every device builds a fresh texel buffer: the primary on the caller's stream (ordered after what the caller queued there), the
    // others from the primary's memory on their null stream
    std::vector<DevBuf<float>> built(texels ? s->n_copies() : 0);
    if (texels) {
        const size_t nf = (size_t)(src_hi - src_lo);
        std::vector<int64_t> rel(src_off);   // offsets into a buffer that starts at float src_lo of `texels`
        for (int64_t &o : rel) o -= src_lo;
        DevBuf<float> staged;                // host memory: staged once, on the primary
        const float *d_first = texels + src_lo;
        rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int {
            int rc_;
            if (i == 0) {
                hipStream_t st = (hipStream_t)hip_stream;
                if (!src_on_device) {
                    if ((rc_ = staged.alloc(nf)) != GNXR_OK) return rc_;
                    HIP_TRY(hipMemcpyAsync(staged.p, texels + src_lo, nf * sizeof(float), hipMemcpyDefault, st));
                    d_first = staged.p;
                }
                return tex_build_on_device(c, descs, recs, total, first_texture, n_textures, d_first, rel, st, &built[0]);   // (returns with the stream drained)
            }
            DevBuf<float> raw;
            if ((rc_ = raw.alloc(nf)) != GNXR_OK) return rc_;
            HIP_TRY(hipMemcpyPeer(raw.p, c->device, d_first, s->device, nf * sizeof(float)));
            return tex_build_on_device(c, descs, recs, total, first_texture, n_textures, raw.p, rel, nullptr, &built[i]);
        });
        if (rc) return rc;
    }
    // 3. the only writes that can still fail: the texture records and the address of the new buffer.  A failure puts the old ones back
    rc = s->apply_or_put_back([&](gnxr_scene *c, size_t i) -> int { return tex_write_records(c, recs, texels ? built[i].p : c->tex_texels.p); }, tex_records_back);
    if (rc) return rc;
    // 4. the host scene, then the swaps (the old buffers are released with `built`: hipFree waits for what still reads them)
    cs.desc_textures = std::move(descs);
    cs.textures = std::move(recs);
    if (texels)
        for (size_t i = 0; i < s->n_copies(); ++i) swap_buf(s->copy(i)->tex_texels, built[i]);
    return GNXR_OK;
}

// test hook: the DTexture records of all textures as the first device holds them (which 0), or the float4 texels of all levels of one
// texture, level after level, each read through its record's offset (which 1)
extern "C" int gnxr_scene_texture_tables(gnxr_scene *s, int32_t which, int32_t texture, void *out, int64_t capacity_bytes, int64_t *n_bytes) {
    if (!s || !n_bytes) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (which < 0 || which > 1) { set_error("texture table %d outside [0, 2)", which); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    const size_t n = cs.textures.size();
    if (which == 1 && (texture < 0 || (size_t)texture >= n)) { set_error("texture %d outside the scene's %zu textures", texture, n); return GNXR_ERR_INVALID; }
    const size_t bytes = which == 0 ? n * sizeof(DTexture) : (size_t)texture_texels(cs.textures[texture]) * sizeof(float4);
    *n_bytes = (int64_t)bytes;
    if (!out || capacity_bytes < (int64_t)bytes || bytes == 0) return GNXR_OK;
    if (int rc = s->bind()) return rc;
    if (which == 0) {
        HIP_TRY(hipMemcpy(out, s->textures.p, bytes, hipMemcpyDeviceToHost));
        return GNXR_OK;
    }
    DTexture rec;
    HIP_TRY(hipMemcpy(&rec, s->textures.p + texture, sizeof(DTexture), hipMemcpyDeviceToHost));
    if (texture_texels(rec) * (int64_t)sizeof(float4) != (int64_t)bytes) { set_error("texture %d: the device's record disagrees with the host's (internal error)", texture); return GNXR_ERR_RUNTIME; }
    char *dst = static_cast<char *>(out);
    for (int i = 0, w = rec.w0, h = rec.h0; i < rec.n_levels; ++i, w = std::max(1, w / 2), h = std::max(1, h / 2)) {
        const size_t lb = (size_t)w * h * sizeof(float4);
        HIP_TRY(hipMemcpy(dst, reinterpret_cast<const float4 *>(s->tex_texels.p) + rec.level_offset[i], lb, hipMemcpyDeviceToHost));
        dst += lb;
    }
    return GNXR_OK;
}
