// api_media.hip.h -- gnxr_scene_update_media: host driver of the replacement of density grids and medium records of a live scene
// (media_kernel.hip.h), and the test hook gnxr_scene_media_tables.  Part of api.hip's translation unit (after api_env.hip.h, whose
// structure it follows; swap_buf is api_rebuild.hip.h's).
//
// The records are validated and compiled into a copy first.  With new grids every device of the handle then builds a FRESH packed grid
// buffer (media_build_on_device): the grids of the media the call leaves alone are copied device to device, the new ones are written
// by k_media_grid, which finds their maxima in the same pass.  Only when all devices have built, and agree on every maximum, are the
// DMedium records written (the one device write that could still fail; a failure puts the host's records, still the old ones, back),
// the host scene told once and the buffers swapped into the copies (pointer swaps only), so a refused or failed call leaves the scene
// as it was.  What crosses to the host: one float per new grid; what crosses to the device besides the grids: the DMedium records.
// A density in device memory is read where it lies (the replicas take it by peer copy); host memory is staged on the primary once.
#pragma once

namespace {

static_assert(sizeof(DMedium) == 128, "gnxr_scene_media_tables documents 32 words per record");

// where every GRID medium's grid sits in a packed buffer: 16-byte aligned starts, in medium order
struct MediaLayout {
    std::vector<int64_t> offset;   // per medium, -1: no grid
    int64_t total = 0;             // floats
};

MediaLayout media_layout(const std::vector<gnxr_medium> &media) {
    MediaLayout l;
    l.offset.assign(media.size(), -1);
    for (size_t i = 0; i < media.size(); ++i) {
        const gnxr_medium &m = media[i];
        if (m.type != GNXR_MEDIUM_GRID) continue;
        l.offset[i] = l.total;
        l.total += ((int64_t)m.nx * m.ny * m.nz + 3) / 4 * 4;
    }
    return l;
}

struct MediaBuilt {
    DevBuf<float> grids;
    std::vector<float> maxima;   // per record of the call (0 for a HOMOGENEOUS one): every device finds the same ones
    bool same(const MediaBuilt &o) const { return maxima.size() == o.maxima.size() && (maxima.empty() || memcmp(maxima.data(), o.maxima.data(), maxima.size() * sizeof(float)) == 0); }
};

// GNXR_VERBOSE: every k_media_grid launch between two HIP events of its own, reported on stderr once the stream has drained
// (tests/dev_media_update_time.py reads the lines).  Without the variable nothing is created or recorded.
struct LaunchTimes {
    struct Span { hipEvent_t a, b; long long voxels; };
    std::vector<Span> spans;
    const hipStream_t st;
    const bool on = getenv("GNXR_VERBOSE") != nullptr;
    explicit LaunchTimes(hipStream_t st_) : st(st_) {}
    ~LaunchTimes() { for (Span &e : spans) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); } }
    void begin(long long voxels) {
        Span e{nullptr, nullptr, voxels};
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
                fprintf(stderr, "[gnxr] k_media_grid: device %d, %lld voxels, %.1f us, %.0f GB/s (8 B per voxel)\n", device, e.voxels, ms * 1e3, 8e-6 * e.voxels / std::max(ms, 1e-6f));
        }
    }
    bool open = false;
};

// The packed grid buffer of the edited media list `media` (laid out by `lay`) into `r`, on the copy's (bound) device: records
// [first, first + n) take their grids from d_src + src_off[k] (memory of this device, complete in stream order on st), every other GRID
// medium keeps the grid the copy holds.  Returns with the stream drained; nothing of `s` changes.
int media_build_on_device(gnxr_scene *s, const std::vector<gnxr_medium> &media, const MediaLayout &lay, int first, int n, const float *d_src, const std::vector<int64_t> &src_off,
                          hipStream_t st, MediaBuilt *r) {
    int rc;
    DevBuf<float> d_max;
    if ((rc = r->grids.alloc((size_t)lay.total)) || (rc = d_max.alloc((size_t)n))) return rc;
    r->maxima.assign((size_t)n, 0.f);
    HIP_TRY(hipMemsetAsync(d_max.p, 0, (size_t)n * sizeof(float), st));   // +0: where every fold starts
    LaunchTimes times(st);
    for (int i = 0; i < (int)media.size(); ++i) {
        if (lay.offset[i] < 0) continue;
        const int64_t nv = (int64_t)media[i].nx * media[i].ny * media[i].nz;
        float *dst = r->grids.p + lay.offset[i];
        if (i >= first && i < first + n) {
            const int k = i - first;
            times.begin(nv);
            hipLaunchKernelGGL(mediab::k_media_grid, dim3(grid_for((nv + 3) / 4)), dim3(mediab::kB), 0, st, d_src + src_off[k], dst, nv, d_max.p + k);
            times.end();
        } else {
            HIP_TRY(hipMemcpyAsync(dst, s->grid_density.p + s->cs.dmedia[i].density_offset, (size_t)nv * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(r->maxima.data(), d_max.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    times.report(s->device);
    return GNXR_OK;
}

// one copy's medium records from the host scene's (an each_copy callable): what a failed write puts back
int media_records_back(gnxr_scene *s, size_t) {
    HIP_TRY(hipMemcpy(s->dmedia.p, s->cs.dmedia.data(), s->cs.dmedia.size() * sizeof(DMedium), hipMemcpyHostToDevice));
    return GNXR_OK;
}

}  // namespace

extern "C" int gnxr_scene_update_media(gnxr_scene *s, int32_t first_medium, int32_t n_media, const gnxr_medium *media, const float *density, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_media > 0 && !media) { set_error("null medium array"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    SceneFacts &cs = s->cs;
    const int64_t have = (int64_t)cs.media.size();   // (the number of media never changes)
    if (have == 0) { set_error("the scene was created without media (the medium list of a scene is fixed)"); return GNXR_ERR_UNSUPPORTED; }
    if (first_medium < 0 || n_media < 0 || (int64_t)first_medium + n_media > have) {
        set_error("medium range [%d, %lld) outside the scene's %lld media", first_medium, (long long)first_medium + n_media, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_media == 0) return GNXR_OK;
    // 1. the records into a copy, validated as gnxr_scene_create validates them (compile_medium; the maxima follow from the devices)
    std::vector<gnxr_medium> descs = cs.media;
    std::vector<DMedium> recs = cs.dmedia;
    std::vector<int64_t> src_off((size_t)n_media, 0);
    int64_t src_lo = INT64_MAX, src_hi = 0;   // the floats of `density` the call reads: [src_lo, src_hi)
    for (int k = 0; k < n_media; ++k) {
        const int i = first_medium + k;
        const gnxr_medium &m = media[k];
        if (!compile_medium(m, i, 0.f, &recs[i])) return GNXR_ERR_INVALID;
        descs[i] = m;
        if (m.type != GNXR_MEDIUM_GRID) continue;
        if ((int64_t)m.nx * m.ny >= (1ll << 31) || (int64_t)m.nx * m.ny * m.nz >= (1ll << 31)) {   // (compile_scene's limit; no product here overflows)
            set_error("medium %d: density grid %d x %d x %d too large (2^31 floats or more)", i, m.nx, m.ny, m.nz);
            return GNXR_ERR_INVALID;
        }
        const int64_t nv = (int64_t)m.nx * m.ny * m.nz;
        if (density) {
            if (m.density_offset < 0) { set_error("medium %d: negative density_offset", i); return GNXR_ERR_INVALID; }
            if (m.density_offset >= (1ll << 60)) { set_error("medium %d: density_offset %lld is 2^60 or more", i, (long long)m.density_offset); return GNXR_ERR_INVALID; }   // (offset + size stays an int64_t)
            src_off[k] = m.density_offset;
            src_lo = std::min(src_lo, (int64_t)m.density_offset);
            src_hi = std::max(src_hi, (int64_t)m.density_offset + nv);
        } else {
            const gnxr_medium &was = cs.media[i];
            if (was.type != GNXR_MEDIUM_GRID || was.nx != m.nx || was.ny != m.ny || was.nz != m.nz) {
                set_error("medium %d: a GRID record without density must name a medium that is GRID now, with the same resolution (send the grid)", i);
                return GNXR_ERR_INVALID;
            }
            recs[i].inv_max_density = cs.dmedia[i].inv_max_density;   // the grid stays, and where it sits
            recs[i].density_offset = cs.dmedia[i].density_offset;
        }
    }
    const bool new_grids = density && src_hi > 0;   // (records without a GRID among them: coefficients only, whatever `density` is)
    MediaLayout lay;
    bool src_on_device = false;
    if (new_grids) {
        lay = media_layout(descs);
        if (lay.total >= (1ll << 31)) { set_error("the density grids of the scene would hold %lld floats (2^31 or more)", (long long)lay.total); return GNXR_ERR_INVALID; }
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, density);
        (void)hipGetLastError();
        src_on_device = e == hipSuccess && at.type == hipMemoryTypeDevice;
        if (src_on_device && at.device != s->device) { set_error("density lives on device %d, the scene's first device is %d", at.device, s->device); return GNXR_ERR_INVALID; }
    }
    int rc = s->bind();
    if (rc) return rc;
    // 2. every device builds a fresh grid buffer: the primary on the caller's stream (ordered after what the caller queued there), the
    // others from the primary's memory on their null stream
    std::vector<MediaBuilt> built(new_grids ? s->n_copies() : 0);
    if (new_grids) {
        const size_t nf = (size_t)(src_hi - src_lo);
        std::vector<int64_t> rel(src_off);   // offsets into a buffer that starts at float src_lo of `density`
        for (int k = 0; k < n_media; ++k) rel[k] = media[k].type == GNXR_MEDIUM_GRID ? src_off[k] - src_lo : 0;
        DevBuf<float> staged;                // host memory: staged once, on the primary
        const float *d_first = density + src_lo;
        rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int {
            int rc_;
            if (i == 0) {
                hipStream_t st = (hipStream_t)hip_stream;
                if (!src_on_device) {
                    if ((rc_ = staged.alloc(nf)) != GNXR_OK) return rc_;
                    HIP_TRY(hipMemcpyAsync(staged.p, density + src_lo, nf * sizeof(float), hipMemcpyDefault, st));
                    d_first = staged.p;
                }
                return media_build_on_device(c, descs, lay, first_medium, n_media, d_first, rel, st, &built[0]);   // (returns with the stream drained)
            }
            DevBuf<float> raw;
            if ((rc_ = raw.alloc(nf)) != GNXR_OK) return rc_;
            HIP_TRY(hipMemcpyPeer(raw.p, c->device, d_first, s->device, nf * sizeof(float)));
            return media_build_on_device(c, descs, lay, first_medium, n_media, raw.p, rel, nullptr, &built[i]);
        });
        if (rc) return rc;
        for (size_t i = 1; i < built.size(); ++i)
            if (!built[i].same(built[0])) { set_error("media update: the devices disagree (internal error)"); return GNXR_ERR_RUNTIME; }
        for (int k = 0; k < n_media; ++k)
            if (media[k].type == GNXR_MEDIUM_GRID && !compile_medium(media[k], first_medium + k, built[0].maxima[k], &recs[first_medium + k])) return GNXR_ERR_INVALID;
        for (size_t i = 0; i < descs.size(); ++i)
            if (lay.offset[i] >= 0) recs[i].density_offset = (int32_t)lay.offset[i];
    }
    // 3. the only writes that can still fail: the medium records.  A failure puts the host's records, still the old ones, back
    rc = s->apply_or_put_back([&](gnxr_scene *c, size_t) -> int {
        HIP_TRY(hipMemcpy(c->dmedia.p, recs.data(), recs.size() * sizeof(DMedium), hipMemcpyHostToDevice));
        return GNXR_OK;
    }, media_records_back);
    if (rc) return rc;
    // 4. the host scene, then the swaps (the old buffers are released with `built`: hipFree waits for what still reads them)
    cs.media = std::move(descs);
    cs.dmedia = std::move(recs);
    if (new_grids)
        for (size_t i = 0; i < s->n_copies(); ++i) swap_buf(s->copy(i)->grid_density, built[i].grids);
    return GNXR_OK;
}

// test hook: the DMedium records of all media as the first device holds them, density_offset written as 0 (which 0), or the floats of
// one medium's grid, read through its record's offset (which 1)
extern "C" int gnxr_scene_media_tables(gnxr_scene *s, int32_t which, int32_t medium, void *out, int64_t capacity_bytes, int64_t *n_bytes) {
    if (!s || !n_bytes) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (which < 0 || which > 1) { set_error("media table %d outside [0, 2)", which); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    const size_t n = cs.media.size();
    if (which == 1 && (medium < 0 || (size_t)medium >= n)) { set_error("medium %d outside the scene's %zu media", medium, n); return GNXR_ERR_INVALID; }
    const size_t bytes = which == 0 ? n * sizeof(DMedium)
                                    : (cs.media[medium].type == GNXR_MEDIUM_GRID ? (size_t)cs.media[medium].nx * cs.media[medium].ny * cs.media[medium].nz * sizeof(float) : 0);
    *n_bytes = (int64_t)bytes;
    if (!out || capacity_bytes < (int64_t)bytes || bytes == 0) return GNXR_OK;
    if (int rc = s->bind()) return rc;
    if (which == 0) {
        HIP_TRY(hipMemcpy(out, s->dmedia.p, bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) static_cast<DMedium *>(out)[i].density_offset = 0;
        return GNXR_OK;
    }
    DMedium rec;
    HIP_TRY(hipMemcpy(&rec, s->dmedia.p + medium, sizeof(DMedium), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out, s->grid_density.p + rec.density_offset, bytes, hipMemcpyDeviceToHost));
    return GNXR_OK;
}
