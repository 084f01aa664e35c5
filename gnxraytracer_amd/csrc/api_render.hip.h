// api_render.hip.h -- the render path: launch plan (RenderPlan), per-render state (RenderState's member functions), the stages of a
// render in progress (RenderRun), the three loops, render_one and render_sharded.  Part of api.hip's translation unit (after api_scene.hip.h).
#pragma once

// Launch shape of a traversal kernel (k_trace4 when `wide`, else k_trace) over `total` work items: LDS stack levels, LDS bytes, cached
// top nodes and persistent blocks.  The render's trace stage and the batched queries size their launches here.
struct TraceLaunch {
    int entries;       // deepest stack the walk can need
    int lds_entries;   // of which live in LDS (the rest spill to global memory: spill_needed)
    bool spill_needed;
    size_t lds;        // dynamic LDS bytes per block
    int n_top;         // 4-wide nodes served from the block's LDS copy
    int hot_bytes;     // LDS bytes for the leaves those nodes reference (0: no hot table)
    int blocks;
};
static TraceLaunch trace_launch(const gnxr_scene *s, bool wide, bool spheres, long long total) {
    TraceLaunch t;
    // LDS traversal stack: one column per lane, depth from the BVH (binary walk: depth + 1; 4-wide walk: stack4_need)
    t.entries = wide ? s->cs.stack4_need + 1 : s->cs.bvh_max_depth + 2;
    // 5 blocks of 4 waves per CU is what k_trace4's 96 VGPRs allow (5 waves per SIMD); the LDS of a block -- stack levels plus, for
    // the 4-wide kernel, the set-up ray records and the node cache -- must fit 5 times into the 160 KB; deeper levels spill to
    // global memory (LDS levels are worth more than a bigger node cache: profiles/README.md, r02 A/B table)
    const int per_cu = g_trace_blocks_per_cu;
    // besides the stack: the set-up ray records, the top-of-tree node cache, the order table and the hot leaves
    const size_t fixed_b = wide ? (size_t)(kRayRecDwords + (spheres ? 1 : 0)) * kRqStride * sizeof(int) + (size_t)kTopCache * 128 + kOrderTableBytes + kHotBytes : 0;
    t.lds_entries = std::min(std::min(t.entries, Knobs::trace_lds_levels()), std::max(2, (int)(((160 * 1024) / per_cu - 1024 - fixed_b) / (kBlock * sizeof(int)))));
    t.spill_needed = t.entries > t.lds_entries;
    t.lds = (size_t)t.lds_entries * kBlock * sizeof(int) + fixed_b;
    t.n_top = (int)std::min<size_t>(kTopCache, s->cs.root4 >= 0 ? s->cs.n_nodes4 : 0);
    // (a hot reference takes its offset from the top of the 24-bit range: a scene with that many triangles keeps the global path)
    t.hot_bytes = (wide && t.n_top > 0 && s->cs.n_triangles < (size_t)kHotBase) ? kHotBytes : 0;
    // persistent waves: enough blocks to fill the chip, never more than the work needs
    t.blocks = (int)std::min<long long>((long long)g_num_cus * per_cu, (total + kBlock - 1) / kBlock);
    return t;
}

static int count_local_rows(const gnxr_render_params *p) {
    int rows = 0;
    for (int y = 0; y < p->height; ++y)
        if ((y / p->shard_rows) % p->shard_count == p->shard_index) ++rows;
    return rows;
}

// gnxr_li_device: where the paths of render_one's loops come from and where their radiance goes when they do not come from the camera.
// The loops then work on chunks of `n` caller rays (k_raygen_rays) instead of sub-passes of samples per pixel, and a finished chunk is
// stored per ray (k_store_li) instead of being summed into the image (li_kernel.hip.h).  All three arrays are device memory.
struct RaySource {
    const gnxr_ray *rays;
    const gnxr_li_sample *samples;
    float *L;                     // float4 per ray
    long long n;
};

// gnxr_render_views_device: the cameras of render_one's loops when a call renders several views.  The V views are one path population of
// V * W * H pixels per sample (views_kernel.hip.h): the loops size their passes on it, and the image is the V images one after the other.
struct ViewSource {
    const gnxr_camera *cameras;   // host memory, n_views records
    const int32_t *media;         // host memory, n_views entries in [-1, n_media) (checked by the caller), or nullptr: all -1
    int n_views;
};

// gnxr_render_filtered_device: the film that takes the place of k_resolve / k_finish (film_kernel.hip.h).  A finished sub-pass is added to the
// accumulator layer by layer -- a sample's film offset is recomputed from its Halton index while its tile is staged, so the path state
// does not grow -- and the image is resolved from the accumulator at the end.
struct FilmSource {
    FilmFilter f;
    FilmTable tab;
    float4 *accum;                // device memory, (npix, 4): the caller's accumulator, or nullptr: the handle's (RenderState::accum)
    bool keep;                    // the caller's accumulator continues (GNXR_FILM_CONTINUE); else it is zeroed first
};

static FilmImage film_image(int W, int H, int n_views) {
    FilmImage im;
    im.W = W; im.H = H;
    im.npix = (long long)n_views * W * H;
    im.tiles_x = (W + kFilmTile - 1) / kFilmTile;
    im.tiles_y = (H + kFilmTile - 1) / kFilmTile;
    im.n_tiles = (long long)n_views * im.tiles_y * im.tiles_x;
    return im;
}
// blocks of a k_film_add launch: one per tile while the device has room for them (a block's LDS, ~15 KB, lets ten share a CU)
static int film_grid(const FilmImage &im) { return grid_for(im.n_tiles * kBlock, 32); }

// gnxr_render_adaptive_device: the pixels of render_one's loops when they stop at different sample counts (adaptive_kernel.hip.h,
// api_adaptive.hip.h).  The call works in rounds; the unit of work of a round is one path (as for caller rays), path j of a round being
// sample n0 + j / n_active of active pixel j % n_active, and a finished chunk is added to the per-pixel sums in chunk order.
struct PixelListSource {
    gnxr_adaptive_params ap;
    int32_t *count_out;           // device memory, (H, W) int32, or nullptr
    PixelRound round;             // the round in progress (run_adaptive)
    int rounds;                   // what the call did (run_adaptive): rounds, samples over all pixels, pixels that reached spp
    long long samples, at_budget;
};

// The schedule: samples a round gives every active pixel that has taken n0 so far.  Round 0 takes min_spp; a later round step_spp, or an
// eighth of what the pixel has (rounded down) where that is more, cut at the budget.  The growing steps keep the number of rounds
// logarithmic in spp / step_spp -- every round ends with a drain of the path loop ("Adaptive sampling") -- and a late decision
// comes at most 12.5 % of a pixel's samples after the point where a fixed step would have taken it.
constexpr int kAdaptiveGrowth = 8;
static int adaptive_round_samples(const gnxr_adaptive_params &ap, int spp, int n0) {
    return n0 == 0 ? ap.min_spp : std::min(std::max(ap.step_spp, n0 / kAdaptiveGrowth), spp - n0);
}

// ---- the launch plan ----
// What render_one decides before it allocates or enqueues anything.  plan_render() fills the part that needs no device (it runs before the
// handle is locked), RenderPlan::size_passes() the pass sizes, which depend on the free device memory (after the bind and the light grid).
struct RenderPlan {
    gnxr_render_params p;                       // normalised: shard_count / shard_rows >= 1, spp_end set
    bool direct, volpath, whitted;              // whitted: Whitted and DirectLighting share the depth-first state machine of whitted_kernel.hip.h
    int wmode;
    int n_records, max_light_samples;           // NEE records per vertex, and the largest Light::nSamples (the array samples multiply the Halton index by it)
    bool textured_scene;                        // an image-textured material (shade class 3) is present
    int class_mask;                             // bit c: a material of shade class c is present
    bool area_only, area_env_only;              // the light set (selects the shade kernels' LT_* specialisation)
    bool escape_queue;                          // escaped continuation rays get shade queue 3 to themselves
    int queue_kernel[4];                        // PathIntegrator: the kernel behind each of the four shade queues (SHADE_Q_*, plan_shade_queues)
    unsigned kind_queue;                        // byte k: the shade queue of the class-1 materials of kind k (k_compact<COMPACT_HITCLASS>)
    bool caller_rays;                           // RaySource: no image
    int n_views;                                // ViewSource: views of the call, else 0
    bool pixel_list;                            // PixelListSource: rounds over lists of pixels; a unit is one path, unit_end the paths of the largest round
    int local_rows, npix;
    long long unit, unit_begin, unit_end;       // the unit of work the loops cut into passes: one sample of every pixel (npix paths), or one caller ray
    int spill_entries;                          // deepest traversal stack either BVH layout can need (sizes trace_spill)
    // size_passes():
    int k, in_flight;                           // units per (sub-)pass, sub-passes alive at once (PathIntegrator)
    size_t half, cap, nrec;                     // slots of one region, of all regions; NEE records kept per slot

    bool path_int() const { return !whitted && !volpath; }
    int nsamples() const { return p.spp_end - p.spp_begin; }
    int size_passes(size_t slots_held, bool have_mem, size_t free_b);
};

// What a shade queue of the PathIntegrator launches (RenderRun::shade_stage)
enum ShadeQueueKernel { SHADE_Q_NONE = 0, SHADE_Q_DIFFUSE, SHADE_Q_GLOSSY, SHADE_Q_CONDUCTOR, SHADE_Q_ROUGH_DIELECTRIC, SHADE_Q_ALL, SHADE_Q_TEX, SHADE_Q_ESCAPE };

// The four shade queues of the binning pass.  Queue c belongs to shade class c (0 diffuse, 1 glossy, 2 any lobe, 3 image textures -- or,
// without them, escaped rays).  The class-1 materials come in kinds (material_kind): where the queues that the scene leaves free suffice,
// every kind present gets a queue and the kernel compiled for it -- a wave then holds lanes of one material kind, and the conductor and
// rough-dielectric kernels carry none of the other's code.  Needed are class 0, the kinds present, class 2 and class 3 / the escape queue
// if present; beyond four, all class-1 materials share queue 1 and k_shade<LM_GLOSSY>.  Sphere hits get their class from the traversal
// kernels (pclass), which know no kinds: a scene with spheres keeps the shared queue.
static void plan_shade_queues(const SceneFacts &cs, RenderPlan *pl) {
    int *qk = pl->queue_kernel;
    qk[0] = SHADE_Q_DIFFUSE;
    qk[1] = (pl->class_mask & 2) ? SHADE_Q_GLOSSY : SHADE_Q_NONE;
    qk[2] = (pl->class_mask & 4) ? SHADE_Q_ALL : SHADE_Q_NONE;
    qk[3] = (pl->class_mask & 8) ? SHADE_Q_TEX : (pl->escape_queue ? SHADE_Q_ESCAPE : SHADE_Q_NONE);
    pl->kind_queue = 0x01010101u;
    int kinds = 0, n_kinds = 0;
    for (const DMaterial &m : cs.materials) if (m.shade_class == 1) kinds |= 1 << material_kind(m);
    for (int k = 0; k < MATERIAL_KINDS; ++k) n_kinds += (kinds >> k) & 1;
    const int n_free = 1 + (qk[2] == SHADE_Q_NONE ? 1 : 0) + (qk[3] == SHADE_Q_NONE ? 1 : 0);
    if (!pl->path_int() || cs.n_spheres > 0 || (kinds & ~1) == 0 || n_kinds > n_free || Knobs::no_material_queues()) return;
    const bool narrow = !Knobs::no_narrow_shade();
    pl->kind_queue = 0;
    for (int k = 0, q = 1; k < MATERIAL_KINDS; ++k) {
        if (!((kinds >> k) & 1)) { pl->kind_queue |= 1u << (8 * k); continue; }   // (no triangle has this kind)
        while (q < 3 && qk[q] != SHADE_Q_NONE && !(q == 1 && qk[1] == SHADE_Q_GLOSSY)) ++q;   // (n_kinds <= n_free: a free queue exists)
        qk[q] = !narrow ? SHADE_Q_GLOSSY : (k == MATERIAL_KIND_CONDUCTOR ? SHADE_Q_CONDUCTOR : (k == MATERIAL_KIND_ROUGH_DIELECTRIC ? SHADE_Q_ROUGH_DIELECTRIC : SHADE_Q_GLOSSY));
        pl->kind_queue |= (unsigned)q << (8 * k);
        ++q;
    }
}

// The plan rules that tests/test_full_scale.py restates
static const long long kSubPassPaths = 64ll << 20;                          // PathIntegrator: paths of an automatic sub-pass
static const unsigned long long kSlotBytesEstimate = 238;                    // path state per slot as the in-flight rule counts it (not RenderState::state_bytes)
static const double kStateFreeFraction = 0.45;                              // of the free memory that new path state may take
static const unsigned long long kStateCapBytes = 150ull * 1000 * 1000 * 1000;   // never more path state than this

// Validates the parameters and derives what follows from them and the scene alone.  No device is touched.
static int plan_render(const SceneFacts &cs, const gnxr_render_params *pin, const RaySource *src, const ViewSource *views, const PixelListSource *pix, RenderPlan *out) {
    RenderPlan &pl = *out;
    gnxr_render_params &p = pl.p;
    p = *pin;
    if (p.shard_count <= 0) p.shard_count = 1;
    if (p.shard_rows <= 0) p.shard_rows = 1;
    if (p.spp_end <= 0) p.spp_end = p.spp;
    if (!image_and_samples_ok(p) || p.shard_index < 0 || p.shard_index >= p.shard_count || p.max_depth < 0 || p.max_depth > 250) return invalid_render_params();
    if (p.integrator != GNXR_INTEGRATOR_PATH && p.integrator != GNXR_INTEGRATOR_VOLPATH && p.integrator != GNXR_INTEGRATOR_WHITTED &&
        p.integrator != GNXR_INTEGRATOR_DIRECT) {
        set_error("unknown integrator %d", p.integrator);
        return GNXR_ERR_UNSUPPORTED;
    }
    pl.direct = p.integrator == GNXR_INTEGRATOR_DIRECT;
    if (pl.direct && p.direct_strategy != GNXR_DIRECT_SAMPLE_ALL && p.direct_strategy != GNXR_DIRECT_SAMPLE_ONE) {
        set_error("unknown direct-lighting strategy %d", p.direct_strategy);
        return GNXR_ERR_INVALID;
    }
    pl.volpath = p.integrator == GNXR_INTEGRATOR_VOLPATH;
    pl.whitted = p.integrator == GNXR_INTEGRATOR_WHITTED || pl.direct;
    pl.wmode = !pl.direct ? WM_WHITTED : (p.direct_strategy == GNXR_DIRECT_SAMPLE_ONE ? WM_DIRECT_ONE : WM_DIRECT_ALL);
    pl.n_records = (int)cs.desc_lights.size();
    pl.max_light_samples = 1;
    if (pl.wmode == WM_DIRECT_ONE) pl.n_records = 1;
    if (pl.wmode == WM_DIRECT_ALL) {
        pl.n_records = 0;
        for (const gnxr_light &l : cs.desc_lights) { pl.n_records += std::max(1, l.n_samples); pl.max_light_samples = std::max(pl.max_light_samples, l.n_samples); }
        pl.n_records = std::max(1, pl.n_records);
    }
    // (media in the scene are fine: these integrators never look at them -- a medium boundary without material is passed
    // through by the main ray, WhittedIntegrator.cpp:34-35, and blocks shadow rays like any other surface, Light.cpp:28-31)
    if (pl.whitted && (pl.n_records > 256 || p.max_depth > 32)) {
        set_error("Whitted / DirectLighting on the device: at most 256 light samples per vertex (every light is sampled at every vertex), depth 32");
        return GNXR_ERR_UNSUPPORTED;
    }
    pl.class_mask = 0;
    for (const DMaterial &m : cs.materials) pl.class_mask |= 1 << m.shade_class;
    pl.textured_scene = (pl.class_mask & 8) != 0;
    if (src && pl.textured_scene && (pl.whitted || pl.volpath)) {
        // (their texture lookups at the first vertex take the camera's ray differentials, whitted_kernel.hip.h / vol_kernel.hip.h; caller
        // rays carry none.  PathIntegrator drops them: PathIntegrator.cpp:67)
        set_error("Li for caller rays: Whitted, DirectLighting and VolPath need camera ray differentials on scenes with image textures");
        return GNXR_ERR_UNSUPPORTED;
    }
    if (pix && pl.textured_scene && (pl.whitted || pl.volpath)) {
        // (their shade kernels find the camera's ray differentials through slot % npix: whitted_kernel.hip.h / vol_kernel.hip.h; the slots
        // of a round hold a list of pixels.  PathIntegrator drops the differentials)
        set_error("adaptive: Whitted, DirectLighting and VolPath take the pixel of a path from its slot on scenes with image textures; PathIntegrator renders them");
        return GNXR_ERR_UNSUPPORTED;
    }
    if (views && pl.textured_scene && pl.volpath) {
        // (k_vol_step recomputes the camera's offset rays at the first surface from DRender::cam, vol_kernel.hip.h: the one camera read
        // inside a shade kernel.  Whitted / DirectLighting store them per path at raygen, PathIntegrator drops them: both render views)
        set_error("views: VolPath on a scene with image textures recomputes the camera's ray differentials inside its shade kernels; render its views one by one");
        return GNXR_ERR_UNSUPPORTED;
    }
    pl.area_only = pl.area_env_only = true;
    for (const gnxr_light &l : cs.desc_lights) {
        if (l.type != GNXR_LIGHT_AREA_TRI) pl.area_only = false;
        if (l.type != GNXR_LIGHT_AREA_TRI && l.type != GNXR_LIGHT_INFINITE) pl.area_env_only = false;
    }
    // escaped continuation rays of a scene with infinite lights get shade queue 3 to themselves when no image-textured material claims it
    pl.escape_queue = pl.path_int() && !pl.textured_scene && !cs.infinite_lights.empty() && !Knobs::no_escape_queue();
    plan_shade_queues(cs, &pl);
    pl.caller_rays = src != nullptr;
    pl.n_views = views ? views->n_views : 0;
    pl.local_rows = count_local_rows(&p);
    pl.npix = views ? views->n_views * p.width * p.height : pl.local_rows * p.width;
    pl.pixel_list = pix != nullptr;
    pl.unit = (src || pix) ? 1 : pl.npix;
    pl.unit_begin = (src || pix) ? 0 : p.spp_begin;
    pl.unit_end = src ? src->n : p.spp_end;
    // the largest round: the one with the most samples, with no pixel stopped yet (run_adaptive rewrites unit_end for every round)
    if (pix) {
        int most = 0;
        for (int n0 = 0; n0 < p.spp;) { const int ns = adaptive_round_samples(pix->ap, p.spp, n0); most = std::max(most, ns); n0 += ns; }
        pl.unit_end = (long long)pl.npix * most;
    }
    pl.spill_entries = std::max(cs.stack4_need + 1, cs.bvh_max_depth + 2);
    pl.k = pl.in_flight = 0;
    pl.half = pl.cap = pl.nrec = 0;
    return GNXR_OK;
}

// Pass sizes: k units per (sub-)pass, in_flight sub-passes alive at once, cap path slots -- or the refusal of a pass that overflows the
// 32-bit work indices.  slots_held: path slots this handle already owns; free_b: free device memory (have_mem: the query succeeded).
int RenderPlan::size_passes(size_t slots_held, bool have_mem, size_t free_b) {
    const long long n_units = unit_end - unit_begin;
    if (pixel_list && p.samples_per_pass <= 0) {
        // Rounds of pixel lists, auto: plan the render these parameters describe (a unit = one sample of every pixel) and live in its
        // slots -- what gnxr_render_reserve allocates for that render then holds every round.  A round that fits them is ONE sub-pass:
        // a round ends with a drain whatever its cut, and every staggered start only adds loop turns to it (measured: DESIGN.md,
        // "Adaptive sampling").  A larger round (min_spp near spp) takes the render's own sub-passes.
        RenderPlan rp = *this;
        rp.pixel_list = false; rp.unit = npix; rp.unit_begin = 0; rp.unit_end = p.spp;
        if (int rc = rp.size_passes(slots_held, have_mem, free_b)) return rc;
        const bool fits = n_units <= (long long)rp.cap;
        k = fits ? (int)n_units : (int)rp.half;
        in_flight = fits ? 1 : (int)std::min<long long>(rp.in_flight, (n_units + k - 1) / k);
        half = (size_t)k; cap = (size_t)in_flight * half; nrec = rp.nrec;   // (cap <= rp.cap: the render's index checks cover it)
        return GNXR_OK;
    }
    k = p.samples_per_pass;
    if (k <= 0) {
        // auto.  PathIntegrator: sub-passes of ~64 M paths, four of them in flight (below) -- launches stay thick because they mix the
        // bounces of different sub-passes.  Measured at 1080p on cfg 3 (1024 spp per call, profiles/README.md round 3): 4 x 32 spp
        // (59 GB of state) renders as fast as round 2's two 128-spp passes (118 GB); 4 x 16 spp (29.5 GB) costs 2 % -- every launch of
        // the persistent traversal kernel pays a ramp and a drain of ~0.3 ms, and the number of launches grows as the resident state shrinks.  VolPath / Whitted / DirectLighting render one pass at a
        // time: big passes keep their thin late rounds from under-filling the GPU, so take up to a quarter of the free HBM for path state
        // (~230 B per path), at most 256 M paths; Whitted / DirectLighting keep max_depth frames and n_records NEE records per path
        long long target = 32ll << 20;
        if (have_mem) target = std::max<long long>(target, std::min<long long>(256ll << 20, (long long)(free_b / 4 / 230)));
        if (volpath) target = std::min<long long>(target, 64ll << 20);   // + 8 float4 of VolPath state per path
        if (whitted) target = (4ll << 20) / std::max(1, n_records / 4);
        if (path_int()) target = kSubPassPaths;
        k = (int)std::max<long long>(1, std::min<long long>(n_units, target / unit));
    }
    k = (int)std::min<long long>(k, n_units);
    // PathIntegrator: up to kMaxRegions sub-passes in flight at once, each in its own region of the state arrays (run_path_loop).
    // passes_in_flight = 0 picks 4, fewer when the call has fewer sub-passes or the state would not fit the 32-bit work indices
    // or ~45 % of the free HBM (~230 B per path slot beyond what this handle already holds).
    half = (size_t)unit * k;
    in_flight = 1;
    if (path_int() && Knobs::pipeline()) {
        const int n_subs = (int)std::min<long long>(kMaxRegions, (n_units + k - 1) / k);
        in_flight = p.passes_in_flight > 0 ? p.passes_in_flight : (Knobs::regions() > 0 ? Knobs::regions() : 4);
        in_flight = std::max(1, std::min(std::min(in_flight, kMaxRegions), n_subs));
        // pixel lists with samples_per_pass = paths per sub-pass: never more slots than one pass of the render that takes the number as
        // samples per pixel (gnxr_render_reserve with the same parameters)
        if (pixel_list && p.samples_per_pass > 0) in_flight = (int)std::max<long long>(1, std::min<long long>(in_flight, (long long)npix * std::min(p.samples_per_pass, p.spp) / k));
        for (; in_flight > 1; --in_flight) {
            const unsigned long long want = (unsigned long long)in_flight * half, held = (unsigned long long)slots_held;
            const bool idx_ok = want < (1ull << 31) && want * 3ull < (1ull << 32);
            bool mem_ok = true;
            if (want > held && have_mem) mem_ok = (want - held) * kSlotBytesEstimate < (unsigned long long)(kStateFreeFraction * (double)free_b);
            // (and never beyond ~150 GB of path state: a 177 GB configuration -- 6 x 64 spp at 1080p -- rendered three times SLOWER than the
            // 118 GB one on the 288 GB card, profiles/r03_shard_efficiency.log)
            if (want * kSlotBytesEstimate > kStateCapBytes) mem_ok = false;
            if (idx_ok && mem_ok) break;
        }
    }
    cap = (size_t)in_flight * half;
    nrec = whitted ? (size_t)std::max(1, n_records) : 1;   // Whitted / DirectLighting keep one NEE record per light sample of a vertex
    // k_trace's work cursor is 32-bit unsigned: continuation rays + two NEE items per record; record slots are `record * cap + path`
    const unsigned long long recs = nrec;
    if (cap >= (1ull << 31) || (unsigned long long)cap * recs >= (1ull << 31) || (unsigned long long)cap * (1ull + 2ull * recs) >= (1ull << 32)) {
        set_error("pass too large: %zu paths x %llu NEE records per vertex overflow the 32-bit work indices; lower samples_per_pass", cap, recs);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

// ---- the per-render state of a handle (RenderState, api_scene.hip.h) ----
// Grows every array to what `pl` needs; arrays only ever grow.
int RenderState::reserve(const RenderPlan &pl) {
    const size_t cap = pl.cap, nrec = pl.nrec;
    int rc;
#define AL(f) if ((rc = f.alloc(cap)) != GNXR_OK) return rc;
    for (int i = 0; i < kRecGroups; ++i) {
        const size_t per_slot = i < 2 ? 1 : (i < 4 ? nrec : (pl.direct ? nrec : 1));
        if ((rc = rec[i].alloc(cap * per_slot * kRS)) != GNXR_OK) return rc;
    }
    if ((rc = mis_Y.alloc(cap * (pl.direct ? nrec : 1))) != GNXR_OK) return rc;
    AL(L) AL(hit) AL(queue_a) AL(queue_b) AL(queue_nee) AL(queue_c0) AL(queue_c1) AL(queue_c2) AL(queue_c3) AL(pflags) AL(pclass) AL(nee_vis)
    if (pl.whitted) {
        const size_t nl = (size_t)std::max(1, pl.n_records), md = (size_t)std::max(1, pl.p.max_depth);
        if ((rc = wh_rec.alloc(cap * nl)) ||
            (rc = wh_o.alloc(cap * md)) || (rc = wh_d.alloc(cap * md)) || (rc = wh_L.alloc(cap * md)) || (rc = wh_w.alloc(cap * md)) ||
            (rc = wh_pdf.alloc(cap * md)) || (rc = vol_vs.alloc(cap)))
            return rc;
        if (pl.textured_scene && ((rc = wh_rxo.alloc(cap * (md + 1))) || (rc = wh_rxd.alloc(cap * (md + 1))) || (rc = wh_ryo.alloc(cap * (md + 1))) || (rc = wh_ryd.alloc(cap * (md + 1)))))
            return rc;
    }
    if (pl.volpath) {
        AL(vol_n1) AL(vol_f) AL(vol_Li) AL(vol_Tr) AL(vol_Ld) AL(vol_mres) AL(vol_vs) AL(vol_state)
        AL(vol_Lout) AL(vol_alt_state) AL(vol_orig) AL(vol_alt_orig) AL(vol_newslot)
        for (int i = 0; i < kVolPackF4; ++i) AL(vol_alt[i])
        for (int i = 0; i < kRecGroups; ++i) if ((rc = vol_alt_rec[i].alloc(cap * kRS)) != GNXR_OK) return rc;
    }
#undef AL
    // global part of k_trace's traversal stacks (the deepest walk either BVH layout can need), sized for a full grid
    if ((rc = trace_spill.alloc((size_t)g_num_cus * g_trace_blocks_per_cu * kBlock * (size_t)pl.spill_entries)) != GNXR_OK) return rc;
    if (!pl.caller_rays && (rc = accum.alloc(pl.npix)) != GNXR_OK) return rc;
    // (pixel lists: the compaction that lists the next round's pixels runs over the image)
    const size_t max_tiles = (std::max(cap, pl.pixel_list ? (size_t)pl.npix : (size_t)0) + kCompactTile - 1) / kCompactTile;
    if (tile_desc.n < kCompactMaxOut * max_tiles || !tile_desc.p) {   // fresh memory: every descriptor "not ready" (tag 0 belongs to no compaction)
        if ((rc = tile_desc.alloc(kCompactMaxOut * max_tiles)) != GNXR_OK) return rc;
        HIP_TRY(hipMemset(tile_desc.p, 0, tile_desc.n * sizeof(unsigned long long)));
        HIP_TRY(hipDeviceSynchronize());   // the render's stream may not wait for the null stream: the clear is complete before any compaction is queued
        compact_seq = 0;
    }
    if ((rc = compact_ticket.alloc(2)) != GNXR_OK) return rc;
    if (pl.n_views > 0 && (rc = view_cams.alloc((size_t)pl.n_views)) != GNXR_OK) return rc;
    return GNXR_OK;
}

// gnxr_stats::state_bytes: what a render keeps resident per path slot -- the float4 / uint2 / int state arrays, the queues and the
// per-path bytes.  This is the stats' own count; it is NOT the 238 B estimate (kSlotBytesEstimate) that the in-flight rule plans with.
unsigned long long RenderState::state_bytes(const RenderPlan &pl) {
    const unsigned long long per_slot = (2ull * kRecGroups + 2) * sizeof(float4) + 8ull * sizeof(int) + 2 + sizeof(unsigned int);   // five record groups + mis_Y + L, hit + seven queues, pflags + pclass, nee_vis
    const unsigned long long tiles = ((unsigned long long)pl.cap + kCompactTile - 1) / kCompactTile;   // + the compaction's tile descriptors
    return (unsigned long long)pl.cap * per_slot + tiles * kCompactMaxOut * sizeof(unsigned long long) +
           (pl.volpath ? (unsigned long long)pl.cap * (6ull * sizeof(float4) + sizeof(int4) + 1) : 0ull);
}

PathArrays RenderState::path_arrays() {
    PathArrays pa;
    float4 *rec_primary[kRecGroups];
    record_ptrs(rec, rec_primary);
    pa.bind_records(rec_primary);
    pa.mis_Y = mis_Y.p;
    pa.L = L.p; pa.hit = hit.p; pa.pflags = pflags.p; pa.pclass = pclass.p; pa.nee_vis = nee_vis.p;
    return pa;
}
VolArrays RenderState::vol_arrays() {
    VolArrays va;
    float4 *rec_primary[kRecGroups];
    record_ptrs(rec, rec_primary);
    va.bind_records(rec_primary);
    va.mis_Y = mis_Y.p;
    va.vs = vol_vs.p; va.n1 = vol_n1.p; va.f = vol_f.p;
    va.Li = vol_Li.p; va.Tr = vol_Tr.p; va.Ld = vol_Ld.p; va.mres = vol_mres.p; va.state = vol_state.p;
    va.orig = vol_orig.p; va.Lout = vol_Lout.p;
    return va;
}
WhittedArrays RenderState::whitted_arrays(const RenderPlan &pl, int n_lights) {
    WhittedArrays wa;
    wa.ws = vol_vs.p; wa.fr_o = wh_o.p; wa.fr_d = wh_d.p; wa.fr_L = wh_L.p; wa.fr_w = wh_w.p; wa.fr_pdf = wh_pdf.p;
    wa.fr_rxo = wh_rxo.p; wa.fr_rxd = wh_rxd.p; wa.fr_ryo = wh_ryo.p; wa.fr_ryd = wh_ryd.p;
    wa.cap = (int)pl.cap; wa.n_lights = n_lights; wa.n_records = pl.n_records;
    // DirectLightingIntegrator::Preprocess requests maxDepth x lights x 2 2D arrays (DirectLightingIntegrator.cpp:19-25)
    wa.start_dim = pl.wmode == WM_DIRECT_ALL ? 5 + 2 * (pl.p.max_depth * n_lights * 2) : 5;
    return wa;
}
// VolPath packing (k_vol_pack, vol_kernel.hip.h): the two sets of the per-path arrays that carry state across rounds
VolPackSet RenderState::pack_set(bool alt) {
    VolPackSet ps;
    if (!alt) {
        float4 *a[kVolPackF4] = {L.p, reinterpret_cast<float4 *>(vol_vs.p), vol_n1.p, vol_f.p, vol_Li.p, vol_Tr.p, vol_Ld.p, mis_Y.p, vol_mres.p};
        for (int i = 0; i < kVolPackF4; ++i) ps.f4[i] = a[i];
        record_ptrs(rec, ps.rec);
        ps.state = vol_state.p; ps.orig = vol_orig.p;
    } else {
        for (int i = 0; i < kVolPackF4; ++i) ps.f4[i] = vol_alt[i].p;
        record_ptrs(vol_alt_rec, ps.rec);
        ps.state = vol_alt_state.p; ps.orig = vol_alt_orig.p;
    }
    return ps;
}

// ---- one render in progress ----
// What the stages of a render share: the handle, the stream, the plan, the kernels' argument structs and the host-side counters.
struct RenderRun {
    gnxr_scene *s;
    RenderState &st;
    hipStream_t stream;
    const RenderPlan &pl;       // (a PixelListSource's rounds: run_adaptive sets unit_begin / unit_end of this plan before each run of the loops)
    const RaySource *src;
    const ViewSource *views;
    const PixelListSource *pix;
    const FilmSource *film = nullptr;   // set by render_one after construction
    float4 *film_accum = nullptr;
    DScene sc;
    DRender r;
    PathArrays pa;
    VolArrays va;
    WhittedArrays wa;
    DMediaTables mt;
    Counters *dctr;
    KernelTimer timer;
    // counting: bit 1 = on the reference's binary tree, bit 2 = on the timed (4-wide) walk + the medium kernel's tracking steps
    const bool timing = (g_profiling & 1) != 0, count_wide = (g_profiling & 4) != 0, counting = (g_profiling & 2) != 0 && !count_wide;
    bool spheres;
    // shade_stage, where the lights are all area lights: 0 = k_shade<LM, LT_AREA>, 1 = SM_DIR_FIRST, 2 = SM_DEFER; the list's drain threshold
    const int mis_mode = Knobs::no_mis_defer() ? 0 : Knobs::mis_defer_step(), mis_drain_at = Knobs::mis_defer_drain_at();
    bool list_media = false;   // VolPath with caller rays (each names a medium) or views in different media: raygen marks the slots that start inside one
    int n_lights, n_scene_media;
    unsigned long long rays_closest = 0, rays_any = 0, rays_mis = 0, media_segments = 0;
    unsigned long long new_paths = 0;   // PathIntegrator: camera rays started (their count is known to the host; the other rays are counted on the device)
    unsigned int launches = 0, passes = 0, loop_iterations = 0;

    RenderRun(gnxr_scene *scene, hipStream_t stream_, const RenderPlan &plan, const RaySource *src_, const ViewSource *views_, const PixelListSource *pix_, const DScene &sc_,
              const DRender &r_)
        : s(scene), st(scene->st), stream(stream_), pl(plan), src(src_), views(views_), pix(pix_), sc(sc_), r(r_), pa(st.path_arrays()), va(st.vol_arrays()),
          wa(st.whitted_arrays(plan, (int)scene->cs.desc_lights.size())), mt(scene->media_tables()), dctr(scene->counters.p), spheres(scene->cs.n_spheres > 0),
          n_lights((int)scene->cs.desc_lights.size()), n_scene_media((int)scene->cs.media.size()) {}

    void launch_trace(TraceWork w, int n_sh, int n_mis, bool count_rays = true);
    void compact(int mode, const int *qin, int nin, const unsigned char *keys, int nout, int nscatter, unsigned int *totals, int *o0, int *o1, int *o2, int *o3 = nullptr, int split = 0,
                 const unsigned *n_dev = nullptr, unsigned kind_queue = 0x01010101u);   // kind_queue: HITCLASS only (RenderPlan::kind_queue)
    int shade_stage(const int *q_in, int n, int *q_out, const unsigned *n_dev);
    void raygen(const PathArrays &at, long long u0, int kk, unsigned char *medium_keys);
    void resolve(const PathArrays &at, long long u0, int kk);
    void bind_set(const VolPackSet &ps);
};

// One launch of the traversal kernel over the closest-hit rays and NEE items of `w`.
// (device-driven loop: w.n_closest / w.n_nee are upper bounds that size the launch, the kernel reads the counts through
// w.n_closest_dev / w.n_nee_dev, and the rays are counted on the device: count_rays = false)
void RenderRun::launch_trace(TraceWork w, int n_sh, int n_mis, bool count_rays) {
    long long total = (long long)w.n_closest + w.n_nee;   // one work item per continuation ray and per NEE vertex (TraceWork)
    if (total <= 0) return;
    w.order = nullptr;
    // (binning the rays of a launch by kind / octant / origin cell with a radix sort was measured in round 2 and lost -- 57.6 - 62.0 ms against
    // 51.7 ms per pass without counting the sort: slot order is already coherent in origin and sorting breaks the coalescing of the state
    // reads; the switch and its library sort are gone, `order` stays in TraceWork for callers that bring their own permutation)
    (void)hipMemsetAsync(&dctr->cursor, 0, sizeof(unsigned int), stream);
    const bool wide = s->wide_ok && !counting;
    const TraceLaunch tl = trace_launch(s, wide, spheres, total);
    if (timing) timer.begin(0, stream);
    // rays per atomic: at most kTraceChunk; the kernel shrinks the chunk for thin launches so that every wave gets one (trace_chunk())
    const int chunk = Knobs::trace_chunk();
#define GX_TRACE(C, W, S) hipLaunchKernelGGL((k_trace<C, W, S>), dim3(tl.blocks), dim3(kBlock), tl.lds, stream, sc, pa, w, &dctr->cursor, dctr, tl.lds_entries, st.trace_spill.p, chunk)
#define GX_TRACE4(C, S, P) hipLaunchKernelGGL((k_trace4<C, S, P>), dim3(tl.blocks), dim3(kBlock), tl.lds, stream, sc, pa, w, &dctr->cursor, dctr, tl.lds_entries, st.trace_spill.p, chunk, tl.n_top, tl.hot_bytes)
#define GX_TRACE4_CS(C, S) do { if (tl.spill_needed) GX_TRACE4(C, S, true); else GX_TRACE4(C, S, false); } while (0)
    if (wide) {   // the 4-wide walk (trace4_kernel.hip.h); count_wide: its counting variant
        if (spheres) { if (count_wide) GX_TRACE4_CS(true, true); else GX_TRACE4_CS(false, true); }
        else { if (count_wide) GX_TRACE4_CS(true, false); else GX_TRACE4_CS(false, false); }
    } else {      // the reference's binary tree: counting runs on BVHAccel's own walk, and scenes the 4-wide encoding cannot hold
        const bool cnt = counting || count_wide;
        if (spheres) { if (cnt) GX_TRACE(true, false, true); else GX_TRACE(false, false, true); }
        else { if (cnt) GX_TRACE(true, false, false); else GX_TRACE(false, false, false); }
    }
#undef GX_TRACE4_CS
#undef GX_TRACE4
#undef GX_TRACE
    if (timing) timer.end(stream);
    if (count_rays) {
        rays_closest += (unsigned long long)w.n_closest + (unsigned long long)n_mis;
        rays_any += (unsigned long long)n_sh;
        rays_mis += (unsigned long long)n_mis;
    }
    ++launches;
}

// stream compaction (compact_kernel.hip.h): one launch, one pass over the queue
// (n_dev: the item count lives on the device; `nin` then bounds it and sizes the launch)
void RenderRun::compact(int mode, const int *qin, int nin, const unsigned char *keys, int nout, int nscatter, unsigned int *totals, int *o0, int *o1, int *o2, int *o3, int split,
                        const unsigned *n_dev, unsigned kind_queue) {
    const int tiles = (nin + kCompactTile - 1) / kCompactTile;
    const int g = std::max(1, std::min(tiles, g_num_cus * kCompactBlocksPerCu));
    // every compaction of the handle has a sequence number of its own; when the 30 bits of a descriptor's tag run out, start over on cleared descriptors
    if (st.compact_seq >= (1u << 30) - 1u) {
        (void)hipMemsetAsync(st.tile_desc.p, 0, st.tile_desc.n * sizeof(unsigned long long), stream);
        st.compact_seq = 0;
    }
    const unsigned seq = ++st.compact_seq;
    const CompactScratch cs{st.tile_desc.p, tiles, st.compact_ticket.p + (seq & 1u), st.compact_ticket.p + ((seq + 1u) & 1u), seq};
    // HITCLASS: the class of the triangle a path hit is looked up from `hit`; `keys` (pclass) holds it for misses and sphere hits
    const bool hitclass = mode == COMPACT_HITCLASS;
    const int *hit = hitclass ? (const int *)st.hit.p : nullptr;
    const unsigned char *cls = hitclass ? (const unsigned char *)s->tri_class.p : nullptr;
#define GX_COMPACT(M, N, NS) hipLaunchKernelGGL((k_compact<M, N, NS>), dim3(g), dim3(kCompactBlock), 0, stream, qin, nin, keys, cs, totals, o0, o1, o2, o3, hit, cls, kind_queue, split, n_dev, dctr)
    if (mode == COMPACT_FLAGS) {
        // a fifth count: the paths that continue AND live in the lower half of the state arrays (slot < split)
        if (nout == 5) { if (nscatter == 3) GX_COMPACT(COMPACT_FLAGS, 5, 3); else GX_COMPACT(COMPACT_FLAGS, 5, 2); }
        else { if (nscatter == 3) GX_COMPACT(COMPACT_FLAGS, 4, 3); else GX_COMPACT(COMPACT_FLAGS, 4, 2); }
    } else if (hitclass) { if (nout == 4) GX_COMPACT(COMPACT_HITCLASS, 4, 4); else GX_COMPACT(COMPACT_HITCLASS, 3, 3); }
    else if (nout == 4) GX_COMPACT(COMPACT_CLASS, 4, 4);
    else GX_COMPACT(COMPACT_CLASS, 3, 3);
#undef GX_COMPACT
    launches += 1;
}
// a look-back of k_compact gave up (Counters::compact_stall): the queues of this render are incomplete
static int compact_stalled(const Counters &c) {
    if (!c.compact_stall) return GNXR_OK;
    set_error("queue compaction: a tile waited for its predecessors beyond the poll limit (k_compact); the render was abandoned");
    return GNXR_ERR_RUNTIME;
}

constexpr size_t kShadeLdsBudget = 52 * 1024;   // LDS of a k_shade block that runs three to a CU (160 KB; the rest is allocation slack)

// PathIntegrator::Li at the vertices the last trace found: class binning, one k_shade per class, queue compaction.  What they spawned is
// counted on the device.  `n` bounds the number of queued paths (it sizes the launches); the count itself is read through n_dev.
// Returns the status of the fork / join of the class streams; the launches themselves are checked once per loop turn (run_path_loop).
int RenderRun::shade_stage(const int *q_in, int n, int *q_out, const unsigned *n_dev) {
    if (timing) timer.begin(2, stream);
    const int *qk = pl.queue_kernel;
    // bin the paths by the shade queue of the material they hit (plan_shade_queues; pclass written by k_trace for misses and sphere hits)
    const int n_classes = qk[3] != SHADE_Q_NONE ? 4 : 3;   // image-textured materials, escaped rays or a material kind have shade queue 3
    compact(COMPACT_HITCLASS, q_in, n, st.pclass.p, n_classes, n_classes, &dctr->q_class[0], st.queue_c0.p, st.queue_c1.p, st.queue_c2.p, st.queue_c3.p, 0, n_dev, pl.kind_queue);
    int *qc[4] = {st.queue_c0.p, st.queue_c1.p, st.queue_c2.p, st.queue_c3.p};
    // 32 blocks per CU: of a k_shade grid only 2 - 3 blocks per CU are resident at a time (168 - 256 registers), and many short blocks
    // balance the end of the launch better than few long ones (8 / 16 / 32 / 64 / 128 / 1024 per CU: shade 171.4 / 167.1 / 165.7 / 165.4 /
    // 168.4 / 176.4 ms on cfg 3, profiles/r03_ab_shade_grid_cfg3.log; each block refills its LDS tables, which is what the large grids pay)
    dim3 g(grid_for(n, Knobs::shade_blocks_per_cu())), b(kBlock);
    // the Halton tables of the first dimensions go to LDS (device_sampler.h LdsSampler): 64 dimensions (the camera sample + 6 path vertices:
    // 18.8 KB per block; deeper vertices read global memory).  A/B on cfg 3: shade -3 % at 64 / 88 dimensions, +4 % at 112 (occupancy)
    const int sdims = std::min<int>(Knobs::shade_lds_dims(), (int)s->cs.prime_sums.size() - 1);
    const int snperm = sdims > 0 ? s->cs.prime_sums[sdims] : 0;
    // + the scene's material and light tables when they are small (k_shade: dependent gathers along the BSDF code become LDS reads)
    const bool shade_lds_tabs = Knobs::shade_lds_tables();
    const int lmats = (shade_lds_tabs && s->cs.materials.size() <= 12) ? (int)s->cs.materials.size() : 0;
    const int llights = (shade_lds_tabs && n_lights > 0 && n_lights <= 16) ? n_lights : 0;
    const size_t slds = (sdims > 0 ? ((((size_t)snperm * 2 + 15) & ~(size_t)15) + (size_t)sdims * 32) : 0) + (size_t)lmats * sizeof(DMaterial) + (size_t)llights * sizeof(DLight);
    // the class kernels work on disjoint paths: with three or more of them (cfg 4: diffuse, glossy, Disney, escaped rays) classes 1 - 3 run on
    // two auxiliary streams beside class 0, so that the blocks of one fill the thinning end of another (fork / join with events): cfg 4 shade
    // -4 %; with two kernels of similar size (cfg 3 with one glossy queue) the same costs 1.5 %, so they stay in line
    // (profiles/r03_ab_shade_streams_*.log; GNXR_SHADE_STREAMS = 0 / 1 forces either).  cfg 3 with a queue per material kind has three: forked
    // 5170 against 5151 Mrays/s in line (profiles/README.md, "One shade queue per kind of glossy material"), so the rule covers it as it stands
    const int shade_streams = Knobs::shade_streams();
    int n_class_kernels = 0;
    for (int q = 0; q < 4; ++q) n_class_kernels += qk[q] != SHADE_Q_NONE ? 1 : 0;
    const bool fork = (shade_streams < 0 ? n_class_kernels >= 3 : (shade_streams != 0 && n_class_kernels >= 2)) && s->aux_stream[0] && s->aux_stream[1];
    hipStream_t cst[4] = {stream, stream, stream, stream};
    if (fork) {
        HIP_TRY(hipEventRecord(s->ev_fork, stream));
        HIP_TRY(hipStreamWaitEvent(s->aux_stream[0], s->ev_fork, 0));
        HIP_TRY(hipStreamWaitEvent(s->aux_stream[1], s->ev_fork, 0));
        cst[1] = s->aux_stream[0]; cst[2] = s->aux_stream[1]; cst[3] = s->aux_stream[1];
    }
    const bool area_only = pl.area_only, area_env_only = pl.area_env_only;
#define GX_SHADE_KA(K, C, LDS, LL) hipLaunchKernelGGL(K, g, b, LDS, cst[C], sc, r, pa, (const int *)qc[C], (const unsigned int *)&dctr->q_class[C], sdims, snperm, lmats, LL)
#define GX_SHADE_K(K, C) GX_SHADE_KA(K, C, slds, llights)
#define GX_SHADE(LMV, LTV, C) do { if (spheres) GX_SHADE_K((k_shade<LMV, LTV, true>), C); else GX_SHADE_K((k_shade<LMV, LTV, false>), C); } while (0)
    // area lights only: the kernels with the MIS half of EstimateDirect reordered (mis_step, above; 0: k_shade<LM, LT_AREA>, the same bits)
#define GX_SHADE_AREA_S(LMV, SPHV, C) do { \
        if (mis_step == 2) GX_SHADE_KA((k_shade<LMV, LT_AREA | SM_DEFER, SPHV>), C, slds_mis, llights_mis); \
        else if (mis_step == 1) GX_SHADE_K((k_shade<LMV, LT_AREA | SM_DIR_FIRST, SPHV>), C); \
        else GX_SHADE_K((k_shade<LMV, LT_AREA, SPHV>), C); } while (0)
#define GX_SHADE_AREA(LMV, C) do { if (spheres) GX_SHADE_AREA_S(LMV, true, C); else GX_SHADE_AREA_S(LMV, false, C); } while (0)
#define GX_SHADE_TEX(LTV) do { if (spheres) GX_SHADE_K((k_shade<LM_ALL, LTV, true, true>), 3); else GX_SHADE_K((k_shade<LM_ALL, LTV, false, true>), 3); } while (0)
    // BASELINE config 4's light set (area lights + one InfiniteAreaLight) has kernels without the delta-light and sky-box code
    const int light_set = area_only ? 0 : ((area_env_only && !spheres && !(pl.class_mask & 8)) ? 1 : 2);
    // Area lights alone: the MIS half of EstimateDirect direction first (k_shade's SM_DIR_FIRST), and its rare vertices on a list per wave in
    // LDS (SM_DEFER) where the lists fit beside the tables: three blocks per CU share 160 KB, so a block has kShadeLdsBudget.  Where they
    // do not (more than a handful of materials in LDS) the plan falls back to SM_DIR_FIRST.
    int mis_step = light_set == 0 ? mis_mode : 0;
    const size_t slds_mis = slds + (size_t)(kBlock / 64) * ((size_t)kMisEntryWords * kMisCap + 1) * sizeof(int);
    const int llights_mis = llights | (std::min(mis_drain_at, kMisCap) << 8);
    if (mis_step == 2 && slds_mis > kShadeLdsBudget) mis_step = 1;
#define GX_SHADE_LM(LMV, C) do { \
        if (light_set == 0) GX_SHADE_AREA(LMV, C); \
        else if (light_set == 1) GX_SHADE_K((k_shade<LMV, LT_AREA | LT_ENV, false>), C); \
        else GX_SHADE(LMV, LT_ALL, C); } while (0)
    // (the narrow kernels exist without spheres only: plan_shade_queues gives a scene with spheres no queue per kind)
#define GX_SHADE_NARROW(LMV, C) do { \
        if (light_set == 0) GX_SHADE_AREA_S(LMV, false, C); \
        else if (light_set == 1) GX_SHADE_K((k_shade<LMV, LT_AREA | LT_ENV, false>), C); \
        else GX_SHADE_K((k_shade<LMV, LT_ALL, false>), C); } while (0)
    for (int q = 0; q < 4; ++q) {
        switch (qk[q]) {
        case SHADE_Q_DIFFUSE: GX_SHADE_LM(LM_DIFFUSE, q); break;
        case SHADE_Q_GLOSSY: GX_SHADE_LM(LM_GLOSSY, q); break;
        case SHADE_Q_CONDUCTOR: GX_SHADE_NARROW(LM_CONDUCTOR, q); break;
        case SHADE_Q_ROUGH_DIELECTRIC: GX_SHADE_NARROW(LM_ROUGH_DIELECTRIC, q); break;
        case SHADE_Q_ALL: GX_SHADE_LM(LM_ALL, q); break;
        case SHADE_Q_TEX: if (light_set == 0) GX_SHADE_TEX(LT_AREA); else GX_SHADE_TEX(LT_ALL); break;
        case SHADE_Q_ESCAPE:
            if (area_env_only) hipLaunchKernelGGL((k_shade_escape<LT_AREA | LT_ENV>), g, b, 0, cst[q], sc, pa, (const int *)qc[q], (const unsigned int *)&dctr->q_class[q]);
            else hipLaunchKernelGGL((k_shade_escape<LT_ALL>), g, b, 0, cst[q], sc, pa, (const int *)qc[q], (const unsigned int *)&dctr->q_class[q]);
            break;
        default: continue;
        }
        ++launches;
    }
#undef GX_SHADE_NARROW
#undef GX_SHADE_LM
#undef GX_SHADE_TEX
#undef GX_SHADE_AREA
#undef GX_SHADE_AREA_S
#undef GX_SHADE
#undef GX_SHADE_K
#undef GX_SHADE_KA
    if (fork) {
        HIP_TRY(hipEventRecord(s->ev_join[0], s->aux_stream[0]));
        HIP_TRY(hipEventRecord(s->ev_join[1], s->aux_stream[1]));
        HIP_TRY(hipStreamWaitEvent(stream, s->ev_join[0], 0));
        HIP_TRY(hipStreamWaitEvent(stream, s->ev_join[1], 0));
    }
    // next-vertex queue + NEE queue from the per-path flags; totals also count shadow and MIS rays
    compact(COMPACT_FLAGS, q_in, n, st.pflags.p, 4, 2, &dctr->q_next, q_out, st.queue_nee.p, nullptr, nullptr, 0, n_dev);
    if (timing) timer.end(stream);
    return GNXR_OK;
}

// The two image stages of the loops, or their caller-ray counterparts (RaySource, li_kernel.hip.h): start the paths of units
// [u0, u0 + kk) in the slots of `at`, and hand the radiance of a finished (sub-)pass -- L by slot -- to the image or to the caller.
void RenderRun::raygen(const PathArrays &at, long long u0, int kk, unsigned char *medium_keys) {
    const int n_new = (int)(pl.unit * kk);
    if (pix) hipLaunchKernelGGL(k_raygen_pixels, dim3(grid_for(n_new)), dim3(kBlock), 0, stream, sc, r, at, pix->round, n_new, u0);
    else if (views) hipLaunchKernelGGL(k_raygen_views, dim3(grid_for(n_new)), dim3(kBlock), 0, stream, sc, r, (const DCamera *)st.view_cams.p, at, n_new, (int)u0, medium_keys);
    else if (!src) hipLaunchKernelGGL(k_raygen, dim3(grid_for(n_new)), dim3(kBlock), 0, stream, sc, r, at, n_new, (int)u0);
    else hipLaunchKernelGGL(k_raygen_rays, dim3(grid_for(n_new)), dim3(kBlock), 0, stream, sc, r, at, reinterpret_cast<const float4 *>(src->rays + u0),
                            reinterpret_cast<const int4 *>(src->samples + u0), n_new, n_scene_media, medium_keys, dctr, u0);
}
void RenderRun::resolve(const PathArrays &at, long long u0, int kk) {
    if (pix) hipLaunchKernelGGL(k_adaptive_accum, dim3(grid_for(pix->round.n_active)), dim3(kBlock), 0, stream, (const float4 *)at.L, pix->round, kk, u0, st.accum.p, st.ad_A.p);
    else if (film) {   // layer j of the sub-pass: sample u0 + j of every pixel (slot = j * npix + pixel, as k_resolve reads it)
        const FilmImage im = film_image(r.W, r.H, std::max(1, pl.n_views));
        hipLaunchKernelGGL(k_film_add<true>, dim3(film_grid(im)), dim3(kBlock), 0, stream, im, film->f, film->tab, (const float4 *)at.L, (const float2 *)nullptr, sc.st, (int)u0, kk, film_accum);
    }
    else if (!src) hipLaunchKernelGGL(k_resolve, dim3(grid_for(r.npix)), dim3(kBlock), 0, stream, at, st.accum.p, r.npix, kk);
    else hipLaunchKernelGGL(k_store_li, dim3(grid_for(kk)), dim3(kBlock), 0, stream, (const float4 *)at.L, reinterpret_cast<const int4 *>(src->samples + u0), r,
                            n_scene_media, kk, reinterpret_cast<float4 *>(src->L) + u0);
}
// VolPath packing: point the kernels' views at a set
void RenderRun::bind_set(const VolPackSet &ps) {
    pa.bind_records(ps.rec); va.bind_records(ps.rec);
    pa.L = ps.f4[0]; va.vs = reinterpret_cast<int4 *>(ps.f4[1]); va.n1 = ps.f4[2]; va.f = ps.f4[3]; va.Li = ps.f4[4]; va.Tr = ps.f4[5]; va.Ld = ps.f4[6]; pa.mis_Y = va.mis_Y = ps.f4[7]; va.mres = ps.f4[8];
    va.state = ps.state; va.orig = ps.orig;
}

// ---- the three loops ----
// a launch that failed since the last check (launches report through the runtime's last error, not through a return value)
#define GX_CHECK_LAUNCHES(where)                                                                                    \
    do {                                                                                                            \
        const hipError_t le_ = hipGetLastError();                                                                   \
        if (le_ != hipSuccess) { set_error("HIP runtime error in " where ": %s", hipGetErrorString(le_)); return hip_status(le_); } \
    } while (0)

// PathIntegrator: the device-driven path loop, one vertex of every live path per turn.  The units of a call are cut into sub-passes of
// `k` samples per pixel; up to `in_flight` of them
// are alive at once, each in its own region of the state arrays, staggered in time: a launch then mixes the camera rays and first
// bounces of one sub-pass with the thin late bounces of the others (Russian roulette and escapes leave a few hundred thousand of a
// sub-pass's paths after five bounces), so launches stay thick while the resident state is in_flight x k samples per pixel
// instead of two 128-sample passes.  Queues hold slots of all regions in ascending order; results per path do not depend on who
// shares a launch, and k_resolve runs per sub-pass in sample order, so images are unchanged bit for bit.  Caller rays (RaySource): a
// sub-pass is a chunk of up to k rays, and a chunk that has ended is stored at once (every ray owns its result: no order to keep).
//
// The host never waits for the iteration it enqueues: every queue count stays on the device (kernels read them there; launches are
// sized by upper bounds), and what the host needs for its decisions -- how many paths of each region are left -- it reads from a
// ring of pinned copies that lag the GPU by up to `lag` iterations.  A stale zero is still a zero (a region only refills when the
// host starts a sub-pass in it), and a stale count is an upper bound.  Reference loop: core/Integrator.cpp:256-293.
static int run_path_loop(RenderRun &run) {
    gnxr_scene *s = run.s;
    RenderState &st = run.st;
    const RenderPlan &pl = run.pl;
    hipStream_t stream = run.stream;
    Counters *dctr = run.dctr;
    const size_t half = pl.half;
    struct Sub { long long u0; int kk; };
    std::vector<Sub> subs;
    for (long long u0 = pl.unit_begin; u0 < pl.unit_end; u0 += pl.k) subs.push_back(Sub{u0, (int)std::min<long long>(pl.k, pl.unit_end - u0)});
    const int R = pl.in_flight;
    struct Region { int sub = -1, started = -1; long long paths = 0; } reg[kMaxRegions];
    const int lag = std::max(1, std::min(gnxr_scene::kRing - 2, Knobs::loop_lag() >= 0 ? Knobs::loop_lag() : 2));
    // a sub-pass lives max_depth + 2 iterations (+ the lag until the host sees that it has ended): spread the starts over that time
    const int stagger = Knobs::pipe_cut() >= 0 ? Knobs::pipe_cut() : std::max(1, (pl.p.max_depth + 2 + lag + R - 1) / R);
    int *qbuf[2] = {st.queue_a.p, st.queue_b.p};
    int in_idx = 0;
    const int nee_in_trace = Knobs::no_trace_nee_apply() ? 0 : 1;   // TraceWork::nee_in_trace
    const unsigned *cnt_ptr = &dctr->n_queue;  // where the count of the queue in flight lives on the device (k_loop_tail / k_queue_merge write it)
    size_t next_sub = 0, done_subs = 0;
    int iter = 0, last_start = -(1 << 20), newest_seen = -1;
    int ring_iter[gnxr_scene::kRing];          // iteration whose counters were copied into each ring slot (-1: none)
    for (int &v : ring_iter) v = -1;
    Counters seen;
    memset(&seen, 0, sizeof(seen));
    long long guard = 0;
    while (done_subs < subs.size()) {
        // 1. the newest copy of the counters that has arrived (never the iteration just enqueued, unless the GPU is already through it)
        {
            // at most `lag` iterations ahead of what has been seen: wait for the oldest outstanding copy beyond that
            int oldest_needed = iter - 1 - lag;
            for (int j = newest_seen + 1; j <= oldest_needed; ++j) {
                const int slot = j % gnxr_scene::kRing;
                if (j >= 0 && ring_iter[slot] == j) HIP_TRY(hipEventSynchronize(s->ring_ev[slot]));
            }
            for (int j = iter - 1; j > newest_seen; --j) {
                const int slot = ((j % gnxr_scene::kRing) + gnxr_scene::kRing) % gnxr_scene::kRing;
                if (j < 0 || ring_iter[slot] != j) continue;
                const hipError_t q = hipEventQuery(s->ring_ev[slot]);
                if (q == hipSuccess) { seen = s->h_ring[slot]; newest_seen = j; if (int rc = compact_stalled(seen)) return rc; break; }
                if (q != hipErrorNotReady) { set_error("HIP runtime error in the path loop: hipEventQuery: %s", hipGetErrorString(q)); return hip_status(q); }
                (void)hipGetLastError();   // "not ready" is reported as an error: clear that one, and nothing else
            }
        }
        // 2. sub-passes none of whose paths continues are complete once their last light estimates are added (stream order: the
        //    k_nee_combine of the iteration that produced the zero is already enqueued): colObj += Li in sample order
        //    -- and in sub-pass order: a sub-pass that ends before an earlier one keeps its region until that one is added
        for (bool progress = true; progress;) {
            progress = false;
            for (int rg = 0; rg < R; ++rg) {
                Region &g = reg[rg];
                if (g.sub >= 0 && (run.src || g.sub == (int)done_subs) && newest_seen > g.started && seen.region_alive[rg] == 0) {
                    run.resolve(run.pa.at((size_t)rg * half), subs[g.sub].u0, subs[g.sub].kk);
                    ++run.launches; ++run.passes; ++done_subs;
                    g.sub = -1;
                    progress = true;
                }
            }
        }
        if (done_subs == subs.size()) break;
        // upper bound of the paths queued for this iteration's shade stage
        bool any_active = false;
        long long n_upper = 0;
        for (int rg = 0; rg < R; ++rg) {
            const Region &g = reg[rg];
            if (g.sub < 0) continue;
            any_active = true;
            n_upper += newest_seen > g.started ? std::min<long long>(g.paths, seen.region_alive[rg]) : g.paths;
        }
        // A. shade what the last trace found; survivors go to the buffer that does not hold the input queue
        const int out_idx = 1 - in_idx;
        if (any_active) {
            if (int rc = run.shade_stage(qbuf[in_idx], (int)n_upper, qbuf[out_idx], cnt_ptr)) return rc;
            hipLaunchKernelGGL(k_loop_tail, dim3(1), dim3(64), 0, stream, (const int *)qbuf[out_idx], dctr, R, (int)half, (unsigned)iter);
            ++run.launches;
            const int slot = iter % gnxr_scene::kRing;
            HIP_TRY(hipMemcpyAsync(&s->h_ring[slot], dctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipEventRecord(s->ring_ev[slot], stream));
            ring_iter[slot] = iter;
        }
        // B. start the next sub-pass in a free region
        int trace_idx = out_idx;
        long long n_trace_upper = n_upper;
        int free_rg = -1;
        for (int rg = 0; rg < R && free_rg < 0; ++rg) if (reg[rg].sub < 0) free_rg = rg;
        const bool start = next_sub < subs.size() && free_rg >= 0 && (!any_active || iter - last_start >= stagger);
        if (start) {
            const Sub &nw = subs[next_sub];
            const int n_new = (int)(pl.unit * nw.kk);
            const size_t base = (size_t)free_rg * half;
            run.raygen(run.pa.at(base), nw.u0, nw.kk, nullptr);
            // survivors + every slot of the new sub-pass, ascending: into the buffer the shaded queue came from
            hipLaunchKernelGGL(k_queue_merge, dim3(grid_for(n_upper + n_new)), dim3(kBlock), 0, stream, (const int *)qbuf[out_idx], dctr, any_active ? 0 : 1, free_rg, (int)base, n_new, qbuf[in_idx]);
            run.launches += 2;
            trace_idx = in_idx; n_trace_upper = n_upper + n_new;
            run.new_paths += (unsigned long long)n_new;
            reg[free_rg].sub = (int)next_sub; reg[free_rg].started = iter; reg[free_rg].paths = n_new;
            last_start = iter;
            ++next_sub;
        }
        // C. continuation rays (and new camera rays), shadow and MIS rays of the vertices just shaded; then their light estimates
        if (any_active || start) {
            TraceWork tw{qbuf[trace_idx], (int)n_trace_upper, st.queue_nee.p, any_active ? (int)n_upper : 0, nullptr, reinterpret_cast<unsigned char *>(st.nee_vis.p), cnt_ptr,
                         any_active ? (const unsigned *)&dctr->q_nee : nullptr, nee_in_trace};
            run.launch_trace(tw, 0, 0, false);
            if (any_active) {
                if (run.timing) run.timer.begin(1, stream);
                hipLaunchKernelGGL(k_nee_combine, dim3(grid_for(n_upper)), dim3(kBlock), 0, stream, run.pa, (const int *)st.queue_nee.p, (int)n_upper, reinterpret_cast<const unsigned char *>(st.nee_vis.p),
                                   (const unsigned *)&dctr->q_nee, &dctr->nee_applied_sweep);   // the sweep: every vertex k_trace4 has not added itself
                if (run.timing) run.timer.end(stream);
                ++run.launches;
            }
            in_idx = trace_idx;
        }
        GX_CHECK_LAUNCHES("the path loop");   // this turn's launches; no synchronisation: the host still runs ahead of the GPU
        ++iter; ++run.loop_iterations;
        if (++guard > (1ll << 24)) { set_error("path loop did not terminate"); return GNXR_ERR_INVALID; }
    }
    return GNXR_OK;
}

// Whitted / DirectLighting, one pass: depth-first recursion per path (whitted_kernel.hip.h): the path's ray + the previous vertex's shadow
// rays per round.  The paths of units [u0, u0 + kk) have been started by raygen.
static int run_whitted_pass(RenderRun &run, long long u0, int kk) {
    RenderState &st = run.st;
    const RenderPlan &pl = run.pl;
    hipStream_t stream = run.stream;
    Counters *dctr = run.dctr;
    const DScene &sc = run.sc;
    const DRender &r = run.r;
    const PathArrays &pa = run.pa;
    const WhittedArrays &wa = run.wa;
    const int n_paths = (int)(pl.unit * kk), n_records = pl.n_records;
    const bool textured = pl.textured_scene;
    hipLaunchKernelGGL(k_whitted_init, dim3(grid_for(n_paths)), dim3(kBlock), 0, stream, pa, wa, n_paths);
    ++run.launches;
    if (textured) {
        if (run.views) hipLaunchKernelGGL(k_whitted_init_diff_views, dim3(grid_for(n_paths)), dim3(kBlock), 0, stream, sc, r, (const DCamera *)st.view_cams.p, pa, wa, n_paths);
        else hipLaunchKernelGGL(k_whitted_init_diff, dim3(grid_for(n_paths)), dim3(kBlock), 0, stream, sc, r, pa, wa, n_paths);
        ++run.launches;
    }
    int n = n_paths, n_cl = n_paths, n_shp = 0, guard = 0;
    const int *q_in = nullptr, *q_cl = nullptr;   // paths alive at this vertex / with a closest-hit ray to trace (nullptr == identity), ascending
    int *q_cur = st.queue_a.p, *q_other = st.queue_b.p;
    unsigned long long *d_shadow = &dctr->whitted_shadow;
    while (n > 0) {
        if (n_shp > 0) {
            hipLaunchKernelGGL(k_whitted_expand, dim3(grid_for((long long)n_shp * n_records)), dim3(kBlock), 0, stream, (const int *)st.queue_nee.p, n_shp, n_records, (int)pl.cap, st.wh_rec.p);
            ++run.launches;
        }
        run.launch_trace(TraceWork{q_cl, n_cl, st.wh_rec.p, n_shp * n_records}, 0, 0);
        if (run.timing) run.timer.begin(2, stream);
#define GX_WH2(MODEV, LTV, SPHV)                                                                                                                     \
    do {                                                                                                                                             \
        if (textured) hipLaunchKernelGGL((k_whitted_step<MODEV, LTV, SPHV, true>), dim3(grid_for(n)), dim3(kBlock), 0, stream, sc, r, pa, wa, q_in, n, d_shadow); \
        else hipLaunchKernelGGL((k_whitted_step<MODEV, LTV, SPHV>), dim3(grid_for(n)), dim3(kBlock), 0, stream, sc, r, pa, wa, q_in, n, d_shadow);   \
    } while (0)
#define GX_WH(LTV, SPHV) do { if (pl.wmode == WM_WHITTED) GX_WH2(WM_WHITTED, LTV, SPHV); else if (pl.wmode == WM_DIRECT_ONE) GX_WH2(WM_DIRECT_ONE, LTV, SPHV); else GX_WH2(WM_DIRECT_ALL, LTV, SPHV); } while (0)
        if (pl.area_only) { if (run.spheres) GX_WH(LT_AREA, true); else GX_WH(LT_AREA, false); }
        else { if (run.spheres) GX_WH(LT_ALL, true); else GX_WH(LT_ALL, false); }
#undef GX_WH
#undef GX_WH2
        ++run.launches;
        run.compact(COMPACT_FLAGS, q_in, n, st.pflags.p, 4, 3, &dctr->q_next, q_cur, st.queue_nee.p, st.queue_c0.p);
        if (run.timing) run.timer.end(stream);
        HIP_TRY(hipMemcpyAsync(run.s->h_counters, dctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = compact_stalled(*run.s->h_counters)) return rc;
        n = (int)run.s->h_counters->q_next;
        n_shp = (int)run.s->h_counters->q_nee;
        n_cl = (int)run.s->h_counters->q_shadow;   // count of pflags bit2: paths with a closest-hit ray to trace
        q_cl = st.queue_c0.p;
        q_in = q_cur;
        std::swap(q_cur, q_other);
        if (++guard > (1 << 20)) { set_error("path loop did not terminate"); return GNXR_ERR_INVALID; }
    }
    return GNXR_OK;
}

// VolPath, one pass: one closest-hit ray per live path and round: k_trace -> k_vol_media -> k_vol_step -> compaction (vol_kernel.hip.h).
// The paths of units [u0, u0 + kk) have been started by raygen.
static int run_volpath_pass(RenderRun &run, long long u0, int kk) {
    gnxr_scene *s = run.s;
    RenderState &st = run.st;
    const RenderPlan &pl = run.pl;
    hipStream_t stream = run.stream;
    Counters *dctr = run.dctr;
    const DScene &sc = run.sc;
    const DRender &r = run.r;
    const DMediaTables &mt = run.mt;
    const PathArrays &pa = run.pa;   // (views of the sets bind_set() points them at)
    const VolArrays &va = run.va;
    const int n_paths = (int)(pl.unit * kk), class_mask = pl.class_mask, nL = run.n_lights;
    int n = n_paths, guard = 0;
    const int *q_in = nullptr;            // paths alive at this vertex (nullptr == identity), ascending
    int *q_cur = st.queue_a.p, *q_other = st.queue_b.p;
    hipLaunchKernelGGL(k_vol_init, dim3(grid_for(n_paths)), dim3(kBlock), 0, stream, pa, va, n_paths);
    ++run.launches;
    int n_media = r.cam.medium >= 0 ? n : 0;      // paths whose ray in flight travels inside a medium
    const int *q_media = nullptr;
    if (run.list_media) {   // caller rays: each record names its own medium (views: each view); list the slots raygen marked (pflags bit 1)
        run.compact(COMPACT_FLAGS, nullptr, n, st.pflags.p, 4, 2, &dctr->q_next, q_cur, st.queue_nee.p, nullptr);
        HIP_TRY(hipMemcpyAsync(s->h_counters, dctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = compact_stalled(*s->h_counters)) return rc;
        n_media = (int)s->h_counters->q_nee;
        q_media = st.queue_nee.p;
    }
    // packing (k_vol_pack, vol_kernel.hip.h): the live paths move between the two sets of the per-path arrays (RenderState::pack_set)
    bool in_alt = false;
    long long span = n_paths;     // the live paths lie in slots [0, span)
    run.bind_set(st.pack_set(false));
    while (n > 0) {
        run.launch_trace(TraceWork{q_in, n, nullptr, 0}, 0, 0);
        if (n_media > 0) {
            (void)hipMemsetAsync(&dctr->cursor, 0, sizeof(unsigned int), stream);
            // (4 / 5 / 8 / 16 / 32 blocks per CU: k_vol_media 0.357 s per 3 x 256 spp of cfg 5 each time -- its waves persist; profiles/r03_ab_vol_step_occupancy_cfg5.log)
            int blocks = (int)std::min<long long>((long long)g_num_cus * 8, ((long long)n_media + kBlock - 1) / kBlock);
            const int vm_cap = Knobs::volmedia_step_cap();   // read per launch so that a test can vary it (0: no cap)
            if (run.timing) run.timer.begin(1, stream);
            const long long mwaves = (long long)blocks * (kBlock / 64);
            const int mchunk = (int)std::min<long long>(kMediaChunk, std::max<long long>(64, ((n_media + mwaves - 1) / mwaves + 63) / 64 * 64));
            if (run.count_wide) hipLaunchKernelGGL(k_vol_media<true>, dim3(blocks), dim3(kBlock), (size_t)kVmRecDwords * kVmStride * sizeof(int), stream, sc, mt, pa, va, q_media, n_media, &dctr->cursor, mchunk, dctr, vm_cap);
            else hipLaunchKernelGGL(k_vol_media<false>, dim3(blocks), dim3(kBlock), (size_t)kVmRecDwords * kVmStride * sizeof(int), stream, sc, mt, pa, va, q_media, n_media, &dctr->cursor, mchunk, dctr, vm_cap);
            run.media_segments += (unsigned long long)n_media;
            if (run.timing) run.timer.end(stream);
            ++run.launches;
        }
        if (run.timing) run.timer.begin(2, stream);
        // bin the live paths by state (main ray / shadow-ray segment / scattering-ray segment), one k_vol_step instantiation per bin
        // (32 blocks per CU for the step kernels, as for k_shade: many short blocks balance the end of a launch better; cfg 5 -2 %)
        run.compact(COMPACT_CLASS, q_in, n, va.state, 3, 3, &dctr->q_class[0], st.queue_c0.p, st.queue_c1.p, st.queue_c2.p);
        {
            int *qc[3] = {st.queue_c0.p, st.queue_c1.p, st.queue_c2.p};
            // the scene's material and light tables go to LDS when they are small (as for k_shade)
            const int vmats = s->cs.materials.size() <= 12 ? (int)s->cs.materials.size() : 0, vlights = (nL > 0 && nL <= 16) ? nL : 0;
            const size_t vlds = (size_t)vmats * sizeof(DMaterial) + (size_t)vlights * sizeof(DLight);
#define GX_VS_K(K, ST) hipLaunchKernelGGL(K, dim3(grid_for(n, 32)), dim3(kBlock), vlds, stream, sc, mt, r, pa, va, (const int *)qc[ST], (const unsigned int *)&dctr->q_class[ST], vmats, vlights)
#define GX_VS(LMV, LTV) do { GX_VS_K((k_vol_step<LMV, LTV, VS_MAIN>), VS_MAIN); GX_VS_K((k_vol_step<LMV, LTV, VS_SHADOW>), VS_SHADOW); GX_VS_K((k_vol_step<LMV, LTV, VS_MIS>), VS_MIS); } while (0)
#define GX_VST(LTV) do { GX_VS_K((k_vol_step<LM_ALL, LTV, VS_MAIN, true>), VS_MAIN); GX_VS_K((k_vol_step<LM_ALL, LTV, VS_SHADOW, true>), VS_SHADOW); GX_VS_K((k_vol_step<LM_ALL, LTV, VS_MIS, true>), VS_MIS); } while (0)
            if (pl.textured_scene) { if (pl.area_only) GX_VST(LT_AREA); else GX_VST(LT_ALL); }
            else if (pl.area_only) { if (class_mask <= 1) GX_VS(LM_DIFFUSE, LT_AREA); else if (class_mask <= 3) GX_VS(LM_GLOSSY, LT_AREA); else GX_VS(LM_ALL, LT_AREA); }
            else { if (class_mask <= 1) GX_VS(LM_DIFFUSE, LT_ALL); else if (class_mask <= 3) GX_VS(LM_GLOSSY, LT_ALL); else GX_VS(LM_ALL, LT_ALL); }
#undef GX_VST
#undef GX_VS
#undef GX_VS_K
            run.launches += 2;
        }
        ++run.launches;
        run.compact(COMPACT_FLAGS, q_in, n, st.pflags.p, 4, 2, &dctr->q_next, q_cur, st.queue_nee.p, nullptr);
        if (run.timing) run.timer.end(stream);
        HIP_TRY(hipMemcpyAsync(s->h_counters, dctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = compact_stalled(*s->h_counters)) return rc;
        n = (int)s->h_counters->q_next;
        n_media = (int)s->h_counters->q_nee;
        q_media = st.queue_nee.p;
        q_in = q_cur;
        std::swap(q_cur, q_other);
        if (Knobs::vol_pack() && n >= (1 << 16) && 2ll * n <= span) {
            // the survivors fill at most half of the span they are spread over: move them to the front of the other set
            const VolPackSet from = st.pack_set(in_alt), to = st.pack_set(!in_alt);
            hipLaunchKernelGGL(k_vol_pack, dim3(grid_for(n)), dim3(kBlock), 0, stream, q_in, n, from, to, st.vol_newslot.p);
            if (n_media > 0) hipLaunchKernelGGL(k_vol_remap, dim3(grid_for(n_media)), dim3(kBlock), 0, stream, st.queue_nee.p, n_media, (const int *)st.vol_newslot.p);
            run.launches += 2;
            in_alt = !in_alt;
            run.bind_set(to);
            q_in = nullptr;   // the queue is the identity again
            span = n;
        }
        if (++guard > (1 << 20)) { set_error("path loop did not terminate"); return GNXR_ERR_INVALID; }
    }
    if (in_alt) run.bind_set(st.pack_set(false));   // the next pass's k_raygen writes the primary set again
    return GNXR_OK;
}

// Whitted / DirectLighting / VolPath render one pass at a time: raygen, the pass, resolve.
static int run_passes(RenderRun &run) {
    const RenderPlan &pl = run.pl;
    for (long long u0 = pl.unit_begin; u0 < pl.unit_end; u0 += pl.k) {
        const int kk = (int)std::min<long long>(pl.k, pl.unit_end - u0);
        run.raygen(run.pa, u0, kk, run.list_media ? run.st.pflags.p : nullptr);
        ++run.launches;
        if (int rc = pl.whitted ? run_whitted_pass(run, u0, kk) : run_volpath_pass(run, u0, kk)) return rc;
        PathArrays pr = run.pa;
        if (pl.volpath) pr.L = run.st.vol_Lout.p;   // VolPath: results sit at the paths' original slots (packing moves the working state)
        run.resolve(pr, u0, kk);
        ++run.launches;
        ++run.passes;
        if (run.timing) { HIP_TRY(hipStreamSynchronize(run.stream)); run.timer.collect(); }
    }
    return GNXR_OK;
}

// after the final synchronisation: s->h_counters holds the device counters of the whole render
static void fill_stats(const RenderRun &run, double seconds_render, double seconds_total, gnxr_stats *stats) {
    const RenderPlan &pl = run.pl;
    const Counters &c = *run.s->h_counters;
    unsigned long long rays_closest = run.rays_closest, rays_any = run.rays_any, rays_mis = run.rays_mis, media_segments = run.media_segments;
    memset(stats, 0, sizeof(*stats));
    if (pl.path_int()) {   // the device-driven loop counts on the device; only the camera rays are known to the host
        rays_closest = run.new_paths + c.rays_continue + c.rays_mis;
        rays_any = c.rays_shadow;
        rays_mis = c.rays_mis;
    }
    if (pl.volpath) {   // a segment k_vol_media left at its step cap was traced and handed over once more: the same ray, counted once
        rays_closest -= c.media_cont;
        media_segments -= c.media_cont;
    }
    stats->rays_closest = rays_closest + (pl.whitted ? c.whitted_mis : 0);
    stats->rays_any = pl.whitted ? c.whitted_shadow : rays_any;
    stats->camera_samples = run.src ? (uint64_t)run.src->n : (uint64_t)run.r.npix * pl.nsamples();
    stats->nodes_visited = c.nodes;
    stats->tris_tested = c.tris;
    stats->seconds_render = seconds_render;
    stats->seconds_total = seconds_total;
    stats->kernel_launches = run.launches;
    stats->passes = run.passes;
    stats->passes_in_flight = (uint32_t)pl.in_flight;
    stats->loop_iterations = run.loop_iterations;
    stats->state_bytes = RenderState::state_bytes(pl);
    stats->seconds_closest = run.timer.seconds[0]; stats->seconds_nee = run.timer.seconds[1]; stats->seconds_shade = run.timer.seconds[2];
    stats->seconds_trace = run.timer.seconds[0] + run.timer.seconds[1];
    stats->launches_closest = run.timer.launches[0]; stats->launches_nee = run.timer.launches[1];
    stats->rays_closest_nee = rays_mis;
    stats->media_segments = media_segments;
    stats->media_steps = c.media_steps;
    stats->leaf_retests = c.retests;
    stats->nodes_from_memory = c.nodes_global;
}

// One device: the wavefront loop over the rows `pin` assigns to this shard, on the device the scene's tables live on.
// reserve_only: stop after the allocations (gnxr_render_reserve).
// src != nullptr: Li for the caller's rays instead (gnxr_li_device); `d_rgba_out` is then unused.
// views != nullptr: the views' cameras instead of the scene's (gnxr_render_views_device); `d_rgba_out` holds n_views images.
// pix != nullptr: rounds over lists of pixels instead of passes over the image (gnxr_render_adaptive_device, run_adaptive).
static int run_adaptive(RenderRun &run, RenderPlan &pl, PixelListSource &pix, void *d_rgba_out);
static void adaptive_stats(const PixelListSource &pix, gnxr_stats *stats);
static int render_one(gnxr_scene *s, const gnxr_render_params *pin, void *d_rgba_out, void *hip_stream, gnxr_stats *stats, bool reserve_only = false,
                      const RaySource *src = nullptr, const ViewSource *views = nullptr, PixelListSource *pix = nullptr, const FilmSource *film = nullptr) {
    if (!s || !pin || (!d_rgba_out && !src && !(film && film->accum))) { set_error("null argument"); return GNXR_ERR_INVALID; }
    RenderPlan pl;
    int rc = plan_render(s->cs, pin, src, views, pix, &pl);
    if (rc) return rc;
    const gnxr_render_params &p = pl.p;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    if (int brc = s->bind()) return brc;
    auto t_start = std::chrono::steady_clock::now();
    hipStream_t stream = (hipStream_t)hip_stream;
    if ((rc = s->ensure_grid(p.light_strategy)) != GNXR_OK) return rc;
    DScene sc = s->device_scene(p.width, p.height);
    if ((rc = halton_index_bound(&sc.st.h, p.spp, pl.max_light_samples)) != GNXR_OK) return rc;
    if (pl.whitted) sc.materials = s->materials_single.p + 1;
    sc.escape_class = pl.escape_queue ? 3 : 0;
    DRender r;
    memset(&r, 0, sizeof(r));
    // views: one DCamera per view; r.cam (the first view's) is read by no kernel of a views render
    bool views_mixed_media = false;
    if (views) {
        s->h_view_cams.resize(std::max<size_t>(s->h_view_cams.size(), (size_t)views->n_views));
        make_view_cameras(views->cameras, views->media, views->n_views, p.width, p.height, s->h_view_cams.data());
        for (int v = 1; v < views->n_views; ++v) if (s->h_view_cams[v].medium != s->h_view_cams[0].medium) views_mixed_media = true;
        r.cam = s->h_view_cams[0];
    } else {
        r.cam = make_camera(s->cs.camera, p.width, p.height, s->cs.camera_medium);
    }
    r.W = p.width; r.H = p.height; r.spp = p.spp; r.max_depth = p.max_depth; r.rr_threshold = p.rr_threshold;
    r.shard_index = p.shard_index; r.shard_count = p.shard_count; r.shard_rows = p.shard_rows;
    r.npix = pl.npix;
    if (r.npix == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }
    {   // one query of the free memory serves both rules of the plan that read it
        size_t free_b = 0, total_b = 0;
        const bool have_mem = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        if ((rc = pl.size_passes(s->st.L.n, have_mem, free_b)) != GNXR_OK) return rc;
    }
    if ((rc = s->st.reserve(pl)) != GNXR_OK) return rc;
    if (pix && (rc = s->st.reserve_adaptive(pl)) != GNXR_OK) return rc;
    if (pix && !s->h_ad_count && hipHostMalloc((void **)&s->h_ad_count, sizeof(unsigned int)) != hipSuccess) { s->h_ad_count = nullptr; set_error("hipHostMalloc failed"); return GNXR_ERR_OOM; }
    if (reserve_only) { if (stats) memset(stats, 0, sizeof(*stats)); return GNXR_OK; }

    RenderRun run(s, stream, pl, src, views, pix, sc, r);
    run.list_media = pl.volpath && (src || views_mixed_media);
    run.film = film;
    run.film_accum = film && film->accum ? film->accum : s->st.accum.p;
    // (stream-ordered: the table is read by this call's raygen kernels only, and the call returns after the stream has drained)
    if (views) HIP_TRY(hipMemcpyAsync(s->st.view_cams.p, s->h_view_cams.data(), (size_t)views->n_views * sizeof(DCamera), hipMemcpyHostToDevice, stream));
    if (!src) HIP_TRY(hipMemsetAsync(s->st.accum.p, 0, sizeof(float4) * r.npix, stream));
    if (film && film->accum && !film->keep) HIP_TRY(hipMemsetAsync(film->accum, 0, sizeof(float4) * r.npix, stream));
    HIP_TRY(hipMemsetAsync(run.dctr, 0, sizeof(Counters), stream));
    HIP_TRY(hipMemsetAsync(s->st.compact_ticket.p, 0, 2 * sizeof(unsigned int), stream));   // once per render; from pass to pass k_compact zeroes its successor's counter
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, stream));
    if (pix) { if ((rc = run_adaptive(run, pl, *pix, d_rgba_out)) != GNXR_OK) return rc; }
    else if ((rc = pl.path_int() ? run_path_loop(run) : run_passes(run)) != GNXR_OK) return rc;
    if (film) {
        if (d_rgba_out) { hipLaunchKernelGGL(k_film_resolve, dim3(grid_for(r.npix)), dim3(kBlock), 0, stream, (const float4 *)run.film_accum, (long long)r.npix, (float4 *)d_rgba_out); ++run.launches; }
    } else if (!src && !pix) {
        hipLaunchKernelGGL(k_finish, dim3(grid_for(r.npix)), dim3(kBlock), 0, stream, r, (const float4 *)s->st.accum.p, (float4 *)d_rgba_out);
        ++run.launches;
    }
    HIP_TRY(hipEventRecord(ev.b, stream));
    HIP_TRY(hipMemcpyAsync(s->h_counters, run.dctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    if (run.timing) run.timer.collect();
    if ((rc = compact_stalled(*s->h_counters)) != GNXR_OK) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    if (stats) fill_stats(run, ms * 1e-3, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), stats);
    if (stats && pix) adaptive_stats(*pix, stats);
    if (src && s->h_counters->li_bad) {
        set_error("gnxr_li_device: sample record %llu is out of range (px in [0, %d), py in [0, %d), s in [0, %d), medium in [-1, %d)); its L is (0, 0, 0, 0)",
                  ~s->h_counters->li_bad, p.width, p.height, p.spp, run.n_scene_media);
        return GNXR_ERR_INVALID;
    }
    return GNXR_OK;
}

// Several devices behind one handle (gnxr_init_devices): the rows of this render are dealt round-robin over the devices, each
// device renders its rows concurrently (one host thread and one stream per device, nothing exchanged during rendering) into a
// full-size plane of its own, and the rows are then copied into the caller's image on the primary device (peer copies over xGMI,
// one strided 2D copy per device).  A single device takes the direct path.
static int render_sharded(gnxr_scene *s, const gnxr_render_params *pin, void *d_rgba_out, void *hip_stream, gnxr_stats *stats, bool reserve_only = false) {
    if (!s || !pin || !d_rgba_out) { set_error("null argument"); return GNXR_ERR_INVALID; }
    const int nd = (int)s->n_copies();
    if (nd == 1) return render_one(s, pin, d_rgba_out, hip_stream, stats, reserve_only);
    gnxr_render_params base = *pin;
    if (base.shard_count <= 0) base.shard_count = 1;
    if (base.shard_rows <= 0) base.shard_rows = 1;
    if (base.shard_rows != 1) { set_error("multi-device rendering deals single rows: shard_rows must be 1"); return GNXR_ERR_UNSUPPORTED; }
    if (base.width <= 0 || base.height <= 0 || base.shard_index < 0 || base.shard_index >= base.shard_count) return invalid_render_params();
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const size_t npx = (size_t)base.width * base.height;
    std::vector<int> rcs(nd, GNXR_OK);
    std::vector<std::string> errs(nd);
    std::vector<gnxr_stats> sts(nd);
    std::vector<int> staged(nd, 0);   // rows a shard left in its pinned staging buffer (no peer access between its device and the primary)
    hipStream_t caller = (hipStream_t)hip_stream;
    int rc = s->bind();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(caller));   // the image must be safe to write from the other devices' streams
    auto worker = [&](int i) {
        gnxr_scene *r = s->copy(i);
        gnxr_render_params p = base;   // rows y == shard_index (mod shard_count) of the caller, every nd-th of them
        p.shard_index = base.shard_index + base.shard_count * i;
        p.shard_count = base.shard_count * nd;
        int rc_ = r->bind();
        void *dst = d_rgba_out;
        if (rc_ == GNXR_OK && i > 0) { rc_ = r->shard_out.alloc(npx); dst = r->shard_out.p; }
        if (rc_ == GNXR_OK) rc_ = render_one(r, &p, dst, i == 0 ? hip_stream : nullptr, &sts[i], reserve_only);
        if (rc_ == GNXR_OK && i > 0 && !reserve_only) {
            // rows p.shard_index, + p.shard_count, ...
            const int first = p.shard_index, step = p.shard_count;
            const int rows = first < base.height ? (base.height - first + step - 1) / step : 0;
            const size_t rowb = (size_t)base.width * sizeof(float4);
            const bool peer = (size_t)i < g_peer_ok.size() ? g_peer_ok[i] != 0 : r->device == s->device;
            if (rows > 0 && peer) {
                // one strided copy into the primary's image (peer access was enabled both ways at init: the runtime routes it over the link)
                hipError_t e = hipMemcpy2DAsync((char *)d_rgba_out + (size_t)first * rowb, rowb * step, (const char *)dst + (size_t)first * rowb, rowb * step, rowb, rows,
                                                hipMemcpyDeviceToDevice, nullptr);
                if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
                if (e != hipSuccess) { set_error("peer copy from device %d failed: %s", r->device, hipGetErrorString(e)); rc_ = hip_status(e); }
            } else if (rows > 0) {
                // no peer access for this pair: the shard's rows go to a pinned host buffer here (packed), and the primary uploads them after the join
                if (r->h_stage_bytes < rowb * rows) {
                    if (r->h_stage) (void)hipHostFree(r->h_stage);
                    r->h_stage = nullptr; r->h_stage_bytes = 0;
                    if (hipHostMalloc(&r->h_stage, rowb * rows) != hipSuccess) { set_error("hipHostMalloc of the %zu-byte staging buffer for device %d failed", rowb * rows, r->device); rc_ = GNXR_ERR_OOM; }
                    else r->h_stage_bytes = rowb * rows;
                }
                if (rc_ == GNXR_OK) {
                    hipError_t e = hipMemcpy2D(r->h_stage, rowb, (const char *)dst + (size_t)first * rowb, rowb * step, rowb, rows, hipMemcpyDeviceToHost);
                    if (e != hipSuccess) { set_error("download of device %d's rows failed: %s", r->device, hipGetErrorString(e)); rc_ = hip_status(e); }
                    else staged[i] = rows;
                }
            }
        }
        rcs[i] = rc_;
        if (rc_ != GNXR_OK) errs[i] = get_error();
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nd; ++i) pool.emplace_back(worker, i);
    worker(0);
    for (auto &t : pool) t.join();
    (void)s->bind();
    for (int i = 1; i < nd; ++i) {   // host-staged shards: upload their rows into the image on the primary device
        if (staged[i] <= 0 || rcs[i] != GNXR_OK) continue;
        gnxr_scene *r = s->copy(i);
        const int first = base.shard_index + base.shard_count * i, step = base.shard_count * nd;
        const size_t rowb = (size_t)base.width * sizeof(float4);
        hipError_t e = hipMemcpy2D((char *)d_rgba_out + (size_t)first * rowb, rowb * step, r->h_stage, rowb, rowb, staged[i], hipMemcpyHostToDevice);
        if (e != hipSuccess) { rcs[i] = hip_status(e); errs[i] = std::string("upload of the staged rows failed: ") + hipGetErrorString(e); }
    }
    for (int i = 0; i < nd; ++i) if (rcs[i] != GNXR_OK) { set_error("device %d: %s", s->copy(i)->device, errs[i].c_str()); return rcs[i]; }
    if (stats) {
        *stats = sts[0];
        for (int i = 1; i < nd; ++i) {
            const gnxr_stats &t = sts[i];
            stats->rays_closest += t.rays_closest; stats->rays_any += t.rays_any; stats->camera_samples += t.camera_samples;
            stats->nodes_visited += t.nodes_visited; stats->tris_tested += t.tris_tested; stats->kernel_launches += t.kernel_launches;
            stats->rays_closest_nee += t.rays_closest_nee; stats->media_segments += t.media_segments; stats->media_steps += t.media_steps; stats->leaf_retests += t.leaf_retests;
            stats->nodes_from_memory += t.nodes_from_memory;
            stats->seconds_render = std::max(stats->seconds_render, t.seconds_render); stats->seconds_total = std::max(stats->seconds_total, t.seconds_total);
            stats->passes = std::max(stats->passes, t.passes);
        }
    }
    return GNXR_OK;
}
