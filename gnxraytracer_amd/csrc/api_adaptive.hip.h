// api_adaptive.hip.h -- gnxr_render_adaptive_device: render to a noise threshold, per-pixel sample counts (the definition: include/gnxr.h).
// render_one's loops (api_render.hip.h) with a PixelListSource in place of the image: the rounds of run_adaptive, each one pass of the loops
// over the paths of the round's active pixels (adaptive_kernel.hip.h).  Part of api.hip's translation unit.
#pragma once

// The per-pixel arrays of an adaptive call beyond accum (RenderState, api_scene.hip.h); they only ever grow.
int RenderState::reserve_adaptive(const RenderPlan &pl) {
    const size_t npix = (size_t)pl.npix;
    int rc;
    if ((rc = ad_A.alloc(npix)) || (rc = ad_state[0].alloc(npix)) || (rc = ad_state[1].alloc(npix)) || (rc = ad_list[0].alloc(npix)) || (rc = ad_list[1].alloc(npix)) ||
        (rc = ad_totals.alloc(8)))   // four totals of the compaction + the word the host reads
        return rc;
    return GNXR_OK;
}

// The rounds.  Round 0 gives every pixel samples [0, min_spp); every later round gives the pixels still active their next
// max(step_spp, n / 8), cut at spp (adaptive_round_samples).  A round is one run of the integrator's loop over n_active * ns paths (unit = one path, cut into chunks of pl.k paths as the
// plan sized them for the largest round); its finished chunks are added to S and A in chunk order (RenderRun::resolve -> k_adaptive_accum).
// Then, on the stream: the criterion per active pixel, the guard pass over the image, the compaction of its bytes into the next list --
// and ONE 4-byte count comes back to size the next round.  All active pixels share their sample count (a stopped pixel never restarts),
// so the host knows when the budget is reached and what the totals are without reading anything else.
static int run_adaptive(RenderRun &run, RenderPlan &pl, PixelListSource &pix, void *d_rgba_out) {
    gnxr_scene *s = run.s;
    RenderState &st = run.st;
    hipStream_t stream = run.stream;
    const gnxr_adaptive_params &ap = pix.ap;
    const int npix = pl.npix, W = pl.p.width, H = pl.p.height, spp = pl.p.spp;
    HIP_TRY(hipMemsetAsync(st.ad_A.p, 0, sizeof(float4) * (size_t)npix, stream));
    HIP_TRY(hipMemsetAsync(st.ad_totals.p, 0, 8 * sizeof(unsigned int), stream));
    PixelRound &rd = pix.round;
    rd.list = nullptr; rd.n_active = npix; rd.n0 = 0; rd.npix = npix;
    int cur = 0, rounds = 0;
    long long samples = 0, at_budget = 0;
    for (;;) {
        const int ns = adaptive_round_samples(ap, spp, rd.n0);
        pl.unit_begin = 0;
        pl.unit_end = (long long)rd.n_active * ns;
        if (int rc = pl.path_int() ? run_path_loop(run) : run_passes(run)) return rc;
        ++rounds;
        samples += pl.unit_end;
        const int n = rd.n0 + ns;
        hipLaunchKernelGGL(k_adaptive_criterion, dim3(grid_for(rd.n_active)), dim3(kBlock), 0, stream, rd, n, ap.threshold, ap.floor, st.accum.p, (const float4 *)st.ad_A.p, st.ad_state[cur].p);
        ++run.launches;
        if (n >= spp) { at_budget = rd.n_active; break; }
        hipLaunchKernelGGL(k_adaptive_guard, dim3(grid_for(npix)), dim3(kBlock), 0, stream, (const unsigned char *)st.ad_state[cur].p, W, H, ap.guard, st.ad_state[1 - cur].p);
        ++run.launches;
        // bit 0 of the guard pass's bytes -> the next list, ascending (the three other counts of COMPACT_FLAGS are zero: no other bit is set)
        int *next = st.ad_list[rounds & 1].p;
        run.compact(COMPACT_FLAGS, nullptr, npix, st.ad_state[1 - cur].p, 4, 2, st.ad_totals.p, next, next, nullptr);
        // the count, or ~0u for a compaction that gave up: its list is never used
        hipLaunchKernelGGL(k_adaptive_count, dim3(1), dim3(64), 0, stream, (const unsigned int *)st.ad_totals.p, (const Counters *)run.dctr, st.ad_totals.p + 4);
        ++run.launches;
        GX_CHECK_LAUNCHES("an adaptive round");
        HIP_TRY(hipMemcpyAsync(s->h_ad_count, st.ad_totals.p + 4, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const unsigned int n_next = *s->h_ad_count;
        if (n_next == ~0u) { Counters stalled; memset(&stalled, 0, sizeof(stalled)); stalled.compact_stall = 1; return compact_stalled(stalled); }
        if (n_next > (unsigned)rd.n_active) { set_error("adaptive: the list of a round grew (%u pixels after %d)", n_next, rd.n_active); return GNXR_ERR_RUNTIME; }
        if (run.timing) run.timer.collect();
        if (n_next == 0) break;
        rd.list = next; rd.n_active = (int)n_next; rd.n0 = n;
        cur = 1 - cur;
    }
    hipLaunchKernelGGL(k_adaptive_finish, dim3(grid_for(npix)), dim3(kBlock), 0, stream, (const float4 *)st.accum.p, npix, (float4 *)d_rgba_out, (int *)pix.count_out);
    ++run.launches;
    pix.rounds = rounds; pix.samples = samples; pix.at_budget = at_budget;
    return GNXR_OK;
}

// gnxr_stats of an adaptive call: filled as by a render (fill_stats); the camera samples are the sum of the per-pixel counts
static void adaptive_stats(const PixelListSource &pix, gnxr_stats *stats) { stats->camera_samples = (uint64_t)pix.samples; }

extern "C" {

int gnxr_render_adaptive_device(gnxr_scene *s, const gnxr_render_params *p, const gnxr_adaptive_params *ap, void *d_rgba_out, int32_t *d_count_out, void *hip_stream,
                                gnxr_stats *stats, gnxr_adaptive_info *info) {
    if (!s || !p || !ap || !info) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    if (ap->struct_size != (int32_t)sizeof(gnxr_adaptive_params) || info->struct_size != (int32_t)sizeof(gnxr_adaptive_info)) {
        set_error("adaptive: struct_size must be sizeof(gnxr_adaptive_params) = %zu and sizeof(gnxr_adaptive_info) = %zu", sizeof(gnxr_adaptive_params), sizeof(gnxr_adaptive_info));
        return GNXR_ERR_INVALID;
    }
    if (p->spp_begin != 0 || p->spp_end != 0) { set_error("adaptive: spp_begin and spp_end must be 0 (every pixel starts at sample 0 and stops where the criterion says)"); return GNXR_ERR_INVALID; }
    if (int rc = check_unsharded(*p, "adaptive", "the guard window reads the neighbouring rows")) return rc;
    if (!image_and_samples_ok(*p) || p->max_depth < 0 || p->max_depth > 250) return invalid_render_params();
    if ((long long)p->width * p->height > 0x7fffffffll) { set_error("adaptive: width * height overflows the 32-bit pixel index"); return GNXR_ERR_INVALID; }
    if (ap->min_spp < 1 || ap->min_spp > p->spp || ap->step_spp < 1 || ap->guard < 0 || ap->guard > 8 || !(ap->threshold >= 0.f) || !(ap->floor >= 0.f)) {
        set_error("adaptive: min_spp in [1, spp], step_spp >= 1, guard in [0, 8], threshold >= 0 and floor >= 0 (no NaN) are required");
        return GNXR_ERR_INVALID;
    }
    if (!d_rgba_out || ((uintptr_t)d_rgba_out & 15u) != 0) { set_error("d_rgba_out is null or not 16-byte aligned"); return GNXR_ERR_INVALID; }
    if (((uintptr_t)d_count_out & 3u) != 0) { set_error("d_count_out is not 4-byte aligned"); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    const size_t npix = (size_t)p->width * p->height;
    const QueryArg args[] = {{d_rgba_out, npix * sizeof(float4), "d_rgba_out"}, {d_count_out, npix * sizeof(int32_t), "d_count_out"}};
    DeviceCall call;
    if (int rc = call.bind(s, args)) return rc;
    gnxr_render_params pp = *p;
    pp.shard_count = 1; pp.shard_rows = 1;
    PixelListSource pix;
    memset(&pix, 0, sizeof(pix));
    pix.ap = *ap;
    pix.count_out = d_count_out;
    if (int rc = render_one(call.r, &pp, d_rgba_out, hip_stream, stats, /*reserve_only=*/false, nullptr, nullptr, &pix)) return rc;
    info->rounds = pix.rounds; info->samples = pix.samples; info->pixels_at_budget = pix.at_budget;
    return GNXR_OK;
}

}  // extern "C"
