// adaptive_kernel.hip.h -- adaptive sampling (gnxr_render_adaptive_device): the image stages of a render whose pixels stop at different
// sample counts.
//
// The call works in rounds.  A round gives every ACTIVE pixel its next `ns` samples (adaptive_round_samples, api_render.hip.h: min_spp, then
// max(step_spp, n / 8), cut at spp); the active pixels are a device list in ascending
// pixel order (round 0: every pixel, no list).  A pixel that has stopped never restarts, so every active pixel has taken the same number
// of samples n0 before the round: n0 travels as a kernel argument and the per-pixel count is only written, never gathered.
// Only the stages that depend on the image are here -- tracing, shading, NEE and the media stages run unchanged on the paths they start:
//   k_raygen_pixels      path j of the round -> (pixel list[j % n_active], sample n0 + j / n_active): sample-major, so neighbouring lanes
//                        hold neighbouring pixels; the camera ray is k_raygen's (camera_ray, the same Halton index)
//   k_adaptive_accum     the counterpart of k_resolve for one finished chunk of the round's paths: S += L, and A += L for even samples, one
//                        lane per active pixel, in sample order inside the chunk.  The host hands the chunks over in chunk order
//                        (run_path_loop resolves sub-passes in order), so the sums are added in sample order whatever the chunk size is
//   k_adaptive_criterion one lane per active pixel after the round: the stopping test on (S, A, n), the count, the `noisy` bit
//   k_adaptive_guard     one lane per pixel: active' = active && a pixel of the (2 guard + 1)^2 window, clipped to the image, is active and
//                        noisy.  Plain neighbour reads: the map is one byte per pixel and the window's rows are shared through the caches
//   k_adaptive_finish    S / (float)n and n, in the layout of k_finish
// k_compact<COMPACT_FLAGS> (compact_kernel.hip.h) turns the guard pass's bytes into the next round's list.
// All are plain streaming kernels: no LDS, no scratch, no atomics.  Every list entry is checked against the pixel count before it
// indexes anything, so a compaction that gave up (Counters::compact_stall) cannot turn into a write outside the per-pixel arrays.
//
// Per-pixel state, 42 bytes: S (float4: rgb sums, w = n as int bits -- the accumulator of k_resolve), A (float4), two state bytes
// (ping-pong: bit 0 active, bit 1 noisy) and two list entries (ping-pong).
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// what the image stages of one round read (RenderRun::raygen / resolve: api_render.hip.h, filled by run_adaptive: api_adaptive.hip.h)
struct PixelRound {
    const int *list;     // active pixels, ascending; nullptr: the identity (round 0)
    int n_active;
    int n0;              // samples every active pixel has taken before this round
    int npix;            // W * H: bound of every list entry
};

// Paths [first, first + n_paths) of the round in slots [0, n_paths) of `pa`.
static __global__ void __launch_bounds__(kBlock) k_raygen_pixels(DScene sc, DRender r, PathArrays pa, PixelRound pr, int n_paths, long long first) {
    for (int slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n_paths; slot += gridDim.x * blockDim.x) {
        const long long j = first + slot;
        const int t = (int)(j / pr.n_active);
        const int a = (int)(j - (long long)t * pr.n_active);
        const int lp = pr.list ? pr.list[a] : a;
        float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = make_float4(0.f, 0.f, 1.f, __int_as_float(-1));   // a zero-length ray: hits nothing
        uint32_t index = 0;
        int dim = 5;
        if ((unsigned)lp < (unsigned)pr.npix) {
            const int py = lp / r.W, px = lp - py * r.W;
            index = halton_pixel_offset(sc.st.h, px, py) + (uint32_t)(pr.n0 + t) * (uint32_t)sc.st.h.stride;
            V3 o, d;
            float tMax;
            camera_ray(r.cam, sc.st, px, py, index, &o, &d, &tMax, &dim);
            ro = make_float4(o.x, o.y, o.z, tMax);
            rd = make_float4(d.x, d.y, d.z, __int_as_float(r.cam.medium));
        }
        pa.ray_o[(size_t)slot * kRS] = ro;
        pa.ray_d[(size_t)slot * kRS] = rd;
        pa.beta[(size_t)slot * kRS] = make_float4(1.f, 1.f, 1.f, 1.f);
        pa.L[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        pa.store_meta(slot, index, (uint32_t)dim);
    }
}

// S += L in sample order (A: the even samples) over the paths [first, first + n_paths) of the round, whose radiance is L[0 .. n_paths).
// Path j = t * n_active + a belongs to active pixel a: lane a walks its t in increasing order.  S.w (the count) is kept.
static __global__ void __launch_bounds__(kBlock) k_adaptive_accum(const float4 *__restrict__ L, PixelRound pr, int n_paths, long long first, float4 *__restrict__ S,
                                                                   float4 *__restrict__ A) {
    const long long end = first + n_paths;
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < pr.n_active; a += gridDim.x * blockDim.x) {
        long long t = first > a ? (first - a + pr.n_active - 1) / pr.n_active : 0;
        long long j = t * pr.n_active + a;
        if (j >= end) continue;
        const int lp = pr.list ? pr.list[a] : a;
        if ((unsigned)lp >= (unsigned)pr.npix) continue;
        float4 s = S[lp], e = A[lp];
        for (; j < end; j += pr.n_active, ++t) {
            const float4 l = L[j - first];
            s.x += l.x; s.y += l.y; s.z += l.z;
            if ((((long long)pr.n0 + t) & 1ll) == 0) { e.x += l.x; e.y += l.y; e.z += l.z; }
        }
        S[lp] = s;
        A[lp] = e;
    }
}

// After a round that brought the active pixels to n samples: the count, and noisy = !(e <= threshold * (m + floor * n)) with
// e = |S - 2 A| summed over rgb and m = Sr + Sg + Sb -- single fp32 operations in this order (the library is built with -ffp-contract=off).
// A NaN compares false and keeps the pixel sampling.  state[pixel] = 1 (active) | noisy << 1.
static __global__ void __launch_bounds__(kBlock) k_adaptive_criterion(PixelRound pr, int n, float threshold, float floor_, float4 *__restrict__ S, const float4 *__restrict__ A,
                                                                       unsigned char *__restrict__ state) {
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < pr.n_active; a += gridDim.x * blockDim.x) {
        const int lp = pr.list ? pr.list[a] : a;
        if ((unsigned)lp >= (unsigned)pr.npix) continue;
        const float4 s = S[lp], h = A[lp];
        const float e = (fabsf(s.x - (h.x + h.x)) + fabsf(s.y - (h.y + h.y))) + fabsf(s.z - (h.z + h.z));
        const float m = (s.x + s.y) + s.z;
        const float bound = threshold * (m + floor_ * (float)n);
        const bool noisy = !(e <= bound);
        S[lp].w = __int_as_float(n);
        state[lp] = (unsigned char)(1u | (noisy ? 2u : 0u));
    }
}

// next[p] = 1 where p was active and some pixel of its window (clipped to the image) is active and noisy, else 0 -- for EVERY pixel, so the
// buffer needs no clearing between rounds and is the key array of the compaction that lists the next round's pixels.
static __global__ void __launch_bounds__(kBlock) k_adaptive_guard(const unsigned char *__restrict__ state, int W, int H, int guard, unsigned char *__restrict__ next) {
    const int npix = W * H;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        unsigned keep = 0;
        if (state[p] & 1u) {
            const int y = p / W, x = p - y * W;
            const int x0 = max(0, x - guard), x1 = min(W - 1, x + guard), y0 = max(0, y - guard), y1 = min(H - 1, y + guard);
            for (int qy = y0; qy <= y1 && !keep; ++qy)
                for (int qx = x0; qx <= x1; ++qx) keep |= (state[(size_t)qy * W + qx] >> 1) & 1u;   // (noisy is only ever set together with active)
        }
        next[p] = (unsigned char)keep;
    }
}

// The one word the host reads after a round: the size of the next list, or ~0u when the compaction that made it gave up
// (Counters::compact_stall: its totals and its list are then undefined)
static __global__ void k_adaptive_count(const unsigned int *__restrict__ totals, const Counters *__restrict__ ctr, unsigned int *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = ctr->compact_stall ? ~0u : totals[0];
}

// (Sr / n, Sg / n, Sb / n, 1) and n: k_finish with the pixel's own divisor
static __global__ void __launch_bounds__(kBlock) k_adaptive_finish(const float4 *__restrict__ S, int npix, float4 *__restrict__ out, int *__restrict__ count) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        const float4 s = S[p];
        const int n = __float_as_int(s.w);
        const float fn = (float)n;
        out[p] = make_float4(s.x / fn, s.y / fn, s.z / fn, 1.f);
        if (count) count[p] = n;
    }
}

}  // namespace gnxr
