// display_kernel.hip.h -- the display stage (the definition: include/gnxr.h, "Display stage"): from a linear float RGBA image in device
// memory to sRGB bytes, with an exposure metered on the device.
//
//   k_luminance_histogram   one lane per pixel and one dwordx4 load per pixel, a grid-stride loop over all views in one launch.  The bin
//                 comes from the bit pattern of the luminance (integers only: no libm, no dependence on the order of the atomics).
//                 Counts go to a per-block LDS histogram of 260 words with LDS integer atomics; the block adds its non-zero words to
//                 the view's histogram in memory with one atomicAdd each.  A block's 256 consecutive pixels may belong to several views
//                 (the end of a view, or views smaller than a block): the view of the block's first and last pixel is uniform over the
//                 block, so the block counts one view at a time and flushes its LDS words whenever the view changes, also between two
//                 turns of the grid-stride loop.  The flushes are what the kernel costs: two blocks per CU, not eight
//   k_exposure    one wave per view: the lanes load the 256 bins into LDS and sum them, lane 0 runs the definition sequentially -- the
//                 order of the operations is the definition
//   k_tonemap     one lane per pixel: one dwordx4 load, the curve on three channels, one dword store.  The curve and the sRGB encoding
//                 are template arguments (only REFERENCE carries gx_exp, only SRGB carries gx_pow)
// Every operation is a single fp32 operation in the order gnxr.h writes (the library is built with -ffp-contract=off; division is IEEE).
#pragma once
#include "kernels.hip.h"

namespace gnxr {

constexpr int kHistWords = 260;   // GNXR_HISTOGRAM_WORDS: 256 bins, below, above, not finite, 0

GX_DEV float display_lum(float r, float g, float b) { return (0.212671f * r + 0.715160f * g) + 0.072169f * b; }

// the word of a view's histogram that a pixel counts in.  bias = (min_log2 + 127) << 4: the bin of 2^min_log2
GX_DEV int display_bin(float4 c, int bias) {
    const float l = display_lum(c.x, c.y, c.z);
    const uint32_t bits = __float_as_uint(l);
    if ((bits & 0x7f800000u) == 0x7f800000u) return 258;   // NaN, +-inf
    if (!(l > 0.f)) return 256;                             // 0, -0, negatives
    const int k = (int)(bits >> 19) - bias;
    return k < 0 ? 256 : (k > 255 ? 257 : k);               // (subnormals are below every min_log2)
}

// npix = n_views * wh pixels, both below 2^31 (check_view_pixels).  hist: n_views * kHistWords words, zeroed on the stream before.
static __global__ void __launch_bounds__(kBlock) k_luminance_histogram(const float4 *__restrict__ rgba, int npix, int wh, int bias, unsigned int *__restrict__ hist) {
    __shared__ unsigned int bins[kHistWords];
    for (int i = threadIdx.x; i < kHistWords; i += kBlock) bins[i] = 0;
    __syncthreads();
    // the block's LDS words to `view`'s histogram, and back to 0
    auto flush = [&](int view) {
        __syncthreads();
        for (int i = threadIdx.x; i < kHistWords; i += kBlock) {
            const unsigned int c = bins[i];
            if (c) { atomicAdd(&hist[(size_t)view * kHistWords + i], c); bins[i] = 0; }
        }
        __syncthreads();
    };
    int held = -1;   // the view whose pixels the LDS words count (uniform over the block)
    for (long long base = (long long)blockIdx.x * kBlock; base < npix; base += (long long)gridDim.x * kBlock) {
        const int p = (int)base + (int)threadIdx.x;
        const bool inside = p < npix;
        int k = 0, view = -1;
        if (inside) {
            k = display_bin(rgba[p], bias);
            view = p / wh;
        }
        const int last = (int)(base + kBlock - 1 < npix ? base + kBlock - 1 : npix - 1);
        const int v0 = (int)base / wh, v1 = last / wh;
        for (int v = v0; v <= v1; ++v) {   // uniform over the block; v0 == v1 except where a view ends
            if (held >= 0 && held != v) flush(held);
            held = v;
            if (inside && view == v) atomicAdd(&bins[k], 1u);
        }
    }
    if (held >= 0) flush(held);
}

struct ExposureParams {
    int min_log2;
    float key, low, high, rate, min_exposure, max_exposure;
};

constexpr int kExposureBlock = 64;   // one wave per view: 64 lanes x 4 words are the 256 bins

struct ExposureSums { float skip, keep, sw, sx; };
GX_DEV void exposure_bin(unsigned int count, int k, ExposureSums *e) {
    float c = (float)count;
    const float s = fminf(c, e->skip);
    c -= s; e->skip -= s;
    const float t = fminf(c, e->keep);
    e->keep -= t;
    e->sw += t;
    e->sx += t * ((float)k + 0.5f);
}

// One wave per view.  Every lane loads four of the view's 256 bins with one dwordx4 load (a view's histogram is 65 x 16 bytes: aligned);
// the integer total is a wave reduction; then lane 0 alone runs the definition in its order over the bins in LDS, four per LDS read, the
// next four requested before these are used.  prev: nullptr, or the records of the frame before; may be `out` itself (a view's record
// is read before it is written, by the same lane).
static __global__ void __launch_bounds__(kExposureBlock) k_exposure(const unsigned int *__restrict__ hist, const float4 *prev, float4 *out, int n_views, ExposureParams ep) {
    __shared__ uint4 bins4[kExposureBlock];
    for (long long v = blockIdx.x; v < n_views; v += gridDim.x) {
        const uint4 mine = reinterpret_cast<const uint4 *>(hist + (size_t)v * kHistWords)[threadIdx.x];
        bins4[threadIdx.x] = mine;
        unsigned int n = (mine.x + mine.y) + (mine.z + mine.w);   // (integers: any order)
        for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
        __syncthreads();
        if (threadIdx.x == 0) {
            const float total = (float)n;
            ExposureSums e;
            e.skip = total * ep.low;
            e.keep = total * ep.high - e.skip;
            e.sw = 0.f; e.sx = 0.f;
            uint4 w = bins4[0];
            for (int q = 0; q < kExposureBlock; ++q) {
                const uint4 next = bins4[q + 1 < kExposureBlock ? q + 1 : q];
                exposure_bin(w.x, 4 * q, &e);
                exposure_bin(w.y, 4 * q + 1, &e);
                exposure_bin(w.z, 4 * q + 2, &e);
                exposure_bin(w.w, 4 * q + 3, &e);
                w = next;
            }
            const float pv = prev ? prev[v].x : 0.f;
            const bool prev_ok = pv > 0.f && gx_finite(pv);
            float L = 0.f, target;
            if (e.sw > 0.f) {
                const float m = e.sx / e.sw;
                L = (float)ep.min_log2 + m * 0.0625f;
                target = fminf(fmaxf(ep.key * gx_pow(2.0f, -L), ep.min_exposure), ep.max_exposure);
            } else {
                target = prev_ok ? pv : 1.0f;   // black, or everything out of range: hold
            }
            const float exposure = prev_ok ? pv + (target - pv) * ep.rate : target;
            out[v] = make_float4(exposure, target, L, e.sw);
        }
        __syncthreads();   // (the next view overwrites the bins)
    }
}

enum { kToneLinear = 0, kToneReference = 1, kToneReinhard = 2, kToneAces = 3 };

template <int CURVE, bool SRGB>
GX_DEV unsigned int tonemap_channel(float in, float E, float ww, bool round) {
    float x = in * E;
    if (!(x > 0.f)) x = 0.f;   // NaN, negatives
    x = fminf(x, 65504.f);
    float y;
    if (CURVE == kToneLinear) y = x;
    else if (CURVE == kToneReference) y = 1.0f - gx_exp(-x / 0.25f);
    else if (CURVE == kToneReinhard) y = (x * (1.0f + x / ww)) / (1.0f + x);
    else y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    y = fminf(fmaxf(y, 0.f), 1.f);
    float z = y;
    if (SRGB) z = y <= 0.0031308f ? 12.92f * y : 1.055f * gx_pow(y, 1.f / 2.4f) - 0.055f;
    return (unsigned int)(round ? z * 255.f + 0.5f : z * 255.f) & 0xffu;   // (z in [0, 1]: the conversion is in range)
}

// exposure: nullptr (E = e_param for every view) or one float4 per view whose x is E.  ww = white * white.
template <int CURVE, bool SRGB>
static __global__ void __launch_bounds__(kBlock) k_tonemap(const float4 *__restrict__ rgba, const float4 *__restrict__ exposure, int npix, int wh, float e_param, float ww,
                                                           int round, unsigned int *__restrict__ out) {
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < npix; q += (long long)gridDim.x * kBlock) {
        const int p = (int)q;
        const float4 c = rgba[p];
        const float E = exposure ? exposure[p / wh].x : e_param;
        const unsigned int r = tonemap_channel<CURVE, SRGB>(c.x, E, ww, round != 0);
        const unsigned int g = tonemap_channel<CURVE, SRGB>(c.y, E, ww, round != 0);
        const unsigned int b = tonemap_channel<CURVE, SRGB>(c.z, E, ww, round != 0);
        out[p] = r | (g << 8) | (b << 16) | 0xff000000u;
    }
}

}  // namespace gnxr
