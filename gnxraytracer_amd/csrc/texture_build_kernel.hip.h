// texture_build_kernel.hip.h -- gnxr_scene_update_textures on the device: the MIP pyramid of an image texture built from its raw texels,
// step by step what build_textures (scene_compile.cpp) builds on the host for gnxr_scene_create.
//
//   k_tex_convert        ImageTexture::GetTexture (ImageTexture.cpp:79-106): the y flip, then convertIn = scale * (gamma ? InverseGammaCorrect(v)
//                        : v), as float4 (rgb_, w lane 0)
//   k_tex_resample_s     MIPMap's Lanczos resample along s (MIPMap.h:93-146) with the texture's wrap mode on the tap index: ry x px, no clamp
//   k_tex_resample_t     ... along t: px x py, clamped to [0, inf)
//   k_tex_pyramid        one level of the box-filter pyramid (MIPMap.h:147-170) from the level below, through MIPMap::Texel's wrap
//   k_tex_pyramid_tail   every level of at most 32 x 32 texels in ONE launch of one block: each level is staged in LDS and the next one
//                        read from there (a level depends on the one below only, so the order of the operations is the chain's)
//
// Every result is bit for bit the host's: each kernel restates its loop of build_textures with the same fp32 operations in the same order.
// The translation unit is compiled with -ffp-contract=off, `/` is the IEEE division and gx_pow is the pinned restatement of glibc's powf
// (device_math.h).  The Lanczos weights depend on the sizes only: the host's resample_weights computes them and they are uploaded.  The
// environment map's kernels (env_build_kernel.hip.h) are the Repeat-only siblings of the resample and pyramid kernels here, with the
// InfiniteAreaLight's own clamping between the passes; they stay as they are.  NaN and infinite texels are outside what is pinned.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "env_build_kernel.hip.h"
#include "gnxr_device_types.h"

namespace gnxr {
namespace texb {

constexpr int kB = 256;           // threads per block
constexpr int kTailSide = 32;     // k_tex_pyramid_tail builds the levels whose sides are at most this
using envb::DResampleWeight;

// build_textures' `wrap` on an index: Repeat is the modulo, Clamp clamps, Black leaves the index alone (the caller skips what is outside)
template <int WRAP>
__device__ __forceinline__ int twrap(int v, int res) {
    if (WRAP == GNXR_WRAP_REPEAT) return envb::emodi(v, res);
    if (WRAP == GNXR_WRAP_CLAMP) return min(max(v, 0), res - 1);
    return v;
}

// InverseGammaCorrect, GNXRayTracer.h:367-371, evaluated left to right as the host writes it
__device__ __forceinline__ float inverse_gamma_correct(float value) {
    if (value <= 0.04045f) return value * 1.f / 12.92f;
    return gx_pow((value + 0.055f) * 1.f / 1.055f, 2.4f);
}

// rgb: w x h x 3 decoded texels, row 0 the top row; tex: w x h float4, row 0 the bottom row
static __global__ void __launch_bounds__(kB) k_tex_convert(const float *__restrict__ rgb, int w, int h, float scale, int gamma, float4 *__restrict__ tex) {
    const long long n = (long long)w * h;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const long long src = ((long long)(h - 1 - y) * w + x) * 3;
        const float v0 = rgb[src], v1 = rgb[src + 1], v2 = rgb[src + 2];
        tex[i] = gamma ? make_float4(scale * inverse_gamma_correct(v0), scale * inverse_gamma_correct(v1), scale * inverse_gamma_correct(v2), 0.f)
                       : make_float4(scale * v0, scale * v1, scale * v2, 0.f);
    }
}

// tex: ry rows of rx texels -> res: ry rows of px.  Four taps accumulated from 0.f in tap order; a tap outside the row is skipped
template <int WRAP>
static __global__ void __launch_bounds__(kB) k_tex_resample_s(const float4 *__restrict__ tex, int rx, int ry, int px, const DResampleWeight *__restrict__ sw,
                                                             float4 *__restrict__ res) {
    const long long n = (long long)ry * px;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / px), s = (int)(i - (long long)t * px);
        const DResampleWeight *wt = sw + s;
        const int first = wt->first;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < 4; ++j) {
            const int o = twrap<WRAP>(first + j, rx);
            if (o >= 0 && o < rx) {
                const float4 v = tex[(long long)t * rx + o];
                const float wj = wt->w[j];
                a0 += wj * v.x; a1 += wj * v.y; a2 += wj * v.z;
            }
        }
        res[i] = make_float4(a0, a1, a2, 0.f);
    }
}

// res: ry rows of px -> out: py rows of px, clamped with clampf(v, 0, INFINITY)'s comparisons
template <int WRAP>
static __global__ void __launch_bounds__(kB) k_tex_resample_t(const float4 *__restrict__ res, int px, int ry, int py, const DResampleWeight *__restrict__ tw,
                                                             float4 *__restrict__ out) {
    const long long n = (long long)py * px;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / px), s = (int)(i - (long long)t * px);
        const DResampleWeight *wt = tw + t;
        const int first = wt->first;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < 4; ++j) {
            const int o = twrap<WRAP>(first + j, ry);
            if (o >= 0 && o < ry) {
                const float4 v = res[(long long)o * px + s];
                const float wj = wt->w[j];
                a0 += wj * v.x; a1 += wj * v.y; a2 += wj * v.z;
            }
        }
        out[i] = make_float4(envb::eclamp0(a0), envb::eclamp0(a1), envb::eclamp0(a2), 0.f);
    }
}

// MIPMap::Texel of the lw x lh level `below` (global memory or LDS): Black is 0 outside, Repeat and Clamp go through the wrap
template <int WRAP>
__device__ __forceinline__ float4 ttexel(const float4 *below, int lw, int lh, int s, int t) {
    if (WRAP == GNXR_WRAP_BLACK && (s < 0 || s >= lw || t < 0 || t >= lh)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return below[(long long)twrap<WRAP>(t, lh) * lw + twrap<WRAP>(s, lw)];
}
// texel (s, t) of the level above `below`: .25f * (the four texels under it), summed in the host's order
template <int WRAP>
__device__ __forceinline__ float4 tbox(const float4 *below, int lw, int lh, int s, int t) {
    const float4 a = ttexel<WRAP>(below, lw, lh, 2 * s, 2 * t), b = ttexel<WRAP>(below, lw, lh, 2 * s + 1, 2 * t);
    const float4 c = ttexel<WRAP>(below, lw, lh, 2 * s, 2 * t + 1), d = ttexel<WRAP>(below, lw, lh, 2 * s + 1, 2 * t + 1);
    return make_float4(.25f * (a.x + b.x + c.x + d.x), .25f * (a.y + b.y + c.y + d.y), .25f * (a.z + b.z + c.z + d.z), 0.f);
}

// below: lw x lh -> lvl: sres x tres = max(1, lw / 2) x max(1, lh / 2)
template <int WRAP>
static __global__ void __launch_bounds__(kB) k_tex_pyramid(const float4 *__restrict__ below, int lw, int lh, int sres, int tres, float4 *__restrict__ lvl) {
    const long long n = (long long)sres * tres;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / sres), s = (int)(i - (long long)t * sres);
        lvl[i] = tbox<WRAP>(below, lw, lh, s, t);
    }
}

// One block.  below: the lw x lh level (global memory) under the first level to build, whose sides are at most kTailSide; out: where that
// level starts -- the n_build levels follow each other without padding, as the packed buffer holds them.  The first level is read from
// global memory, every later one from the copy of its predecessor that the step before left in LDS.
template <int WRAP>
static __global__ void __launch_bounds__(kB) k_tex_pyramid_tail(const float4 *__restrict__ below, int lw, int lh, int n_build, float4 *__restrict__ out) {
    __shared__ float4 stage[2][kTailSide * kTailSide];
    const float4 *src = below;
    int cur = 0;
    for (int l = 0; l < n_build; ++l) {
        const int sres = max(1, lw / 2), tres = max(1, lh / 2), n = sres * tres;   // (n <= kTailSide^2: the host starts the tail there)
        for (int i = threadIdx.x; i < n; i += kB) {
            const int t = i / sres, s = i - t * sres;
            const float4 v = tbox<WRAP>(src, lw, lh, s, t);
            stage[cur][i] = v;
            out[i] = v;
        }
        __syncthreads();   // (one barrier per level: the next step reads stage[cur] and writes the other half, which nobody reads any more)
        src = stage[cur];
        cur ^= 1;
        out += n; lw = sres; lh = tres;
    }
}

}  // namespace texb
}  // namespace gnxr
