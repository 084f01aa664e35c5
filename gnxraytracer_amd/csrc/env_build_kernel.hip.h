// env_build_kernel.hip.h -- gnxr_scene_update_environment on the device: the tables of the InfiniteAreaLight built from a raw lat-long
// map, step by step what build_env (scene_compile.cpp) builds on the host for gnxr_scene_create.
//
//   k_env_texels       texel = r * Sqrt(r), r = L * rgb, with the row flip (InfiniteAreaLight.cpp:33-41), as float4 (rgb_, w lane 0)
//   k_env_resample_s   MIPMap's Lanczos resample along s (MIPMap.h:93-146, wrap = Repeat): ry x px, no clamp
//   k_env_resample_t   ... along t: px x py, clamped to [0, inf)
//   k_env_pyramid      one level of the box-filter pyramid (MIPMap.h:147-170) from the level below; read by InfiniteAreaLight::Power only
//   k_env_image        the 2rx x 2ry sampling image: level-0 bilinear lookup, luminance, times sin(theta) (InfiniteAreaLight.cpp:65-80)
//   k_env_dist1d       Distribution1D per row (Sampling.h:22-35): the conditional rows, and over their integrals the marginal
//   k_env_guide        the FindInterval guide tables over the cdfs (build_env's `upper`)
//
// Every result is bit for bit the host's: each kernel restates its loop of build_env with the same fp32 operations in the same order.
// The translation unit is compiled with -ffp-contract=off, as the host object of scene_compile.cpp is (nothing in build_env is fused
// there: x86-64 without FMA), `/` is the IEEE division and gx_sqrt / gx_sin are the pinned restatements of sqrtf / glibc's sinf
// (device_math.h).  The Lanczos weights depend on the sizes only: the host's resample_weights computes them and they are uploaded.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "gnxr_device_types.h"

namespace gnxr {
namespace envb {

constexpr int kB = 256;          // threads per block
constexpr int kChunk = 2048;     // floats of a Distribution1D row held in LDS at a time (8 KB)

struct DResampleWeight { int32_t first; float w[4]; };   // resample_weights' record (MIPMap.h:41-59)

__device__ __forceinline__ int emodi(int a, int b) { int r = a - (a / b) * b; return r < 0 ? r + b : r; }

// rgb: w x h x 3 as decoded from .hdr; tex: w x h float4
static __global__ void __launch_bounds__(kB) k_env_texels(const float *__restrict__ rgb, int w, int h, int flip_y, float le0, float le1, float le2, float4 *__restrict__ tex) {
    const long long n = (long long)w * h;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / w), i0 = (int)(i - (long long)j * w);
        const long long src = (long long)(flip_y ? h - 1 - j : j) * w + i0;
        const float r0 = le0 * rgb[3 * src], r1 = le1 * rgb[3 * src + 1], r2 = le2 * rgb[3 * src + 2];
        tex[i] = make_float4(r0 * gx_sqrt(r0), r1 * gx_sqrt(r1), r2 * gx_sqrt(r2), 0.f);
    }
}

// tex: ry rows of rx texels -> res: ry rows of px.  Four taps accumulated from 0.f in tap order.
static __global__ void __launch_bounds__(kB) k_env_resample_s(const float4 *__restrict__ tex, int rx, int ry, int px, const DResampleWeight *__restrict__ sw,
                                                             float4 *__restrict__ res) {
    const long long n = (long long)ry * px;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / px), s = (int)(i - (long long)t * px);
        const DResampleWeight *wt = sw + s;
        const int first = wt->first;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < 4; ++j) {
            const float4 v = tex[(long long)t * rx + emodi(first + j, rx)];
            const float wj = wt->w[j];
            a0 += wj * v.x; a1 += wj * v.y; a2 += wj * v.z;
        }
        res[i] = make_float4(a0, a1, a2, 0.f);
    }
}

__device__ __forceinline__ float eclamp0(float v) { return v < 0.f ? 0.f : (v > INFINITY ? INFINITY : v); }   // clampf(v, 0, INFINITY)

// res: ry rows of px -> out: py rows of px, clamped
static __global__ void __launch_bounds__(kB) k_env_resample_t(const float4 *__restrict__ res, int px, int ry, int py, const DResampleWeight *__restrict__ tw,
                                                             float4 *__restrict__ out) {
    const long long n = (long long)py * px;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / px), s = (int)(i - (long long)t * px);
        const DResampleWeight *wt = tw + t;
        const int first = wt->first;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < 4; ++j) {
            const float4 v = res[(long long)emodi(first + j, ry) * px + s];
            const float wj = wt->w[j];
            a0 += wj * v.x; a1 += wj * v.y; a2 += wj * v.z;
        }
        out[i] = make_float4(eclamp0(a0), eclamp0(a1), eclamp0(a2), 0.f);
    }
}

// below: lw x lh -> lvl: sres x tres = max(1, lw / 2) x max(1, lh / 2); the 1-wide levels wrap (MIPMap::Texel, Repeat)
static __global__ void __launch_bounds__(kB) k_env_pyramid(const float4 *__restrict__ below, int lw, int lh, int sres, int tres, float4 *__restrict__ lvl) {
    const long long n = (long long)sres * tres;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / sres), s = (int)(i - (long long)t * sres);
        const int sa = emodi(2 * s, lw), sb = emodi(2 * s + 1, lw), ta = emodi(2 * t, lh), tb = emodi(2 * t + 1, lh);
        const float4 a = below[(long long)ta * lw + sa], b = below[(long long)ta * lw + sb], c = below[(long long)tb * lw + sa], d = below[(long long)tb * lw + sb];
        lvl[i] = make_float4(.25f * (a.x + b.x + c.x + d.x), .25f * (a.y + b.y + c.y + d.y), .25f * (a.z + b.z + c.z + d.z), 0.f);
    }
}

// tex: rx x ry -> img: 2rx x 2ry
static __global__ void __launch_bounds__(kB) k_env_image(const float4 *__restrict__ tex, int rx, int ry, float *__restrict__ img) {
    const int W2 = 2 * rx, H2 = 2 * ry;
    const long long n = (long long)W2 * H2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(i / W2), u = (int)(i - (long long)v * W2);
        const float vp = (v + .5f) / (float)H2;
        const float sinTheta = gx_sin(GX_PI * (v + .5f) / H2);
        const float up = (u + .5f) / (float)W2;
        const float s = up * rx - 0.5f, t = vp * ry - 0.5f;
        const int s0 = (int)floorf(s), t0 = (int)floorf(t);
        const float ds = s - s0, dt = t - t0;
        const int sa = emodi(s0, rx), sb = emodi(s0 + 1, rx), ta = emodi(t0, ry), tb = emodi(t0 + 1, ry);
        const float4 t00 = tex[(long long)ta * rx + sa], t01 = tex[(long long)tb * rx + sa], t10 = tex[(long long)ta * rx + sb], t11 = tex[(long long)tb * rx + sb];
        const float r = (1 - ds) * (1 - dt) * t00.x + (1 - ds) * dt * t01.x + ds * (1 - dt) * t10.x + ds * dt * t11.x;
        const float g = (1 - ds) * (1 - dt) * t00.y + (1 - ds) * dt * t01.y + ds * (1 - dt) * t10.y + ds * dt * t11.y;
        const float b = (1 - ds) * (1 - dt) * t00.z + (1 - ds) * dt * t01.z + ds * (1 - dt) * t10.z + ds * dt * t11.z;
        float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
        y *= sinTheta;
        img[i] = y;
    }
}

// Distribution1D of `n_rows` rows of n function values: cdf (n + 1 per row) and funcInt (one per row).  One block per row.
// cdf[i] = cdf[i - 1] + f[i - 1] / n is a chain of dependent additions and runs in index order on ONE lane; the quotients before it and
// the normalisation after it are elementwise and belong to all lanes.  The row passes through LDS in chunks of kChunk: all lanes form
// the quotients, lane 0 turns them into running sums (four per ds_read_b128 / ds_write_b128), all lanes store them (coalesced).  A
// second pass normalises: every lane rereads exactly the entries it stored itself.
static __global__ void __launch_bounds__(kB) k_env_dist1d(const float *__restrict__ func, int n, int n_rows, float *__restrict__ cdf, float *__restrict__ func_int) {
    __shared__ float4 q4[kChunk / 4];
    __shared__ float carry;
    float *q = reinterpret_cast<float *>(q4);
    const int tid = threadIdx.x;
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const float *f = func + (long long)row * n;
        float *c = cdf + (long long)row * (n + 1);
        if (tid == 0) carry = 0.f;
        for (int base = 0; base < n; base += kChunk) {
            const int m = min(kChunk, n - base);
            for (int i = tid; i < ((m + 3) & ~3); i += kB) q[i] = i < m ? f[base + i] / n : 0.f;   // (whole groups of four: the tail is zero)
            __syncthreads();
            if (tid == 0) {
                float a = carry;
                const int m4 = (m + 3) / 4;
                for (int k = 0; k < m4; ++k) {   // (entries past m in the last group are computed and never stored)
                    float4 v = q4[k];
                    a = a + v.x; v.x = a;
                    a = a + v.y; v.y = a;
                    a = a + v.z; v.z = a;
                    a = a + v.w; v.w = a;
                    q4[k] = v;
                }
                carry = q[m - 1];
            }
            __syncthreads();
            for (int i = tid; i < m; i += kB) c[base + i + 1] = q[i];
            __syncthreads();
        }
        const float fi = carry;   // cdf[n]
        if (tid == 0) { c[0] = 0.f; func_int[row] = fi; }
        if (fi == 0)
            for (int i = tid; i < n; i += kB) c[i + 1] = float(i + 1) / float(n);
        else
            for (int i = tid; i < n; i += kB) c[i + 1] = c[i + 1] / fi;
        __syncthreads();   // (carry is rewritten for the next row)
    }
}

// build_env's `upper`: the number of cdf values <= u (FindInterval's predicate)
__device__ __forceinline__ int eupper(const float *__restrict__ cdf, int size, float u) {
    int n = 0, len = size;
    while (len > 0) {
        const int half = len >> 1;
        if (cdf[n + half] <= u) { n += half + 1; len -= half + 1; } else len = half;
    }
    return n;
}

// guide: n_rows x (G + 1) entries over cdf rows of `size` values; the last bucket is `size`
static __global__ void __launch_bounds__(kB) k_env_guide(const float *__restrict__ cdf, int size, int n_rows, int G, uint16_t *__restrict__ guide) {
    const long long n = (long long)n_rows * (G + 1);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(i / (G + 1)), b = (int)(i - (long long)v * (G + 1));
        guide[i] = b == G ? (uint16_t)size : (uint16_t)eupper(cdf + (long long)v * size, size, (float)b / G);
    }
}

}  // namespace envb
}  // namespace gnxr
