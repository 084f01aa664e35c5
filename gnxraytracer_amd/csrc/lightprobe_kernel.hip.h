// lightprobe_kernel.hip.h -- light probes: incident radiance at points in free space, projected on the nine real spherical harmonics of
// bands 0 to 2 (api_lightprobe.hip.h; the definition, operation by operation: include/gnxr.h, "Light probes").
//   k_lightprobe_rays        (position, pixel, sample) -> uniformly distributed ray over the sphere + sample record
//   k_lightprobe_bake_rays   the same for a sub-batch of a bake, in probe-major order
//   k_sh_project             the hot kernel: a wave per probe, 27 butterfly sums per block of 64 samples, blocks added in order
//   k_lightprobe_finish      sums -> coefficients: (sum * 4 pi) / spp
//   k_sh_irradiance          coefficients + normal -> irradiance
// Every fp32 operation is written once and compiled unfused.
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// ---- the basis ----

// Y_0 .. Y_8 at the direction (x, y, z): the real spherical harmonics of bands 0 to 2 in the order (l, m) = (0,0), (1,-1), (1,0), (1,1),
// (2,-2), (2,-1), (2,0), (2,1), (2,2), with the constants rounded as the header writes them
GX_DEV void sh_basis(float x, float y, float z, float *Y) {
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * (x * y);
    Y[5] = 1.092548f * (y * z);
    Y[6] = 0.315392f * ((3.f * (z * z)) - 1.f);
    Y[7] = 1.092548f * (x * z);
    Y[8] = 0.546274f * ((x * x) - (y * y));
}

// ---- probe rays ----

// core/Sampling.cpp:72-77
GX_DEV V3 uniform_sample_sphere(float u0, float u1) {
    const float z = 1.f - 2.f * u0;
    const float r = gx_sqrt(fmaxf(0.f, 1.f - z * z));
    const float phi = (2.f * GX_PI) * u1;
    float sp, cp;
    gx_sincos(phi, &sp, &cp);
    return V3(r * cp, r * sp, z);
}

// the direction of sample s of pixel (px, py): Halton dimensions 3 and 4 (pLens: the pair Li never draws), as surface_ray takes them
GX_DEV V3 lightprobe_direction(const DSamplerTables &st, int px, int py, int s) {
    const uint32_t index = halton_pixel_offset(st.h, px, py) + (uint32_t)s * (uint32_t)st.h.stride;
    const float u0 = halton_sample(st, index, 3), u1 = halton_sample(st, index, 4);
    return uniform_sample_sphere(u0, u1);
}

GX_DEV bool lightprobe_finite(float x, float y, float z) { return fabsf(x) < GX_INF && fabsf(y) < GX_INF && fabsf(z) < GX_INF; }   // (NaN fails)

// gnxr_lightprobe_rays_device: one record per lane.  A record with a non-finite position, a pixel outside the image or s < 0 is written
// as zeros and flagged: *bad keeps ~index of the first one (k_camera_rays' convention).
static __global__ void __launch_bounds__(kBlock) k_lightprobe_rays(DSamplerTables st, int W, int H, const float *__restrict__ pos, const int *__restrict__ px,
                                                                   const int *__restrict__ py, const int *__restrict__ s, long long n, int medium,
                                                                   float4 *__restrict__ rays, int4 *__restrict__ samples, unsigned long long *bad) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = px[i], y = py[i], k = s[i];
        const float ox = pos[3 * (size_t)i], oy = pos[3 * (size_t)i + 1], oz = pos[3 * (size_t)i + 2];
        float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro;
        int4 rec = make_int4(0, 0, 0, 0);
        if (lightprobe_finite(ox, oy, oz) && x >= 0 && x < W && y >= 0 && y < H && k >= 0) {
            const V3 d = lightprobe_direction(st, x, y, k);
            ro = make_float4(ox, oy, oz, GX_INF);
            rd = make_float4(d.x, d.y, d.z, 0.f);
            rec = make_int4(x, y, k, medium);
        } else {
            atomicMax(bad, ~(unsigned long long)i);
        }
        rays[2 * (size_t)i] = ro;
        rays[2 * (size_t)i + 1] = rd;
        samples[i] = rec;
    }
}

// A sub-batch of a bake: samples [s0, s0 + ns) of the probes [k0, k0 + nk), probe-major: record j is sample s0 + j % ns of probe
// k0 + j / ns, which is pixel (k % W, k / W).  A probe with a non-finite position sends its rays from the origin (k_lightprobe_finish
// zeroes its coefficients): nothing non-finite reaches the traversal.
static __global__ void __launch_bounds__(kBlock) k_lightprobe_bake_rays(DSamplerTables st, int W, const float *__restrict__ pos, int k0, int s0, int ns, long long n,
                                                                        int medium, float4 *__restrict__ rays, int4 *__restrict__ samples) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const int k = k0 + (int)(j / ns), s = s0 + (int)(j % ns);
        const int x = k % W, y = k / W;
        float ox = pos[3 * (size_t)k], oy = pos[3 * (size_t)k + 1], oz = pos[3 * (size_t)k + 2];
        if (!lightprobe_finite(ox, oy, oz)) ox = oy = oz = 0.f;
        const V3 d = lightprobe_direction(st, x, y, s);
        rays[2 * (size_t)j] = make_float4(ox, oy, oz, GX_INF);
        rays[2 * (size_t)j + 1] = make_float4(d.x, d.y, d.z, 0.f);
        samples[j] = make_int4(x, y, s, medium);
    }
}

// ---- projection ----

// One step of the butterfly: v[l] + v[l ^ M] in every lane of the wave, without a trip through the LDS.
//   M = 32, 16   v_permlane32_swap / v_permlane16_swap of the value with a copy of itself leave the two halves (the two rows of a pair)
//                side by side in two registers: one swap and one addition.  Lane l adds (lower, upper), which is v[l] + v[l ^ M] for the
//                lower lanes and v[l ^ M] + v[l] for the upper ones: the same bits, fp32 addition being commutative.
//   M = 8, 4     row_ror:M rotates within the 16 lanes of a row.  After the steps above it the value has period 2 * M over the lanes, so
//                the lane M places on holds what lane l ^ M holds.
//   M = 2, 1     quad_perm [2,3,0,1] and [1,0,3,2]: the exchange itself.
// The DPP forms fold into the addition (v_add_f32_dpp): one VALU instruction per step.
template <int M>
GX_DEV float sh_xor_add(float v) {
    const unsigned int u = __float_as_uint(v);
    if constexpr (M == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else {
        constexpr int ctrl = M == 8 ? 0x128 : M == 4 ? 0x124 : M == 2 ? 0x4e : 0xb1;
        return v + __uint_as_float(__builtin_amdgcn_update_dpp(0u, u, ctrl, 0xf, 0xf, false));
    }
}
// the sum of a block of 64 terms in the defined order; every lane returns the same bits
GX_DEV float sh_block_sum(float v) {
    v = sh_xor_add<32>(v);
    v = sh_xor_add<16>(v);
    v = sh_xor_add<8>(v);
    v = sh_xor_add<4>(v);
    v = sh_xor_add<2>(v);
    return sh_xor_add<1>(v);
}

// gnxr_sh_project_device.  A wave per probe (grid-stride over the probes); per block of 64 consecutive samples every lane loads one L and
// one direction (64 consecutive float4 of L, 64 consecutive 32-byte ray records: coalesced), forms its 27 terms and the wave reduces them;
// the block sums are added to 27 accumulators that every lane holds, in block order.  The next block's loads are issued before the current
// block is reduced.  All 64 lanes stay active through the reductions: a lane past n_samples carries +0.0f.
static __global__ void __launch_bounds__(kBlock) k_sh_project(const float4 *__restrict__ rays, const float4 *__restrict__ L, int n_probes, long long n_samples, int cont,
                                                              float4 *__restrict__ sh_sum) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k = wave; k < n_probes; k += n_waves) {
        float acc[27];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cont) a = sh_sum[9 * (size_t)k + j];
            acc[3 * j] = a.x; acc[3 * j + 1] = a.y; acc[3 * j + 2] = a.z;
        }
        const size_t base = (size_t)k * (size_t)n_samples;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 l = zero, d = zero;
        if (lane < n_samples) { l = L[base + lane]; d = rays[2 * (base + lane) + 1]; }
        for (long long s0 = 0; s0 < n_samples; s0 += 64) {
            const bool live = s0 + lane < n_samples;
            const float4 lc = l, dc = d;
            const long long next = s0 + 64 + lane;
            if (next < n_samples) { l = L[base + next]; d = rays[2 * (base + next) + 1]; }
            float Y[9];
            sh_basis(dc.x, dc.y, dc.z, Y);
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                acc[3 * j] = acc[3 * j] + sh_block_sum(live ? lc.x * Y[j] : 0.f);
                acc[3 * j + 1] = acc[3 * j + 1] + sh_block_sum(live ? lc.y * Y[j] : 0.f);
                acc[3 * j + 2] = acc[3 * j + 2] + sh_block_sum(live ? lc.z * Y[j] : 0.f);
            }
        }
        float4 out = zero;
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (lane == j) out = make_float4(acc[3 * j], acc[3 * j + 1], acc[3 * j + 2], 0.f);
        if (lane < 9) sh_sum[9 * (size_t)k + lane] = out;
    }
}

// sums -> coefficients of a bake: ((sum * 4 pi) / spp, 0); a probe with a non-finite position gets zeros
static __global__ void __launch_bounds__(kBlock) k_lightprobe_finish(const float *__restrict__ pos, long long n_slots, int spp, float4 *__restrict__ sh) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (long long)gridDim.x * blockDim.x) {
        const size_t k = (size_t)(i / 9);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lightprobe_finite(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2])) {
            const float4 a = sh[i];
            v = make_float4((a.x * 12.566370614359172f) / (float)spp, (a.y * 12.566370614359172f) / (float)spp, (a.z * 12.566370614359172f) / (float)spp, 0.f);
        }
        sh[i] = v;
    }
}

// ---- evaluation ----

// gnxr_sh_irradiance_device: one record per lane.  A probe index out of range is written as zeros and flagged in *bad (~index of the first).
static __global__ void __launch_bounds__(kBlock) k_sh_irradiance(const float4 *__restrict__ sh, int n_probes, const int *__restrict__ probe, const float *__restrict__ normals,
                                                                 long long n, float4 *__restrict__ E, unsigned long long *bad) {
    const float A0 = 3.14159265f, A1 = 2.09439510f, A2 = 0.78539816f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int k = probe[i];
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k >= 0 && k < n_probes) {
            float Y[9];
            sh_basis(normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2], Y);
            const float4 *c = sh + 9 * (size_t)k;
            const float4 c0 = c[0];
            e = make_float4(A0 * (c0.x * Y[0]), A0 * (c0.y * Y[0]), A0 * (c0.z * Y[0]), 1.f);
#pragma unroll
            for (int j = 1; j < 9; ++j) {
                const float A = j < 4 ? A1 : A2;
                const float4 cj = c[j];
                e.x = e.x + A * (cj.x * Y[j]);
                e.y = e.y + A * (cj.y * Y[j]);
                e.z = e.z + A * (cj.z * Y[j]);
            }
        } else {
            atomicMax(bad, ~(unsigned long long)i);
        }
        E[i] = e;
    }
}

}  // namespace gnxr
