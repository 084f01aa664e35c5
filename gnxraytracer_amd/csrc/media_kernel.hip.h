// media_kernel.hip.h -- gnxr_scene_update_media on the device: one density grid copied into the scene's grid buffer and its maximum found
// in the same pass, so a grid is read once (4 bytes in and 4 bytes out per voxel; one float per grid goes back to the host).
//
//   k_media_grid   dst[0 .. n) = src[0 .. n), *max_out = the maximum GridDensityMedium.h:28-31 / compile_scene computes
//
// That maximum is the fold  m = 0; for k: m = std::max(m, d[k]),  i.e.  m = (m < d[k]) ? d[k] : m  from +0.  The comparison is false
// for a NaN and for (+0, -0), so the fold skips NaNs and never yields a negative value or -0; over what is left it is an ordinary
// maximum and does not depend on the order: every partial here starts from +0 and partials are combined with the same `a < b ? b : a`
// (not fmaxf, which may return -0 for (+0, -0): 1 / -0 is -inf where the reference has +inf).  A partial is therefore the bit pattern
// of a non-negative, non-NaN float, and those patterns order as signed integers do: the block partials are combined by an integer
// atomicMax on the bits, which is exact.  *max_out must hold +0 (all bits clear) when the kernel starts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gnxr {
namespace mediab {

constexpr int kB = 256;   // kBlock: four waves of 64

typedef float float4a4 __attribute__((ext_vector_type(4), aligned(4)));   // a dwordx4 at a 4-byte aligned address

__device__ __forceinline__ float fold_max(float m, float d) { return (m < d) ? d : m; }   // std::max(m, d)

// src is 4-byte aligned in general (density + density_offset): a scalar head up to its first 16-byte boundary, 16-byte loads from
// there, a scalar tail.  dst follows with the same head, so its stores are 16-byte aligned exactly when src and dst agree modulo 16.
static __global__ void __launch_bounds__(kB) k_media_grid(const float *__restrict__ src, float *__restrict__ dst, int64_t n, float *__restrict__ max_out) {
    const int64_t tid = (int64_t)blockIdx.x * kB + threadIdx.x, stride = (int64_t)gridDim.x * kB;
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const int64_t n4 = (n - head) >> 2, tail = head + 4 * n4;
    float m = 0.f;
    if (tid < head) { const float v = src[tid]; dst[tid] = v; m = fold_max(m, v); }
    const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(src + head);
    float *__restrict__ d4 = dst + head;
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 v = s4[i];
        float4a4 o;
        o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
        *reinterpret_cast<float4a4 *>(d4 + 4 * i) = o;
        m = fold_max(fold_max(fold_max(fold_max(m, v.x), v.y), v.z), v.w);
    }
    if (tid < n - tail) { const float v = src[tail + tid]; dst[tail + tid] = v; m = fold_max(m, v); }
    // the wave, then the block through LDS, then one atomic per block
    for (int o = 32; o > 0; o >>= 1) m = fold_max(m, __shfl_xor(m, o));
    __shared__ float part[kB / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kB / 64; ++w) m = fold_max(m, part[w]);
        if (m > 0.f) atomicMax(reinterpret_cast<int *>(max_out), __float_as_int(m));
    }
}

}  // namespace mediab
}  // namespace gnxr
