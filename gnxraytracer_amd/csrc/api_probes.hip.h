// api_probes.hip.h -- the two peak-rate probes (gnxr_probe_valu_peak / gnxr_probe_gather_peak).  Part of api.hip's translation unit.
#pragma once

namespace {
// Issue-rate probe: 8 independent v_fma_f32 chains per lane with all three operands in vector registers, no memory traffic; with 8 waves
// on every SIMD the loop is bound by VALU issue alone.  Inline asm: the compiler would otherwise keep `a` and `b` in scalar registers (a
// VOP3 with two scalar operands issues at half the rate: 578 instead of ~900 G wave-instructions/s) or pack pairs of chains into
// v_pk_fma_f32 (half the instructions at half the rate).  tools/probes/valu_probe.hip has the same loop for every instruction kind the
// kernels use: add / sub / mul / fma / logic issue in 2 cycles per wave64, min / max / compare / shift / integer multiply / conversion /
// packed and fp64 arithmetic in 4, rcp / sqrt in 8 (profiles/r02_valu_probe.log).
__global__ void __launch_bounds__(256) k_valu_peak(float *out, int iters, float a_in, float b_in) {
    float x0 = threadIdx.x, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
    float a = a_in, b = b_in;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("v_mov_b32 %0, %0" : "+v"(a));
    asm volatile("v_mov_b32 %0, %0" : "+v"(b));
#define GX_FMA1(x) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x) : "v"(a), "v"(b));
#else
#define GX_FMA1(x) x = __builtin_fmaf(x, a, b);
#endif
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { GX_FMA1(x0) GX_FMA1(x1) GX_FMA1(x2) GX_FMA1(x3) GX_FMA1(x4) GX_FMA1(x5) GX_FMA1(x6) GX_FMA1(x7) }
    }
#undef GX_FMA1
    out[blockIdx.x * blockDim.x + threadIdx.x] = ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7));
}
// Gather-rate probe: every lane reads the 8 dwordx4 of its own pseudo-random 128-byte record (a BVH node visit without the arithmetic),
// the next record depends on what was read (a traversal's dependent chain).
__global__ void __launch_bounds__(256) k_gather_peak(const float4 *__restrict__ tab, unsigned nrec, int iters, float *out) {
    unsigned idx = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        idx = idx * 1664525u + 1013904223u;
        const float4 *p = tab + (size_t)((idx >> 8) % nrec) * 8;
        const float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5], g = p[6], h = p[7];
        acc += a.x + b.y + c.z + d.w + e.x + f.y + g.z + h.w;
        idx ^= __float_as_uint(acc) & 1u;
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}
}  // namespace

extern "C" {

int gnxr_probe_gather_peak(double *giga_lane_loads_per_s) {
    if (!giga_lane_loads_per_s) { set_error("null argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    const unsigned nrec = 8u * 1024 * 1024 / 128;
    const int blocks = g_num_cus * 5, iters = 1000;
    DevBuf<float4> tab;
    DevBuf<float> out;
    if ((rc = tab.alloc((size_t)nrec * 8)) != GNXR_OK || (rc = out.alloc((size_t)blocks * 256)) != GNXR_OK) return rc;
    HIP_TRY(hipMemset(tab.p, 0, (size_t)nrec * 128));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    double best = 0;
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_gather_peak, dim3(blocks), dim3(256), 0, 0, (const float4 *)tab.p, nrec, iters, out.p);
        (void)hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) break;
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0) best = std::max(best, (double)blocks * 256 * (double)iters * 8 / (ms * 1e-3) / 1e9);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIP_TRY(hipGetLastError());
    *giga_lane_loads_per_s = best;
    return GNXR_OK;
}

int gnxr_probe_valu_peak(double *giga_wave_insts_per_s) {
    if (!giga_wave_insts_per_s) { set_error("null argument"); return GNXR_ERR_INVALID; }
    int rc = ensure_device();
    if (rc) return rc;
    const int blocks = g_num_cus * 8, iters = 4096;   // 8 blocks x 4 waves per CU = 8 waves per SIMD
    DevBuf<float> out;
    if ((rc = out.alloc((size_t)blocks * 256)) != GNXR_OK) return rc;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    double best = 0;
    for (int rep = 0; rep < 4; ++rep) {   // the first launch warms the clocks up
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_valu_peak, dim3(blocks), dim3(256), 0, 0, out.p, iters, 1.0000001f, 1e-9f);
        (void)hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) break;
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0)
            best = std::max(best, (double)blocks * 4 /* waves */ * (double)iters * 64 /* FMAs per iteration */ / (ms * 1e-3) / 1e9);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIP_TRY(hipGetLastError());
    *giga_wave_insts_per_s = best;
    return GNXR_OK;
}

}  // extern "C"
