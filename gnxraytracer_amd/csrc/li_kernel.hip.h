// li_kernel.hip.h -- SamplerIntegrator::Li for caller-supplied rays (gnxr_li_device).
//
// Integrator::Render is a camera loop around Li (core/Integrator.cpp:256-293).  Only two stages of the wavefront loops depend on the
// image: k_raygen (slot -> pixel, sample -> camera ray) and k_resolve / k_finish (colObj += Li in sample order, box average).  These two
// kernels take their place for a batch of caller rays; tracing, shading, NEE and the media stages run unchanged on the paths they start.
// Both are plain streaming kernels: one ray and one sample record per lane, no LDS, no scratch.
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// gnxr_li_sample {px, py, s, medium}: pixel in [0, W) x [0, H), sample in [0, spp), medium in [-1, n_media)
GX_DEV bool li_sample_ok(const DRender &r, int4 rec, int n_media) {
    return rec.x >= 0 && rec.x < r.W && rec.y >= 0 && rec.y < r.H && rec.z >= 0 && rec.z < r.spp && rec.w >= -1 && rec.w < n_media;
}

// The path state k_raygen writes, for rays [first, first + n_paths) of the batch in slots [0, n_paths) of `pa`: the ray is the caller's
// (tMax bounds the first Intersect) and the sampler stands where GetCameraSample leaves it -- pixel (px, py), sample s, dimension 5, which
// camera_ray returns for every camera.  medium_keys (VolPath): bit 1 set for a ray that starts inside a medium, the key of the compaction
// that lists them.  A record out of range is flagged (ctr->li_bad keeps ~index of the first such ray of the call: atomicMax of the
// complement over a zeroed counter) and its path ends at once: a zero-length ray that can hit nothing; k_store_li writes (0, 0, 0, 0) for it.
static __global__ void __launch_bounds__(kBlock) k_raygen_rays(DScene sc, DRender r, PathArrays pa, const float4 *__restrict__ rays, const int4 *__restrict__ samples,
                                                               int n_paths, int n_media, unsigned char *__restrict__ medium_keys, Counters *ctr, long long first) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_paths; j += gridDim.x * blockDim.x) {
        const float4 o4 = rays[2 * (size_t)j], d4 = rays[2 * (size_t)j + 1];
        const int4 rec = samples[j];
        const bool ok = li_sample_ok(r, rec, n_media);
        float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = make_float4(0.f, 0.f, 1.f, __int_as_float(-1));
        uint32_t index = 0;
        if (ok) {
            index = halton_pixel_offset(sc.st.h, rec.x, rec.y) + (uint32_t)rec.z * (uint32_t)sc.st.h.stride;
            ro = o4;
            rd = make_float4(d4.x, d4.y, d4.z, __int_as_float(rec.w));
        } else {
            atomicMax(&ctr->li_bad, ~(unsigned long long)(first + j));
        }
        pa.ray_o[(size_t)j * kRS] = ro;
        pa.ray_d[(size_t)j * kRS] = rd;
        pa.beta[(size_t)j * kRS] = make_float4(1.f, 1.f, 1.f, 1.f);
        pa.L[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        pa.store_meta(j, index, 5u);
        if (medium_keys) medium_keys[j] = (ok && rec.w >= 0) ? 2 : 0;
    }
}

// The counterpart of k_resolve: every ray owns its result, so a finished chunk is copied out as it is, with no ordered reduction.
// L: the chunk's radiance by slot (VolPath: vol_Lout, where a path's result stays at its original slot).
static __global__ void __launch_bounds__(kBlock) k_store_li(const float4 *__restrict__ L, const int4 *__restrict__ samples, DRender r, int n_media, int n_paths,
                                                            float4 *__restrict__ out) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_paths; j += gridDim.x * blockDim.x) {
        const float4 l = L[j];
        out[j] = li_sample_ok(r, samples[j], n_media) ? make_float4(l.x, l.y, l.z, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace gnxr
