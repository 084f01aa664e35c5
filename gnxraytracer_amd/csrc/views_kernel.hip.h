// views_kernel.hip.h -- many cameras in one render (gnxr_render_views_device) and camera rays on device memory (gnxr_camera_rays_device).
//
// Pixels are independent and every view of a call uses the same HaltonSampler(spp, [0, W) x [0, H)), so V views are ONE path population
// of V * W * H pixels per sample: the accumulator pixel of view v, pixel p is v * W * H + p, DRender::npix is V * W * H, and sub-pass
// sizing, queues, traversal, shading, k_resolve and k_finish (row y of the stacked image = view * H + py) work on it unchanged.  Only the
// kernels that read the camera need a view: they are the kernels of this file, which take the per-view DCamera records as a table in
// device memory.  The kernels of a single-camera render (k_raygen, k_whitted_init_diff) are not touched and DRender does not grow: a
// single camera pays neither the table load nor the view division.
#pragma once
#include "kernels.hip.h"
#include "whitted_kernel.hip.h"

namespace gnxr {

// accumulator pixel of a views render -> view and raster coordinates inside that view's image
GX_DEV void view_pixel(const DRender &r, int lp, int *view, int *px, int *py) {
    const int wh = r.W * r.H;
    const int v = lp / wh, p = lp - v * wh;
    const int y = p / r.W;
    *view = v; *px = p - y * r.W; *py = y;
}

// k_raygen for a views render: slot = sample j * npix + view * W * H + pixel.  The Halton index comes from the pixel inside its own image,
// the ray from cams[view] through the same camera_ray as k_raygen.  medium_keys (VolPath with views in different media): bit 1 set for a
// path that starts inside a medium, the key of the compaction that lists them (the route of k_raygen_rays, li_kernel.hip.h).
static __global__ void __launch_bounds__(kBlock) k_raygen_views(DScene sc, DRender r, const DCamera *__restrict__ cams, PathArrays pa, int n_paths, int s0,
                                                                unsigned char *__restrict__ medium_keys) {
    for (int slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n_paths; slot += gridDim.x * blockDim.x) {
        const int j = slot / r.npix;
        const int lp = slot - j * r.npix;
        int view, px, py;
        view_pixel(r, lp, &view, &px, &py);
        const DCamera cam = cams[view];
        uint32_t index = halton_pixel_offset(sc.st.h, px, py) + (uint32_t)(s0 + j) * (uint32_t)sc.st.h.stride;
        V3 o, d;
        float tMax;
        int dim;
        camera_ray(cam, sc.st, px, py, index, &o, &d, &tMax, &dim);
        pa.ray_o[(size_t)slot * kRS] = make_float4(o.x, o.y, o.z, tMax);
        pa.ray_d[(size_t)slot * kRS] = make_float4(d.x, d.y, d.z, __int_as_float(cam.medium));
        pa.beta[(size_t)slot * kRS] = make_float4(1.f, 1.f, 1.f, 1.f);
        pa.L[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        pa.store_meta(slot, index, (uint32_t)dim);
        if (medium_keys) medium_keys[slot] = cam.medium >= 0 ? 2 : 0;
    }
}

// k_whitted_init_diff for a views render: the offset rays of the view's camera (Whitted / DirectLighting on scenes with image textures
// store them once per path, so the shade kernels never read a camera)
static __global__ void __launch_bounds__(kBlock) k_whitted_init_diff_views(DScene sc, DRender r, const DCamera *__restrict__ cams, PathArrays pa, WhittedArrays wa,
                                                                           int n_paths) {
    for (int slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n_paths; slot += gridDim.x * blockDim.x) {
        int view, px, py;
        view_pixel(r, slot % r.npix, &view, &px, &py);
        const DCamera cam = cams[view];
        store_ray_diff(wa, (size_t)slot, camera_ray_diff(cam, sc.st, px, py, pa.meta[(size_t)slot * kRSm].x, r.spp));
    }
}

// gnxr_camera_rays_device: sample s[i] of pixel (px[i], py[i]) -> the gnxr_ray (o, +inf, d, 0) and the gnxr_li_sample {px, py, s, medium}
// that gnxr_li_device takes; one record per lane, two dwordx4 stores for the ray and one for the sample.  The ray comes from the same
// camera_ray as k_raygen's and the host probe's (k_camera_probe).  A record outside the image or with s < 0 is written as zeros and
// flagged: *bad keeps ~index of the first one (atomicMax of the complement over a zeroed word).
static __global__ void __launch_bounds__(kBlock) k_camera_rays(DSamplerTables st, DCamera cam, int W, int H, const int *__restrict__ px, const int *__restrict__ py,
                                                               const int *__restrict__ s, long long n, float4 *__restrict__ rays, int4 *__restrict__ samples,
                                                               unsigned long long *bad) {
    for (long long i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = px[i], y = py[i], k = s[i];
        float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro;
        int4 rec = make_int4(0, 0, 0, 0);
        if (x >= 0 && x < W && y >= 0 && y < H && k >= 0) {
            uint32_t index = halton_pixel_offset(st.h, x, y) + (uint32_t)k * (uint32_t)st.h.stride;
            V3 o, d;
            float tMax;
            int dim;
            camera_ray(cam, st, x, y, index, &o, &d, &tMax, &dim);
            ro = make_float4(o.x, o.y, o.z, GX_INF);
            rd = make_float4(d.x, d.y, d.z, 0.f);
            rec = make_int4(x, y, k, cam.medium);
        } else {
            atomicMax(bad, ~(unsigned long long)i);
        }
        rays[2 * (size_t)i] = ro;
        rays[2 * (size_t)i + 1] = rd;
        samples[i] = rec;
    }
}

}  // namespace gnxr
