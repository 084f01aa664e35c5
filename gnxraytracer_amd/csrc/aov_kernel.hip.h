// aov_kernel.hip.h -- first-hit feature buffers (gnxr_render_aov_device): depth, geometric and shading normals, albedo and ids per view.
//
// The views of a call are one population of V * W * H pixels, as in views_kernel.hip.h, cut into sub-passes of k samples of every pixel.
// A sub-pass is three launches:
//   k_aov_raygen   slot = sample j * npix + pixel: the camera ray of camera_ray() (the function k_raygen_views and k_camera_rays call) as a
//                  gnxr_ray record, 32 bytes, with the leaf code "nothing" (-1) in its pad word
//   k_trace4       the 4-wide walk in its closest-hit query form (query_kernel.hip.h), exactly as gnxr_trace_closest_device drives it.  The
//                  query form ignores a ray's pad word and writes one int per ray, gnxr_hit::prim of a 32-byte record: handed the address
//                  of ray 0's pad word as its result array, it leaves every ray's leaf code in that ray's own pad.  A record is read and
//                  later written by the one lane that traces it, so the 32 bytes of the ray are the whole state of a camera sample.
//   k_aov_resolve  one lane per pixel, looping over the pixel's k samples in order: the hit is rebuilt from the leaf code the way
//                  k_query_finish does (tri_hit_recompute / sphere_test, then hit_record), the shading normal comes from shade_hit_rebuild
//                  (what k_shade and k_bsdf_query call), the albedo from the scene's table (in LDS) or tex_evaluate without differentials,
//                  and everything is added to the pixel's running sums.  No per-sample feature record ever reaches memory.
// k_aov_finish divides the sums by spp and writes the caller's buffers, one dwordx4 per pixel and four-float channel.  The sample order is
// the loop order, there are no float atomics, so the results do not depend on k.
//
// k_aov_resolve is templated on the channels that need code of their own -- albedo (table, texture lookup), geometric normal (hit_record),
// shading normal (surface point) -- so that a depth / ids request compiles none of it; depth and ids are uniform branches on their pointers.
#pragma once
#include "query_kernel.hip.h"
#include "views_kernel.hip.h"

namespace gnxr {

enum : int { kAovAlbedo = 1, kAovNormal = 2, kAovShading = 4 };
constexpr int kAovLdsMaterials = 256;   // scenes with at most this many (internal) materials read the albedo table and the authored map from LDS: 5 KB

struct AovTables {
    const float4 *albedo;    // per authored material: gnxr_material_albedo's rgb, w = the bits of kd_texture (CompiledScene::aov_albedo)
    const int *authored;     // per internal material: the authored index (CompiledScene::material_authored)
    int n_authored, n_internal;
};
// running sums per pixel between sub-passes; a pointer is null when no requested channel needs it
struct AovAccum {
    float4 *albedo;   // albedo.rgb, coverage
    float4 *normal;   // n.xyz, depth
    float4 *shading;  // ns.xyz, 0
};
struct AovOut {
    float4 *albedo, *normal, *shading;
    float *depth;
    int2 *ids;
};

// rays[2 slot], rays[2 slot + 1] = (o.xyz, tMax), (d.xyz, leaf code -1) for slot = j * npix + pixel, sample s0 + j of the pixel's view
static __global__ void __launch_bounds__(kBlock) k_aov_raygen(DSamplerTables st, DRender r, const DCamera *__restrict__ cams, float4 *__restrict__ rays, long long n_paths, int s0) {
    for (long long slot = blockIdx.x * (long long)blockDim.x + threadIdx.x; slot < n_paths; slot += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(slot / r.npix);
        const int lp = (int)(slot - (long long)j * r.npix);
        int view, px, py;
        view_pixel(r, lp, &view, &px, &py);
        const DCamera cam = cams[view];
        const uint32_t index = halton_pixel_offset(st.h, px, py) + (uint32_t)(s0 + j) * (uint32_t)st.h.stride;
        V3 o, d;
        float tMax;
        int dim;
        camera_ray(cam, st, px, py, index, &o, &d, &tMax, &dim);
        rays[2 * (size_t)slot] = make_float4(o.x, o.y, o.z, tMax);
        rays[2 * (size_t)slot + 1] = make_float4(d.x, d.y, d.z, __int_as_float(-1));
    }
}

// M: kAovAlbedo | kAovNormal | kAovShading.  k: samples per pixel in `rays`; `first`: they start at the lowest sample of the call (ids).
template <int M>
__global__ void __launch_bounds__(kBlock) k_aov_resolve(DScene sc, AovTables at, const float4 *__restrict__ rays, int npix, int k, int first, AovAccum acc,
                                                        int want_depth, int2 *__restrict__ ids) {
    constexpr bool ALB = (M & kAovAlbedo) != 0, NRM = (M & kAovNormal) != 0, SHN = (M & kAovShading) != 0;
    __shared__ float4 s_albedo[ALB ? kAovLdsMaterials : 1];
    __shared__ int s_authored[kAovLdsMaterials];
    const bool lds = at.n_internal <= kAovLdsMaterials && at.n_authored <= kAovLdsMaterials;   // uniform
    if (lds && (ALB || ids)) {
        for (int i = threadIdx.x; i < at.n_internal; i += blockDim.x) s_authored[i] = at.authored[i];
        if (ALB) for (int i = threadIdx.x; i < at.n_authored; i += blockDim.x) s_albedo[i] = at.albedo[i];
        __syncthreads();
    }
    const bool sums = NRM || want_depth;
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < npix; lp += gridDim.x * blockDim.x) {
        float4 aA = make_float4(0.f, 0.f, 0.f, 0.f), aN = aA, aS = aA;
        if (ALB) aA = acc.albedo[lp];
        if (sums) aN = acc.normal[lp];
        if (SHN) aS = acc.shading[lp];
        for (int j = 0; j < k; ++j) {
            const size_t slot = (size_t)j * npix + lp;
            const float4 o4 = rays[2 * slot], d4 = rays[2 * slot + 1];
            const V3 ro(o4.x, o4.y, o4.z), rd(d4.x, d4.y, d4.z);
            const int code = __float_as_int(d4.w);   // a leaf-order triangle, -1 nothing, -2 - i sphere i
            // (t, b0, b1, b2) as k_query_finish recomputes them: the bits of gnxr_trace_closest_device
            TriHit h = {0.f, 0.f, 0.f, 0.f};
            V3 p0, p1, p2;
            if (code >= 0) {
                load_tri(sc.tris, code, &p0, &p1, &p2);
                tri_hit_recompute(p0, p1, p2, ro, rd, &h);
            } else if (code < -1) {
                (void)sphere_test(sc.spheres[-2 - code], ro, rd, o4.w, &h.t);
            }
            int mat = -1;   // internal material of the hit (-1: none, or a miss)
            if (ALB || ids) {
                if (code >= 0) mat = sc.tris[code].material;
                else if (code < -1) mat = sc.spheres[-2 - code].material;
            }
            if (ids && first && j == 0) {
                int prim = -1;
                if (code >= 0) prim = sc.tris[code].prim;
                else if (code < -1) prim = sc.spheres[-2 - code].prim;
                ids[lp] = make_int2(prim, mat >= 0 ? (lds ? s_authored[mat] : at.authored[mat]) : -1);
            }
            if (sums) {
                aN.w += h.t;
                if (NRM) {
                    const gnxr_hit rec = hit_record(sc, ro, rd, code, h);
                    aN.x += rec.n[0]; aN.y += rec.n[1]; aN.z += rec.n[2];
                }
            }
            if (SHN) {   // the interaction k_shade shades
                V3 q0, q1, q2;
                TriHit hs;
                SurfacePoint sp;
                int triMat = -1, triLight = -1;
                V3 ns(0.f, 0.f, 0.f);
                if (shade_hit_rebuild<true, true>(sc, sc.materials, code, ro, rd, o4.w, &q0, &q1, &q2, &hs, &triMat, &triLight, &sp, nullptr, nullptr)) ns = sp.ns;
                aS.x += ns.x; aS.y += ns.y; aS.z += ns.z;
            }
            if (ALB) {
                Spec a(0.f);
                if (mat >= 0) {
                    const int m = lds ? s_authored[mat] : at.authored[mat];
                    const float4 t = lds ? s_albedo[m] : at.albedo[m];
                    a = Spec(t.x, t.y, t.z);
                    const int tex = __float_as_int(t.w);
                    if (tex > 0 && code >= 0) {   // Kd is an ImageTexture: textured_material's lookup with the zero differentials of hasDifferentials == false
                        const DTexTables &tt = tex_tables(sc.materials);
                        float tu, tv;
                        V3 dpdu, dpdv;
                        tri_uv_frame(p0, p1, p2, h, tri_uvs(tt, code), &tu, &tv, &dpdu, &dpdv);
                        RayDiff none;
                        none.has = false;
                        const Spec e = tex_evaluate(tt, tex - 1, tu, tv, compute_differentials(none, V3(), V3(), dpdu, dpdv));
                        a = Spec(tex_clamp0(e.r), tex_clamp0(e.g), tex_clamp0(e.b));
                    }
                }
                aA.x += a.r; aA.y += a.g; aA.z += a.b;
                aA.w += code != -1 ? 1.f : 0.f;
            }
        }
        if (ALB) acc.albedo[lp] = aA;
        if (sums) acc.normal[lp] = aN;
        if (SHN) acc.shading[lp] = aS;
    }
}

// sums / samplesPerPixel, as k_finish divides the render's; pixel lp = view * W * H + x + y * W is the caller's layout already
static __global__ void __launch_bounds__(kBlock) k_aov_finish(AovAccum acc, AovOut out, int npix, int spp_i) {
    const float spp = (float)(long long)spp_i;
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < npix; lp += gridDim.x * blockDim.x) {
        if (out.albedo) { const float4 a = acc.albedo[lp]; out.albedo[lp] = make_float4(a.x / spp, a.y / spp, a.z / spp, a.w / spp); }
        if (out.normal || out.depth) {
            const float4 a = acc.normal[lp];
            if (out.normal) out.normal[lp] = make_float4(a.x / spp, a.y / spp, a.z / spp, 0.f);
            if (out.depth) out.depth[lp] = a.w / spp;
        }
        if (out.shading) { const float4 a = acc.shading[lp]; out.shading[lp] = make_float4(a.x / spp, a.y / spp, a.z / spp, 0.f); }
    }
}

// compiled in inst_aov.hip
#define GX_AOV_RESOLVE_SIGNATURE(M) __global__ void gnxr::k_aov_resolve<M>(gnxr::DScene, gnxr::AovTables, const float4 *, int, int, int, gnxr::AovAccum, int, int2 *);
#define GX_AOV_INSTANCES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

}  // namespace gnxr
