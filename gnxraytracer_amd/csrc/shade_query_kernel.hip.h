// shade_query_kernel.hip.h -- batched shading queries on caller-supplied device memory (gnxr_bsdf_device, gnxr_light_sample_device,
// gnxr_light_le_device): BSDF::f / Pdf / Sample_f at the hit of a ray, Light::Sample_Li / Pdf_Li / the light-selection pdf at a point and
// Light::Le of escaped rays, as entry points of their own.
//
// The BSDF query follows a closest-hit query of k_trace4 (query_kernel.hip.h: the leaf code of every ray in a scratch gnxr_hit::prim) with
// one kernel, k_bsdf_query, that rebuilds the hit and the material with the functions k_shade calls (shade_hit_rebuild, shade_material:
// kernels.hip.h) and evaluates the render's Bsdf<LM> (device_bsdf.h).  The light queries have no traversal: light_sample / light_pdf /
// light_select_pdf / light_Le of device_lights.h on the scene's light tables, one query per lane.
#pragma once
#include "query_kernel.hip.h"

namespace gnxr {

struct BsdfQueryArrays {
    const float4 *rays;      // gnxr_ray i = rays[2 i], rays[2 i + 1]
    const gnxr_hit *codes;   // codes[i].prim: the leaf code k_trace4<..., kT4QueryClosest> (or k_trace_closest_code) left
    const float *wi;         // 3 floats per query, world space
    const float *u;          // 2 floats per query
    const float *diffs;      // nullptr, or 12 floats per query: rxOrigin, rxDirection, ryOrigin, ryDirection
    float4 *out;             // gnxr_bsdf_result i = out[4 i .. 4 i + 3]
};
static_assert(sizeof(gnxr_bsdf_result) == 64 && sizeof(gnxr_light_result) == 48, "the query kernels write these records as float4s");

// Scenes the 4-wide encoding cannot hold: the reference's binary walk (k_trace_closest_api's), leaving the leaf code instead of the record
template <int STACK>
__global__ void __launch_bounds__(kBlock) k_trace_closest_code(DScene sc, const gnxr_ray *rays, long long n, gnxr_hit *codes) {
    __shared__ int stack[STACK * kBlock];
    TraceCounters tc = {0, 0};
    for (long long i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        gnxr_ray r = rays[i];
        V3 ro(r.o[0], r.o[1], r.o[2]), rd(r.d[0], r.d[1], r.d[2]);
        TriHit h;
        float tMax = r.tmax;
        int sphereHit = -1;
        for (int si = 0; si < sc.n_spheres; ++si) { float tH; if (sphere_test(sc.spheres[si], ro, rd, tMax, &tH)) { tMax = tH; sphereHit = si; } }
        int leaf = bvh_traverse<false, kBlock, false>(sc.nodes, sc.tris, ro, rd, tMax, &stack[threadIdx.x], &h, &tc);
        codes[i].prim = leaf >= 0 ? leaf : (sphereHit >= 0 ? -2 - sphereHit : -1);
    }
}

// Scene::Intersect is done (codes); per ray: SurfaceInteraction + ComputeScatteringFunctions(ray, arena, allowMultipleLobes = true,
// TransportMode::Radiance) + BSDF::f / Pdf / Sample_f / NumComponents with wo = isect.wo = Normalize(-ray.d).  Spheres and the per-corner
// tables are always compiled in (SPH = TEX = true of k_shade: a scene without them takes the same arithmetic through the defaults).
template <uint32_t LM>
__global__ void __launch_bounds__(kBlock, 2) k_bsdf_query(DScene sc, BsdfQueryArrays q, long long n, int flags) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float4 a = q.rays[2 * i], b = q.rays[2 * i + 1];
        const V3 ro(a.x, a.y, a.z), rd(b.x, b.y, b.z);
        const int leaf = q.codes[i].prim;
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
        V3 p0, p1, p2, sdpdu, sdpdv;
        TriHit h;
        SurfacePoint sp;
        int triMat = -1, triLight = -1;
        if (shade_hit_rebuild<true, true, true>(sc, sc.materials, leaf, ro, rd, a.w, &p0, &p1, &p2, &h, &triMat, &triLight, &sp, &sdpdu, &sdpdv) && triMat >= 0) {
            RayDiff rdf;
            rdf.has = q.diffs != nullptr;
            UVDiff ud = {};
            if (rdf.has) {
                const float *d = q.diffs + 12 * i;
                rdf.rxo = V3(d[0], d[1], d[2]); rdf.rxd = V3(d[3], d[4], d[5]);
                rdf.ryo = V3(d[6], d[7], d[8]); rdf.ryd = V3(d[9], d[10], d[11]);
                // SurfaceInteraction::ComputeDifferentials on the interaction's own dpdu / dpdv (what the record reports; shade_material
                // takes the same values to the textures)
                V3 dpdu = sdpdu, dpdv = sdpdv;
                if (leaf >= 0) { float tu, tv; tri_uv_frame(p0, p1, p2, h, tri_uvs(tex_tables(sc.materials), leaf), &tu, &tv, &dpdu, &dpdv); }
                ud = compute_differentials(rdf, sp.p, sp.n, dpdu, dpdv);
            }
            DMaterial tm;
            const DMaterial *mat = shade_material<true>(sc, sc.materials + triMat, leaf, p0, p1, p2, h, sp, rdf, &tm);
            Bsdf<LM> bsdf;
            bsdf.mat = mat; bsdf.ns = sp.ns; bsdf.ng = sp.n; bsdf.ss = sp.ss; bsdf.ts = sp.ts;
            const V3 woN = normalize(-rd);   // Interaction::wo
            const V3 wi(q.wi[3 * i], q.wi[3 * i + 1], q.wi[3 * i + 2]);
            const Spec f = bsdf.f(woN, wi, flags);
            const float pdf = bsdf.pdf(woN, wi, flags);
            V3 wis;
            float spdf = 0;
            int sampledType = 0;
            Spec sf = bsdf.sample_f(woN, &wis, q.u[2 * i], q.u[2 * i + 1], &spdf, flags, &sampledType);
            if (spdf == 0) { sf = Spec(0.f); wis = V3(); }
            r0 = make_float4(f.r, f.g, f.b, pdf);
            r1 = make_float4(sf.r, sf.g, sf.b, spdf);
            r2 = make_float4(wis.x, wis.y, wis.z, __int_as_float(sampledType));
            r3 = make_float4(__int_as_float(bsdf.num_components(flags)), __int_as_float(1), ud.dudx, ud.dvdy);
        }
        q.out[4 * i] = r0; q.out[4 * i + 1] = r1; q.out[4 * i + 2] = r2; q.out[4 * i + 3] = r3;
    }
}

// d_queries: three float4 per query -- (p.xyz, light), (n.xyz, u0), (u1, wi_query.xyz).  A light outside [0, n_lights) leaves a zero
// record and its index in *bad (~index, largest wins: the first such query; 0 = none).
template <int LT>
__global__ void __launch_bounds__(kBlock) k_light_sample_query(DLightTables lt, const float4 *__restrict__ queries, long long n, float4 *__restrict__ out,
                                                               unsigned long long *bad) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float4 qa = queries[3 * i], qb = queries[3 * i + 1], qc = queries[3 * i + 2];
        const V3 p(qa.x, qa.y, qa.z), nrm(qb.x, qb.y, qb.z), wiq(qc.y, qc.z, qc.w);
        const int li = __float_as_int(qa.w);
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
        if (li < 0 || li >= lt.n_lights) atomicMax(bad, ~(unsigned long long)i);
        else {
            const LightSample ls = light_sample<LT>(lt, li, p, qb.w, qc.x);
            const float pdfLi = light_pdf<LT>(lt, li, p, V3(), nrm, wiq);   // an Interaction built from (p, n): pError = 0
            r0 = make_float4(ls.Li.r, ls.Li.g, ls.Li.b, ls.pdf);
            r1 = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, pdfLi);
            r2 = make_float4(light_select_pdf(lt, p, li), ls.p1.x, ls.p1.y, ls.p1.z);
        }
        out[3 * i] = r0; out[3 * i + 1] = r1; out[3 * i + 2] = r2;
    }
}

// Light::Le(ray) of one light for escaped rays
template <int LT>
__global__ void __launch_bounds__(kBlock) k_light_le_query(DLightTables lt, int li, const float4 *__restrict__ rays, long long n, float *__restrict__ le) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float4 a = rays[2 * i], b = rays[2 * i + 1];
        const Spec L = light_Le<LT>(lt, li, V3(a.x, a.y, a.z), V3(b.x, b.y, b.z));
        le[3 * i] = L.r; le[3 * i + 1] = L.g; le[3 * i + 2] = L.b;
    }
}

// compiled in inst_shade_query.hip
#define GX_BSDF_QUERY_SIGNATURE(LM) __global__ void gnxr::k_bsdf_query<LM>(gnxr::DScene, gnxr::BsdfQueryArrays, long long, int);
#define GX_LIGHT_SAMPLE_QUERY_SIGNATURE(LT) \
    __global__ void gnxr::k_light_sample_query<LT>(gnxr::DLightTables, const float4 *, long long, float4 *, unsigned long long *);
#define GX_LIGHT_LE_QUERY_SIGNATURE(LT) __global__ void gnxr::k_light_le_query<LT>(gnxr::DLightTables, int, const float4 *, long long, float *);
#define GX_TRACE_CLOSEST_CODE_SIGNATURE(STACK) __global__ void gnxr::k_trace_closest_code<STACK>(gnxr::DScene, const gnxr_ray *, long long, gnxr_hit *);

}  // namespace gnxr
