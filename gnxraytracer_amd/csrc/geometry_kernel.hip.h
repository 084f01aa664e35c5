// geometry_kernel.hip.h -- gnxr_scene_set_geometry on the device: the front of the rebuild pipeline.  From a caller's vertex and index
// arrays and its per-triangle arrays, one pass makes the tables compile_scene (scene_compile.cpp) makes on the host, held in AUTHORING
// order (triangle i at row i), which is what rebuild_on_device (api_rebuild.hip.h) takes as its source and permutes into leaf order.
//
//   k_geom_build     one lane per triangle: validates its record, then writes DTri (corners, prim = i, the AUTHORED material id, the light),
//                    the corner table, tri_media, the padded tri_uv / tri_n / tri_s rows and the own-attribute byte; raises error flags and
//                    counts, per light, the triangles that name it
//
// DTri::material and the class byte depend on the material tables, which depend on the own-attribute bytes of ALL triangles
// (compile_materials): k_material_tris (material_kernel.hip.h) writes both over these tables once the host has compiled mat_map.
//
// An index is compared with n_vertices before it is used: a triangle with a bad index raises its flag and gathers nothing.  Every store is
// a plain vector store by the lane that owns the row; the flags and counters are atomics on global memory.
#pragma once
#include <hip/hip_runtime.h>

#include "gnxr_device_types.h"
#include "refit_kernel.hip.h"

namespace gnxr {
namespace geom {

// chk[0]: the OR of these; chk[1 + l]: how many triangles name light l; chk[1 + n_lights + l]: the largest such triangle
enum : int { G_BAD_INDEX = 1, G_BAD_MATERIAL = 2, G_BAD_MEDIUM = 4, G_BAD_LIGHT = 8, G_EMISSIVE_NORMALS = 16, G_EMISSIVE_TANGENTS = 32, G_NOT_FINITE = 64 };

struct GeomIn {
    const float *vertices; const int *indices, *tri_material, *tri_light, *med_in, *med_out; const float *tri_uv, *tri_n, *tri_s;   // gnxr_geometry
    int n_vertices, n_triangles, n_materials, n_media, n_lights;
};
struct GeomOut {
    DTri *tris; unsigned char *own_attr; int *corner; int2 *tri_media; float4 *tri_uv, *tri_n, *tri_s;   // the last four null where the input is
    int *chk;
};

// 9 floats of a per-corner array -> three padded rows; returns whether any of them has a bit set (memcmp with zeros, as compile_scene)
__device__ __forceinline__ bool geom_rows9(const float *__restrict__ src, float4 *__restrict__ dst) {
    float f[9];
    unsigned any = 0u;
    for (int k = 0; k < 9; ++k) { f[k] = src[k]; any |= __float_as_uint(f[k]); }
    dst[0] = make_float4(f[0], f[1], f[2], f[3]);
    dst[1] = make_float4(f[4], f[5], f[6], f[7]);
    dst[2] = make_float4(f[8], 0.f, 0.f, 0.f);
    return any != 0u;
}

static __global__ void __launch_bounds__(refit::kB) k_geom_build(GeomIn in, GeomOut out) {
    int flags = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < in.n_triangles; i += gridDim.x * blockDim.x) {
        const size_t t = (size_t)i;
        const int i0 = in.indices[3 * t], i1 = in.indices[3 * t + 1], i2 = in.indices[3 * t + 2];
        const int mat = in.tri_material[t], light = in.tri_light ? in.tri_light[t] : -1;
        const int mi = in.med_in ? in.med_in[t] : -1, mo = in.med_out ? in.med_out[t] : -1;
        int bad = 0;
        if ((unsigned)i0 >= (unsigned)in.n_vertices || (unsigned)i1 >= (unsigned)in.n_vertices || (unsigned)i2 >= (unsigned)in.n_vertices) bad |= G_BAD_INDEX;
        if (mat < -1 || mat >= in.n_materials) bad |= G_BAD_MATERIAL;
        if (mi < -1 || mi >= in.n_media || mo < -1 || mo >= in.n_media) bad |= G_BAD_MEDIUM;
        if (light < -1 || light >= in.n_lights) bad |= G_BAD_LIGHT;
        if (bad) { flags |= bad; continue; }   // nothing of a refused triangle is gathered or written: the call fails
        if (light >= 0) { atomicAdd(&out.chk[1 + light], 1); atomicMax(&out.chk[1 + in.n_lights + light], i); }
        const float *p0 = in.vertices + 3 * (size_t)i0, *p1 = in.vertices + 3 * (size_t)i1, *p2 = in.vertices + 3 * (size_t)i2;
        const float4 r0 = make_float4(p0[0], p0[1], p0[2], __int_as_float(i)), r1 = make_float4(p1[0], p1[1], p1[2], __int_as_float(mat)),
                     r2 = make_float4(p2[0], p2[1], p2[2], __int_as_float(light));
        {   // the centroid the build sorts by (k_rb_prims: .5 lo + .5 hi of the corners' box) must be a number: a NaN or an infinite one has no Morton code
            const float cx = .5f * refit::rmin(refit::rmin(r0.x, r1.x), r2.x) + .5f * refit::rmax(refit::rmax(r0.x, r1.x), r2.x);
            const float cy = .5f * refit::rmin(refit::rmin(r0.y, r1.y), r2.y) + .5f * refit::rmax(refit::rmax(r0.y, r1.y), r2.y);
            const float cz = .5f * refit::rmin(refit::rmin(r0.z, r1.z), r2.z) + .5f * refit::rmax(refit::rmax(r0.z, r1.z), r2.z);
            // (a NaN corner can hide behind rmin / rmax, which keep their first operand then: the corners are tested as well)
            const bool nan = r0.x != r0.x || r0.y != r0.y || r0.z != r0.z || r1.x != r1.x || r1.y != r1.y || r1.z != r1.z || r2.x != r2.x || r2.y != r2.y || r2.z != r2.z;
            if (nan || !isfinite(cx) || !isfinite(cy) || !isfinite(cz)) flags |= G_NOT_FINITE;
        }
        float4 *row = reinterpret_cast<float4 *>(out.tris + t);
        row[0] = r0; row[1] = r1; row[2] = r2;
        out.corner[3 * t] = i0; out.corner[3 * t + 1] = i1; out.corner[3 * t + 2] = i2;
        if (out.tri_media) out.tri_media[t] = make_int2(mi, mo);
        bool own = false;
        if (in.tri_uv) {
            // custom: any bit differs from the GetUVs defaults (0,0) (1,0) (1,1)
            const float *uv = in.tri_uv + 6 * t;   // (dword loads: a caller's array need not be aligned beyond its element)
            const float2 a = make_float2(uv[0], uv[1]), b = make_float2(uv[2], uv[3]), c = make_float2(uv[4], uv[5]);
            out.tri_uv[2 * t] = make_float4(a.x, a.y, b.x, b.y);
            out.tri_uv[2 * t + 1] = make_float4(c.x, c.y, 0.f, 0.f);
            const unsigned one = 0x3f800000u;
            own = (__float_as_uint(a.x) | __float_as_uint(a.y) | (__float_as_uint(b.x) ^ one) | __float_as_uint(b.y) | (__float_as_uint(c.x) ^ one) | (__float_as_uint(c.y) ^ one)) != 0u;
        }
        if (in.tri_n) {
            const bool has = geom_rows9(in.tri_n + 9 * t, out.tri_n + 3 * t);
            if (has && light >= 0) flags |= G_EMISSIVE_NORMALS;
            own = own || has;
        }
        if (in.tri_s) {
            const bool has = geom_rows9(in.tri_s + 9 * t, out.tri_s + 3 * t);
            if (has && light >= 0) flags |= G_EMISSIVE_TANGENTS;
            own = own || has;
        }
        out.own_attr[t] = own ? 1 : 0;
    }
    if (flags) atomicOr(&out.chk[0], flags);
}

}  // namespace geom
}  // namespace gnxr
