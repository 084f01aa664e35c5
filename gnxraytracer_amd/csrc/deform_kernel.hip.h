// deform_kernel.hip.h -- deforming smooth meshes on the device: linear-blend skinning with blend shapes (gnxr_skin_vertices_device),
// per-corner attribute edits (gnxr_scene_update_attributes, gnxr_scene_triangle_attributes) and area-weighted shading normals from the
// vertices a scene holds (gnxr_scene_recompute_normals).  The definitions: include/gnxr.h.
//
//   k_skin             one lane per vertex: morph targets in order, then the four bone slots in order
//   k_attr_edit<false> one lane per leaf-order triangle, those of the edited range work: would its own-attribute byte change, is it emissive; writes nothing
//   k_attr_edit<true>  the same lanes: the caller's rows (authoring order, unpadded) into the padded leaf-order tables
//   k_attr_gather      the getter: padded leaf-order rows back to authoring order, unpadded
//   k_adj_corners      the adjacency's input: per AUTHORED corner 3 t + k its vertex, and the number of corners per vertex (integer atomics);
//                      the host driver scans the counts into CSR offsets and sorts the corners by vertex (api_deform.hip.h)
//   k_face_normals    one lane per leaf-order triangle: the unnormalised face normal and the smooth flag of its AUTHORED triangle
//   k_vertex_normals   one lane per vertex: the sum over its corner list, in list order (ascending authored triangle, then corner)
//   k_write_normals    one lane per leaf-order triangle: the corners of smooth triangles take N / sqrt(|N|^2), or keep what they had
//
// The build flags forbid contraction (-ffp-contract=off), so every product and every sum below is one rounded fp32 operation, and
// division and square root are the correctly rounded ones (device_math.h, gx_sqrt).  No float atomics anywhere: the order of every sum is
// part of the definition.  A leaf-order triangle finds its authored number in DTri::prim and its vertices in the refit's corner table, both
// kept current by gnxr_scene_rebuild_bvh and gnxr_scene_set_geometry, so nothing here holds a leaf index across calls.
#pragma once
#include <hip/hip_runtime.h>

#include "gnxr_device_types.h"

namespace gnxr {
namespace deform {

constexpr int kB = 256;   // threads per block

// ---- skinning.  bone_index / bone_weight rows and the bone matrices' rows are 16 bytes and read as such (the entry point checks alignment).
static __global__ void __launch_bounds__(kB) k_skin(int n_vertices, int n_bones, int n_morphs, const float *__restrict__ rest, const int4 *__restrict__ bone_index,
                                                   const float4 *__restrict__ bone_weight, const float4 *__restrict__ bones, const float *__restrict__ morph_delta,
                                                   const float *__restrict__ morph_weight, float *__restrict__ out, int *__restrict__ flag) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vertices; v += gridDim.x * blockDim.x) {
        float qx = rest[3 * (size_t)v], qy = rest[3 * (size_t)v + 1], qz = rest[3 * (size_t)v + 2];
        for (int m = 0; m < n_morphs; ++m) {
            const float w = morph_weight[m];
            const float *d = morph_delta + 3 * ((size_t)m * n_vertices + v);
            qx = qx + w * d[0]; qy = qy + w * d[1]; qz = qz + w * d[2];
        }
        const int4 bi = bone_index[v];
        const float4 bw = bone_weight[v];
        float px = 0.f, py = 0.f, pz = 0.f;
        bool bad = false;
        const auto slot = [&](float w, int b) {   // (called four times: the build does not unroll loops)
            if (w == 0.f) return;   // an unused slot: its index is not looked at
            if ((unsigned)b >= (unsigned)n_bones) { bad = true; return; }   // never dereferenced
            const float4 r0 = bones[3 * (size_t)b], r1 = bones[3 * (size_t)b + 1], r2 = bones[3 * (size_t)b + 2];
            const float tx = ((r0.x * qx + r0.y * qy) + r0.z * qz) + r0.w;
            const float ty = ((r1.x * qx + r1.y * qy) + r1.z * qz) + r1.w;
            const float tz = ((r2.x * qx + r2.y * qy) + r2.z * qz) + r2.w;
            px = px + w * tx; py = py + w * ty; pz = pz + w * tz;
        };
        slot(bw.x, bi.x); slot(bw.y, bi.y); slot(bw.z, bi.z); slot(bw.w, bi.w);
        if (bad) { *flag = 1; continue; }
        out[3 * (size_t)v] = px; out[3 * (size_t)v + 1] = py; out[3 * (size_t)v + 2] = pz;
    }
}

// ---- per-corner attributes.  Tables: uv 2 float4 per leaf-order triangle (u0 v0 u1 v1 | u2 v2 0 0), normals and tangents 3 float4
// (9 floats, 3 of padding): the layout of compile_scene and k_geom_build.
struct AttrTables { float4 *uv, *n, *s; };                     // the scene's tables; null where the scene has none
struct AttrRows { const float *uv, *n, *s; int first, count; };   // the caller's rows for authored triangles [first, first + count); null = leave as is

__device__ __forceinline__ bool uv_custom(float4 a, float4 b) {   // any bit differs from the GetUVs defaults (0,0) (1,0) (1,1)
    const unsigned one = 0x3f800000u;
    return (__float_as_uint(a.x) | __float_as_uint(a.y) | (__float_as_uint(a.z) ^ one) | __float_as_uint(a.w) | (__float_as_uint(b.x) ^ one) | (__float_as_uint(b.y) ^ one)) != 0u;
}
__device__ __forceinline__ bool rows_nonzero(float4 a, float4 b, float4 c) {   // memcmp with nine zeros: -0 counts as set
    return (__float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(a.z) | __float_as_uint(a.w) | __float_as_uint(b.x) | __float_as_uint(b.y) | __float_as_uint(b.z) |
            __float_as_uint(b.w) | __float_as_uint(c.x)) != 0u;
}
__device__ __forceinline__ void load_rows9(const float *__restrict__ src, float4 r[3]) {   // (dword loads: a caller's array need not be aligned beyond its element)
    r[0] = make_float4(src[0], src[1], src[2], src[3]);
    r[1] = make_float4(src[4], src[5], src[6], src[7]);
    r[2] = make_float4(src[8], 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void load_rows6(const float *__restrict__ src, float4 r[2]) {
    r[0] = make_float4(src[0], src[1], src[2], src[3]);
    r[1] = make_float4(src[4], src[5], 0.f, 0.f);
}

enum : int { A_OWN_CHANGES = 1, A_EMISSIVE_NORMALS = 2, A_EMISSIVE_TANGENTS = 4 };

// write == false: the refusals (flag |= A_*), nothing written; write == true: the rows
template <bool kWrite>
static __global__ void __launch_bounds__(kB) k_attr_edit(const DTri *__restrict__ tris, int n_tris, AttrTables tab, AttrRows in, int *__restrict__ flag) {
    int flags = 0;
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int k = tris[li].prim - in.first;
        if (k < 0 || k >= in.count) continue;
        float4 uv[2], n[3], s[3];
        if (in.uv) load_rows6(in.uv + 6 * (size_t)k, uv);
        if (in.n) load_rows9(in.n + 9 * (size_t)k, n);
        if (in.s) load_rows9(in.s + 9 * (size_t)k, s);
        if (kWrite) {
            if (in.uv) { tab.uv[2 * (size_t)li] = uv[0]; tab.uv[2 * (size_t)li + 1] = uv[1]; }
            if (in.n) { tab.n[3 * (size_t)li] = n[0]; tab.n[3 * (size_t)li + 1] = n[1]; tab.n[3 * (size_t)li + 2] = n[2]; }
            if (in.s) { tab.s[3 * (size_t)li] = s[0]; tab.s[3 * (size_t)li + 1] = s[1]; tab.s[3 * (size_t)li + 2] = s[2]; }
            continue;
        }
        // the own-attribute byte before and after (compile_scene: custom uvs, or a normal or tangent row with a bit set)
        bool was = false, now = false;
        if (tab.uv) {
            const bool old = uv_custom(tab.uv[2 * (size_t)li], tab.uv[2 * (size_t)li + 1]);
            was = was || old; now = now || (in.uv ? uv_custom(uv[0], uv[1]) : old);
        }
        if (tab.n) {
            const bool old = rows_nonzero(tab.n[3 * (size_t)li], tab.n[3 * (size_t)li + 1], tab.n[3 * (size_t)li + 2]);
            const bool has = in.n ? rows_nonzero(n[0], n[1], n[2]) : old;
            if (in.n && has && tris[li].light >= 0) flags |= A_EMISSIVE_NORMALS;
            was = was || old; now = now || has;
        }
        if (tab.s) {
            const bool old = rows_nonzero(tab.s[3 * (size_t)li], tab.s[3 * (size_t)li + 1], tab.s[3 * (size_t)li + 2]);
            const bool has = in.s ? rows_nonzero(s[0], s[1], s[2]) : old;
            if (in.s && has && tris[li].light >= 0) flags |= A_EMISSIVE_TANGENTS;
            was = was || old; now = now || has;
        }
        if (was != now) flags |= A_OWN_CHANGES;
    }
    if (!kWrite && flags) atomicOr(flag, flags);
}

// which: 0 uv (6 floats per triangle), 1 normals, 2 tangents (9); table: that table of the scene
static __global__ void __launch_bounds__(kB) k_attr_gather(const DTri *__restrict__ tris, int n_tris, int which, const float4 *__restrict__ table, float *__restrict__ out) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const size_t t = (size_t)tris[li].prim;
        if (which == 0) {
            const float4 a = table[2 * (size_t)li], b = table[2 * (size_t)li + 1];
            float *o = out + 6 * t;
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y;
        } else {
            const float4 a = table[3 * (size_t)li], b = table[3 * (size_t)li + 1], c = table[3 * (size_t)li + 2];
            float *o = out + 9 * t;
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; o[8] = c.x;
        }
    }
}

// ---- the adjacency table: CSR from vertex to authored corner ids 3 t + k, ascending within a vertex.  corner: the refit's table (3 per
// leaf-order triangle: the authored vertex of each corner).  keys / vals are what the stable LSD radix sort of the HLBVH stage
// (k_rs_hist / k_rs_scatter) sorts by vertex: input in ascending corner id, so equal vertices keep that order.
static __global__ void __launch_bounds__(kB) k_adj_corners(const DTri *__restrict__ tris, const int *__restrict__ corner, int n_tris, int n_vertices, uint32_t *__restrict__ keys,
                                                          uint32_t *__restrict__ vals, uint32_t *__restrict__ counts) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const size_t t = (size_t)tris[li].prim;
        for (int k = 0; k < 3; ++k) {
            const int v = corner[3 * (size_t)li + k];
            keys[3 * t + k] = (uint32_t)v;
            vals[3 * t + k] = (uint32_t)(3 * t + k);
            if ((unsigned)v < (unsigned)n_vertices) atomicAdd(&counts[v], 1u);   // (the scene's indices were validated when it took them)
        }
    }
}

// face: per AUTHORED triangle (F.x, F.y, F.z, smooth ? 1 : 0); sign: +1 or -1 (GNXR_NORMALS_FLIP: an exact negation)
static __global__ void __launch_bounds__(kB) k_face_normals(const DTri *__restrict__ tris, int n_tris, const float4 *__restrict__ tri_n, float sign, float4 *__restrict__ face) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const float4 *row = reinterpret_cast<const float4 *>(tris + li);
        const float4 p0 = row[0], p1 = row[1], p2 = row[2];
        const bool smooth = rows_nonzero(tri_n[3 * (size_t)li], tri_n[3 * (size_t)li + 1], tri_n[3 * (size_t)li + 2]);
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z, bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
        const float fx = ay * bz - az * by, fy = az * bx - ax * bz, fz = ax * by - ay * bx;
        face[__float_as_int(p0.w)] = make_float4(sign * fx, sign * fy, sign * fz, smooth ? 1.f : 0.f);
    }
}

// One lane per vertex walks its list: a long list costs that lane time, nothing else (no LDS, no bound on the valence).
static __global__ void __launch_bounds__(kB) k_vertex_normals(int n_vertices, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ corners, const float4 *__restrict__ face,
                                                             float4 *__restrict__ vsum) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vertices; v += gridDim.x * blockDim.x) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        const uint32_t end = offsets[v + 1];
        for (uint32_t j = offsets[v]; j < end; ++j) {
            const float4 f = face[corners[j] / 3u];
            if (f.w != 0.f) { nx = nx + f.x; ny = ny + f.y; nz = nz + f.z; }   // flat triangles take no part
        }
        vsum[v] = make_float4(nx, ny, nz, 0.f);
    }
}

static __global__ void __launch_bounds__(kB) k_write_normals(const DTri *__restrict__ tris, const int *__restrict__ corner, int n_tris, int n_vertices, const float4 *__restrict__ vsum,
                                                            float4 *__restrict__ tri_n) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const float4 r0 = tri_n[3 * (size_t)li], r1 = tri_n[3 * (size_t)li + 1], r2 = tri_n[3 * (size_t)li + 2];
        if (!rows_nonzero(r0, r1, r2)) continue;   // a flat triangle is not written
        const auto corner_normal = [&](int k, float &x, float &y, float &z) {   // (x, y, z): what the corner holds; replaced or kept
            const int v = corner[3 * (size_t)li + k];
            if ((unsigned)v >= (unsigned)n_vertices) return;
            const float4 N = vsum[v];
            const float l2 = (N.x * N.x + N.y * N.y) + N.z * N.z;
            if (!(l2 > 0.f) || !(l2 <= 3.402823466e+38f)) return;   // zero, NaN or infinite: the corner keeps the normal it had
            const float len = __builtin_sqrtf(l2);
            x = N.x / len; y = N.y / len; z = N.z / len;
        };
        float4 w0 = r0, w1 = r1, w2 = r2;
        corner_normal(0, w0.x, w0.y, w0.z);
        corner_normal(1, w0.w, w1.x, w1.y);
        corner_normal(2, w1.z, w1.w, w2.x);
        tri_n[3 * (size_t)li] = w0; tri_n[3 * (size_t)li + 1] = w1; tri_n[3 * (size_t)li + 2] = w2;
    }
}

}  // namespace deform
}  // namespace gnxr
