// refit_kernel.hip.h -- gnxr_scene_update_vertices on the device: new vertex positions into the leaf-order triangles, the binary BVH's
// boxes recomputed bottom-up with its topology and primitive order kept, the 4-wide tree's child slots refilled from it.
//
//   k_refit_check    vertices of emissive triangles must keep their value (DLight holds them): raises a flag, writes nothing
//   k_refit_tris     DTri corners whose authored vertex is in the updated range take the new position (.w ids kept)
//   k_refit_fit      leaf boxes (DNode + leaf_boxes) and interior unions, bottom-up with arrival counters (the form of k_hl_fit)
//   k_refit_wide     DNode4 child slots <- the binary node each one was collapsed from (CompiledScene::node4_src)
//   k_refit_lights   GNXR_UPDATE_MOVE_LIGHTS (instead of k_refit_check): corners, area and normal of every AREA_TRI DLight from its triangle
//
// Every box is a union of primitive bounds -- an exact componentwise min / max -- so the refitted tree is exactly the LinearBVHNode[]
// BVHAccel would hold for this topology over the new vertices.  min / max are written as std::min / std::max are (`b < a ? b : a`,
// `a < b ? b : a`) and applied in the reference's order: a triangle's box is Union(Bounds3f(p0, p1), p2) (Triangle::WorldBound), a
// leaf's box the union of its triangles' boxes in leaf order starting from the empty box (recursiveBuild / emitLBVH), an interior box
// Union(children[0], children[1]) (InitInterior).  That keeps even the sign of a zero where the two operands compare equal.
#pragma once
#include <hip/hip_runtime.h>

#include "gnxr_device_types.h"

namespace gnxr {
namespace refit {

constexpr int kB = 256;   // threads per block

__device__ __forceinline__ float rmin(float a, float b) { return b < a ? b : a; }   // std::min(a, b)
__device__ __forceinline__ float rmax(float a, float b) { return a < b ? b : a; }   // std::max(a, b)

// xyz: the staged positions of vertices [first, first + n)
static __global__ void __launch_bounds__(kB) k_refit_check(const DTri *__restrict__ tris, const int *__restrict__ corner, int n_tris, int first, int n,
                                                          const float *__restrict__ xyz, int *__restrict__ flag) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const DTri &t = tris[li];
        if (t.light < 0) continue;
        const float *p[3] = {t.p0, t.p1, t.p2};
        for (int c = 0; c < 3; ++c) {
            const int v = corner[3 * li + c] - first;
            if (v < 0 || v >= n) continue;
            for (int k = 0; k < 3; ++k)
                if (__float_as_uint(xyz[3 * v + k]) != __float_as_uint(p[c][k])) *flag = 1;   // bit for bit: -0 for +0 is a change too
        }
    }
}

static __global__ void __launch_bounds__(kB) k_refit_tris(DTri *__restrict__ tris, const int *__restrict__ corner, int n_tris, int first, int n,
                                                         const float *__restrict__ xyz) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        DTri &t = tris[li];
        float *p[3] = {t.p0, t.p1, t.p2};
        for (int c = 0; c < 3; ++c) {
            const int v = corner[3 * li + c] - first;
            if (v < 0 || v >= n) continue;
            for (int k = 0; k < 3; ++k) p[c][k] = xyz[3 * v + k];
        }
    }
}

// One lane per binary node; leaves compute their box from their triangles and climb: the first child to arrive at a parent leaves, the
// second forms the union and moves on (k_hl_fit, hlbvh_build.hip.h, with the same fences and agent-scope loads).  `arrived` is zero on entry.
static __global__ void __launch_bounds__(kB) k_refit_fit(int n_nodes, DNode *__restrict__ nodes, const int *__restrict__ parent, unsigned int *__restrict__ arrived,
                                                        const DTri *__restrict__ tris, float *__restrict__ leaf_boxes) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x) {
        const int nPrims = (int)(nodes[i].meta & 0xffffu);
        if (nPrims == 0) continue;
        const int off = nodes[i].offset;
        float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};   // Bounds3f()
        for (int j = off; j < off + nPrims; ++j) {
            const DTri &t = tris[j];
            for (int k = 0; k < 3; ++k) {
                const float tlo = rmin(rmin(t.p0[k], t.p1[k]), t.p2[k]), thi = rmax(rmax(t.p0[k], t.p1[k]), t.p2[k]);
                lo[k] = rmin(lo[k], tlo);
                hi[k] = rmax(hi[k], thi);
            }
        }
        nodes[i].lo[0] = lo[0]; nodes[i].lo[1] = lo[1]; nodes[i].lo[2] = lo[2];
        nodes[i].hi0 = hi[0]; nodes[i].hi1 = hi[1]; nodes[i].hi2 = hi[2];
        float *lb = leaf_boxes + (size_t)off * 8;
        lb[0] = lo[0]; lb[1] = lo[1]; lb[2] = lo[2]; lb[3] = hi[0]; lb[4] = hi[1]; lb[5] = hi[2];
        int p = parent[i];
        while (p >= 0) {
            __threadfence();
            if (atomicAdd(&arrived[p], 1u) == 0u) break;   // the first child waits for nobody: the sibling's thread finishes the node
            __threadfence();
            // the sibling's box was written by another CU: read it past this CU's vector cache (agent-scope loads)
            const DNode *a = &nodes[p + 1], *b = &nodes[nodes[p].offset];
            const float *alo = a->lo, *blo = b->lo, *ahi = &a->hi0, *bhi = &b->hi0;
            float ulo[3], uhi[3];
            for (int k = 0; k < 3; ++k) {
                ulo[k] = rmin(__hip_atomic_load(alo + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(blo + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                uhi[k] = rmax(__hip_atomic_load(ahi + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(bhi + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            nodes[p].lo[0] = ulo[0]; nodes[p].lo[1] = ulo[1]; nodes[p].lo[2] = ulo[2];
            nodes[p].hi0 = uhi[0]; nodes[p].hi1 = uhi[1]; nodes[p].hi2 = uhi[2];
            p = parent[p];
        }
    }
}

// One lane per DNode4 child slot; empty slots (src < 0) keep their inverted box
static __global__ void __launch_bounds__(kB) k_refit_wide(int n_slots, DNode4 *__restrict__ nodes4, const int *__restrict__ src, const DNode *__restrict__ nodes) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_slots; j += gridDim.x * blockDim.x) {
        const int s = src[j];
        if (s < 0) continue;
        DNode4 &d = nodes4[j >> 2];
        const int k = j & 3;
        const DNode &g = nodes[s];
        d.lox[k] = g.lo[0]; d.loy[k] = g.lo[1]; d.loz[k] = g.lo[2];
        d.hix[k] = g.hi0; d.hiy[k] = g.hi1; d.hiz[k] = g.hi2;
    }
}

// One lane per light; every AREA_TRI record (tri_leaf >= 0) takes p0 p1 p2, area, inv_area and n from its leaf-order triangle, moved or
// not.  The arithmetic is compile_scene's (scene_compile.cpp, host_math.h: Triangle::Area and the normal of Triangle::Sample), operation for
// operation, so a record whose corners did not change keeps its bits: fp32 corner differences, a cross product of double products
// (each product of two floats is exact in double; one rounding in the subtraction, one to float), an fp32 dot product summed left to
// right, IEEE sqrt and division, area = length / 2, n = cross * (1 / length).  A zero-area triangle gets area 0, inv_area inf and a NaN
// normal, as gnxr_scene_create gives it.
static __global__ void __launch_bounds__(kB) k_refit_lights(DLight *__restrict__ lights, int n_lights, const DTri *__restrict__ tris, int n_tris) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lights; i += gridDim.x * blockDim.x) {
        DLight &l = lights[i];
        const int li = l.tri_leaf;
        if (li < 0 || li >= n_tris) continue;   // not an area light
        const DTri &t = tris[li];
        float a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            l.p0[k] = t.p0[k]; l.p1[k] = t.p1[k]; l.p2[k] = t.p2[k];
            a[k] = t.p1[k] - t.p0[k];
            b[k] = t.p2[k] - t.p0[k];
        }
        const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
        const float cx = (float)((ay * bz) - (az * by)), cy = (float)((az * bx) - (ax * bz)), cz = (float)((ax * by) - (ay * bx));   // Geometry.h:925-931
        const float len = __builtin_sqrtf(cx * cx + cy * cy + cz * cz);   // (IEEE under hipcc's defaults: device_math.h gx_sqrt)
        const float area = 0.5f * len;
        l.area = area;
        l.inv_area = 1 / area;
        const float inv = 1.f / len;   // Vector3::operator/, Geometry.h:206-210
        l.n[0] = cx * inv; l.n[1] = cy * inv; l.n[2] = cz * inv;
    }
}

}  // namespace refit
}  // namespace gnxr
