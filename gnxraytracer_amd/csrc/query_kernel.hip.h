// query_kernel.hip.h -- batched ray queries on caller-supplied device memory (gnxr_trace_closest_device / gnxr_trace_any_device).
//
// The traversal is k_trace4's own walk (trace4_kernel.hip.h) in one of two query modes, chosen at compile time: the ray source reads
// gnxr_ray records (two dwordx4 loads) instead of path records, and the retire step writes the leaf code of the closest hit into
// gnxr_hit::prim or the occlusion byte of an any-hit query.  Batch set-up, the LDS ray queue, the node cache, the order table, the slab
// and leaf logic and the spill stack are the render's.  k_trace4 keeps neither t nor the barycentrics, so a second, cheap pass
// (k_query_finish) turns the leaf code into the full record with hit_record() -- the function k_trace_closest_api uses for the host entry
// point -- after recomputing (t, b0, b1, b2) the way the path loop does (tri_hit_recompute).
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// k_trace4's ray source / retire step
enum : int { kT4Render = 0, kT4QueryClosest = 1, kT4QueryAny = 2 };

struct QueryArrays {
    const float4 *rays;        // gnxr_ray i = rays[2 i] (o.xyz, tMax), rays[2 i + 1] (d.xyz, pad); indices are relative to the launch
    gnxr_hit *hits;            // kT4QueryClosest: hits[i].prim <- leaf code (a leaf-order triangle, -1 nothing, -2 - s sphere s)
    unsigned char *occluded;   // kT4QueryAny: 1 when anything is hit in (0, tMax)
};
// the work-source argument of k_trace4: the render's path records, or the caller's rays
template <int Q> struct Trace4Src { typedef QueryArrays type; };
template <> struct Trace4Src<kT4Render> { typedef PathArrays type; };

// gnxr_hit of every ray from the leaf code k_trace4<..., kT4QueryClosest> left in hits[i].prim.  The triangle's (t, b0, b1, b2) are the
// values the traversal's accepting test computed (tri_hit_recompute: same operations, same order); a sphere's t does not depend on the
// tMax it was tested with once it is hit, so testing it again with the ray's own tMax returns the same distance.
static __global__ void __launch_bounds__(kBlock) k_query_finish(DScene sc, const float4 *rays, long long n, gnxr_hit *hits) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float4 a = rays[2 * i], b = rays[2 * i + 1];
        const V3 ro(a.x, a.y, a.z), rd(b.x, b.y, b.z);
        const int code = hits[i].prim;
        TriHit h = {0.f, 0.f, 0.f, 0.f};
        if (code >= 0) {
            V3 p0, p1, p2;
            load_tri(sc.tris, code, &p0, &p1, &p2);
            tri_hit_recompute(p0, p1, p2, ro, rd, &h);
        } else if (code < -1) {
            (void)sphere_test(sc.spheres[-2 - code], ro, rd, a.w, &h.t);
        }
        hits[i] = hit_record(sc, ro, rd, code, h);
    }
}

}  // namespace gnxr
