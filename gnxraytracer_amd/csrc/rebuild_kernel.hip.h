// rebuild_kernel.hip.h -- gnxr_scene_rebuild_bvh on the device: what scene_compile.cpp does on the host between the HLBVH device stage
// (hlbvh_build.hip.h) and the upload, restated as kernels so that neither the build tree nor a node or triangle table crosses to the host.
//
//   k_rb_prims       primitive bounds and centroids from the scene's DTri table (written at the AUTHORING index, DTri::prim, so the build
//                    sees compile_scene's order), the old leaf index of every primitive, the bounds of the centroids (exact reduction)
//   k_rb_parents     parent of every node of the build tree (treelet interiors and upper SAH nodes alike; unused slots are all-zero)
//   k_rb_sizes       nodes per subtree, bottom-up with arrival counters (the form of k_hl_fit)
//   k_rb_flatten     `flatten`: one lane per build node walks to the root and sums what lies in front of it in pre-order (1 for a
//                    first child, 1 + size(first subtree) for a second child), which is its index in DNode[]; writes DNode,
//                    node_parent, leaf_boxes and the maximum depth
//   k_rb_cost        `collapse`, pass 1: the costs T(X, 1..4) of wide_collapse.h and every node's decisions, bottom-up with arrival
//                    counters (the form of k_refit_fit)
//   k_rb_cuts        pass 2: one lane per binary interior node replays the decisions along its own root path (at most the tree's depth
//                    steps) and learns whether it is the root of a DNode4; sums the stack need on the way
//   k_rb_collapse    pass 3: a DNode4's depth-first number is the exclusive scan of that flag over pre-order (scan kernels of
//                    hlbvh_build.hip.h); one lane per DNode4 fills it from its cut (wide_cut, the function the host uses)
//   k_rb_bfs         the breadth-first order of the first kTopNodesMax 4-wide nodes: one block, level by level over a queue in LDS
//   k_rb_renumber    DNode4[] in its final order (top block breadth-first, the rest depth-first), child indices remapped, node4_src
//   k_rb_permute     everything held in leaf order follows the new primitive order
//   k_rb_lights      DLight::tri_leaf of the area lights
//   k_rb_leafcheck   compile_scene's leaf1_from_verts check and upload_scene's "leaf over 127 primitives" test, as flags
//
// No block waits for another: phases are ordered by kernel boundaries, k_rb_sizes by arrive-and-leave counters.  Every walk towards the
// root is bounded by the node count and raises the error flag instead of running on.
#pragma once
#include <hip/hip_runtime.h>

#include "gnxr_device_types.h"
#include "host_scene.h"
#include "refit_kernel.hip.h"
#include "wide_collapse.h"

namespace gnxr {
namespace rebuild {

constexpr int kB = 256;   // threads per block
// the scalars that come back to the host
enum { R_ERROR = 0, R_MAX_DEPTH, R_STACK4_NEED, R_LEAF1_MISMATCH, R_LEAF_OVER_127, R_N_TOP, R_COUNT };

// floats as unsigned integers of the same order (atomicMin / atomicMax on them is the exact minimum / maximum)
__host__ __device__ inline uint32_t float_to_ordered(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ordered_to_float(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// cb: the centroid bounds as ordered integers (lo.xyz, hi.xyz), initialised to the empty box by the host
static __global__ void __launch_bounds__(kB) k_rb_prims(const DTri *__restrict__ tris, int n, float *__restrict__ pb6, float *__restrict__ cen3, int *__restrict__ old_of_prim,
                                                       uint32_t *__restrict__ cb, int *__restrict__ res) {
    const float FMAX = 3.402823466e+38f;
    float clo[3] = {FMAX, FMAX, FMAX}, chi[3] = {-FMAX, -FMAX, -FMAX};
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n; li += gridDim.x * blockDim.x) {
        const DTri &t = tris[li];
        const int prim = t.prim;
        if (prim < 0 || prim >= n) { res[R_ERROR] = 1; continue; }
        old_of_prim[prim] = li;
        for (int k = 0; k < 3; ++k) {
            // Box3::grow from the empty box, one vertex after the other (Triangle::WorldBound as compile_scene states it)
            const float lo = refit::rmin(refit::rmin(refit::rmin(FMAX, t.p0[k]), t.p1[k]), t.p2[k]);
            const float hi = refit::rmax(refit::rmax(refit::rmax(-FMAX, t.p0[k]), t.p1[k]), t.p2[k]);
            const float c = __fadd_rn(__fmul_rn(.5f, lo), __fmul_rn(.5f, hi));
            pb6[6 * (size_t)prim + k] = lo; pb6[6 * (size_t)prim + 3 + k] = hi;
            cen3[3 * (size_t)prim + k] = c;
            clo[k] = fminf(clo[k], c); chi[k] = fmaxf(chi[k], c);
        }
    }
    for (int k = 0; k < 3; ++k) {
        for (int o = 32; o > 0; o >>= 1) { clo[k] = fminf(clo[k], __shfl_xor(clo[k], o)); chi[k] = fmaxf(chi[k], __shfl_xor(chi[k], o)); }
        if ((threadIdx.x & 63) == 0) { atomicMin(&cb[k], float_to_ordered(clo[k])); atomicMax(&cb[3 + k], float_to_ordered(chi[k])); }
    }
}

// a slot of the build tree holds an interior node when its two children differ (unused slots are zero: children 0 and 0)
__device__ __forceinline__ bool rb_interior(const HlbvhNode &nd) { return nd.child[0] != nd.child[1]; }

static __global__ void __launch_bounds__(kB) k_rb_parents(const HlbvhNode *__restrict__ nodes, int U, int cap, int *__restrict__ par, int *__restrict__ res) {
    for (int i = U + blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) {
        const int c0 = nodes[i].child[0], c1 = nodes[i].child[1];
        if (c0 == c1) continue;
        if (c0 < 0 || c0 >= cap || c1 < 0 || c1 >= cap) { res[R_ERROR] = 1; continue; }
        par[c0] = i; par[c1] = i;
    }
}

// `arrived` is zero on entry; the second child to arrive at a node adds the two sizes and moves on (fences and loads as in k_hl_fit)
static __global__ void __launch_bounds__(kB) k_rb_sizes(int U, int cap, const HlbvhNode *__restrict__ nodes, const int *__restrict__ par, unsigned int *__restrict__ arrived,
                                                       int *__restrict__ size, int *__restrict__ res) {
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < U; u += gridDim.x * blockDim.x) {
        size[u] = 1;
        int p = par[u];
        for (int steps = 0; p >= 0; ++steps) {
            if (steps > cap) { res[R_ERROR] = 1; break; }
            __threadfence();
            if (atomicAdd(&arrived[p], 1u) == 0u) break;
            __threadfence();
            const int a = __hip_atomic_load(size + nodes[p].child[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int b = __hip_atomic_load(size + nodes[p].child[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            size[p] = a + b + 1;
            p = par[p];
        }
    }
}

// n_nodes = 2 U - 1.  leaf_boxes is zero on entry.
static __global__ void __launch_bounds__(kB) k_rb_flatten(int U, int cap, int root, int n_nodes, int n_tris, const HlbvhNode *__restrict__ nodes, const int *__restrict__ par,
                                                         const int *__restrict__ size, DNode *__restrict__ out, int *__restrict__ node_parent, float *__restrict__ leaf_boxes,
                                                         int *__restrict__ res) {
    int max_depth = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) {
        const HlbvhNode nd = nodes[i];
        const bool leaf = i < U;
        if (!leaf && !rb_interior(nd)) continue;
        int pre = 0, depth = 0, first_delta = 0, c = i;
        bool bad = false;
        for (int p = par[c]; p >= 0; p = par[c]) {
            if (depth > cap) { bad = true; break; }
            const int delta = nodes[p].child[1] == c ? 1 + size[nodes[p].child[0]] : 1;
            if (depth == 0) first_delta = delta;
            pre += delta; ++depth; c = p;
        }
        if (bad || c != root || pre < 0 || pre >= n_nodes) { res[R_ERROR] = 1; continue; }
        DNode d;
        d.lo[0] = nd.b[0]; d.lo[1] = nd.b[1]; d.lo[2] = nd.b[2];
        d.hi0 = nd.b[3]; d.hi1 = nd.b[4]; d.hi2 = nd.b[5];
        if (leaf) {
            d.offset = nd.first;
            d.meta = (uint32_t)nd.n;
            if (nd.first < 0 || nd.n <= 0 || nd.first + nd.n > n_tris) { res[R_ERROR] = 1; continue; }
            float *lb = leaf_boxes + (size_t)nd.first * 8;
            lb[0] = d.lo[0]; lb[1] = d.lo[1]; lb[2] = d.lo[2]; lb[3] = d.hi0; lb[4] = d.hi1; lb[5] = d.hi2;
        } else {
            d.offset = pre + 1 + size[nd.child[0]];
            d.meta = ((uint32_t)nd.axis) << 16;
        }
        out[pre] = d;
        node_parent[pre] = depth == 0 ? -1 : pre - first_delta;
        max_depth = max(max_depth, depth);
    }
    for (int o = 32; o > 0; o >>= 1) max_depth = max(max_depth, __shfl_xor(max_depth, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&res[R_MAX_DEPTH], max_depth);
}

__device__ __forceinline__ bool rb_is_leaf(const DNode &n) { return (n.meta & 0xffffu) != 0; }
__device__ __forceinline__ int32_t rb_leaf_ref(const DNode &n) { return ~(int32_t)((uint32_t)n.offset | ((n.meta & 0x7fu) << 24)); }
// One lane per leaf of the binary tree climbs: the first child to arrive at a parent leaves, the second computes the parent's costs from the
// two children's (k_refit_fit's scheme, fences and agent-scope loads included).  `arrived` is zero on entry.
__device__ __forceinline__ WideCost rb_load_cost(const WideCost *c) {
    WideCost r;
    for (int k = 0; k < 4; ++k) r.t[k] = __hip_atomic_load(&c->t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}
static __global__ void __launch_bounds__(kB) k_rb_cost(int n_nodes, const DNode *__restrict__ bn, const int *__restrict__ node_parent, unsigned int *__restrict__ arrived,
                                                      WideCost *cost, unsigned char *__restrict__ choice) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x) {
        if (!rb_is_leaf(bn[i])) continue;
        cost[i] = wide_cost_leaf();
        int p = node_parent[i];
        while (p >= 0) {
            __threadfence();
            if (atomicAdd(&arrived[p], 1u) == 0u) break;
            __threadfence();
            const DNode X = bn[p];
            if (X.offset <= p + 1 || X.offset >= n_nodes) break;   // (not a pre-order tree: k_rb_flatten has raised the error flag)
            const WideCost a = rb_load_cost(cost + p + 1), b = rb_load_cost(cost + X.offset);
            WideCost c;
            choice[p] = wide_cost_interior(X, a, b, &c);
            cost[p] = c;
            p = node_parent[p];
        }
    }
}

// is4 / root4: 1 where the node becomes a DNode4 (is4 is scanned in place afterwards).  Both are zero on entry.
static __global__ void __launch_bounds__(kB) k_rb_cuts(int n_nodes, const DNode *__restrict__ bn, const int *__restrict__ node_parent, const unsigned char *__restrict__ choice,
                                                      uint32_t *__restrict__ is4, unsigned char *__restrict__ root4, int *__restrict__ res) {
    int need = 1;
    for (int bi = blockIdx.x * blockDim.x + threadIdx.x; bi < n_nodes; bi += gridDim.x * blockDim.x) {
        if (rb_is_leaf(bn[bi])) continue;
        // the way up: which child each node of the root path is (bit s: the step taken from depth s)
        unsigned long long second = 0ull;
        int depth = 0, c = bi;
        bool deep = false;
        for (int p = node_parent[c]; p >= 0; p = node_parent[c]) {
            if (depth == 64) { deep = true; break; }
            second = (second << 1) | (bn[p].offset == c ? 1ull : 0ull);
            ++depth; c = p;
        }
        if (deep) continue;   // deeper than any tree the host accepts (R_MAX_DEPTH): the call fails on that
        if (c != 0) { res[R_ERROR] = 1; continue; }
        // the way down: `slots` is the number of child slots the node shares among its leaves; 1: the node is a child slot, and being
        // interior (every node of the path is) the root of a DNode4 that leaves k - 1 references on the stack while its first child is walked
        int cur = 0, slots = 1, below = 0;
        bool is_root = false;
        for (int s = 0;; ++s) {
            is_root = slots == 1;
            if (is_root) { slots = wide_best_k(choice[cur]); below += slots - 1; }
            if (s == depth) break;
            const int a = wide_split(choice[cur], slots);
            const bool sec = (second >> s) & 1ull;
            slots = sec ? slots - a : a;
            cur = sec ? bn[cur].offset : cur + 1;
            if (cur <= 0 || cur >= n_nodes) break;   // (not a pre-order tree: caught below)
        }
        if (cur != bi) { res[R_ERROR] = 1; continue; }
        if (is_root) { is4[bi] = 1u; root4[bi] = 1; need = max(need, below + 1); }
    }
    for (int o = 32; o > 0; o >>= 1) need = max(need, __shfl_xor(need, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&res[R_STACK4_NEED], need);
}

// id4: the exclusive scan of is4 (the DNode4's number in collapse's depth-first order).  out / src are in that order.
static __global__ void __launch_bounds__(kB) k_rb_collapse(int n_nodes, const DNode *__restrict__ bn, const unsigned char *__restrict__ choice, const unsigned char *__restrict__ root4,
                                                          const uint32_t *__restrict__ id4, int n4, DNode4 *__restrict__ out, int *__restrict__ src, int *__restrict__ res) {
    for (int bi = blockIdx.x * blockDim.x + threadIdx.x; bi < n_nodes; bi += gridDim.x * blockDim.x) {
        if (!root4[bi]) continue;
        const int me = (int)id4[bi];
        if (me < 0 || me >= n4) { res[R_ERROR] = 1; continue; }
        const WideCut cut = wide_cut(bn, choice, bi);
        DNode4 d;
        d.order_lo = cut.order_lo; d.order_hi = cut.order_hi; d.codes = cut.codes;
        d._pad = 0;
        for (int k = 0; k < 4; ++k) {
            const int g = cut.slot[k];
            src[4 * (size_t)me + k] = g;
            if (g < 0) {   // absent children: inverted boxes, which fail every slab test
                d.child[k] = kNode4Empty;
                d.lox[k] = d.loy[k] = d.loz[k] = __builtin_inff();
                d.hix[k] = d.hiy[k] = d.hiz[k] = -__builtin_inff();
                continue;
            }
            if (g >= n_nodes) { res[R_ERROR] = 1; d.child[k] = kNode4Empty; continue; }
            const DNode G = bn[g];
            d.lox[k] = G.lo[0]; d.loy[k] = G.lo[1]; d.loz[k] = G.lo[2];
            d.hix[k] = G.hi0; d.hiy[k] = G.hi1; d.hiz[k] = G.hi2;
            d.child[k] = rb_is_leaf(G) ? rb_leaf_ref(G) : (int32_t)id4[g];
        }
        out[me] = d;
    }
}

// One block of kTopNodesMax threads.  new_of is -1 and placed 0 on entry; the first min(n4, kTopNodesMax) nodes of the breadth-first order
// from node 0 (the root) get their position and their flag.  A level is at most the queue's length, so one thread per entry suffices.
static __global__ void __launch_bounds__(kTopNodesMax) k_rb_bfs(const DNode4 *__restrict__ nodes4, int n4, int *__restrict__ new_of, uint32_t *__restrict__ placed, int *__restrict__ res) {
    __shared__ int q[kTopNodesMax];
    __shared__ int wsum[kTopNodesMax / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) q[0] = 0;
    int head = 0, tail = 1;
    __syncthreads();
    for (int level = 0; head < tail && tail < kTopNodesMax; ++level) {
        if (level > kTopNodesMax) { if (t == 0) res[R_ERROR] = 1; break; }   // (every level consumes an entry: not reached)
        int kids[4], cnt = 0;
        if (head + t < tail) {
            const int o = q[head + t];
            for (int k = 0; k < 4; ++k) { const int c = nodes4[o].child[k]; if (c >= 0 && c != kNode4Empty) kids[cnt++] = c; }
        }
        int inc = cnt;
        for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(inc, off); if (lane >= off) inc += y; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0, total = 0;
        for (int w = 0; w < kTopNodesMax / 64; ++w) { if (w < wave) woff += wsum[w]; total += wsum[w]; }
        const int at = tail + woff + inc - cnt;
        for (int j = 0; j < cnt; ++j) if (at + j < kTopNodesMax) q[at + j] = kids[j];
        __syncthreads();
        head = tail;
        tail = min(tail + total, kTopNodesMax);
    }
    if (t < tail) {
        const int o = q[t];
        if (o < 0 || o >= n4) res[R_ERROR] = 1;
        else { new_of[o] = t; placed[o] = 1u; }
    }
    if (t == 0) res[R_N_TOP] = tail;
}

// placed_before: the exclusive scan of `placed`.  A node outside the top block keeps its depth-first rank among those outside it.
__device__ __forceinline__ int rb_new_index(int o, const int *__restrict__ new_of, const uint32_t *__restrict__ placed_before, int n_top) {
    const int p = new_of[o];
    return p >= 0 ? p : n_top + o - (int)placed_before[o];
}
static __global__ void __launch_bounds__(kB) k_rb_renumber(int n4, const DNode4 *__restrict__ in, const int *__restrict__ src_in, const int *__restrict__ new_of,
                                                          const uint32_t *__restrict__ placed_before, DNode4 *__restrict__ out, int *__restrict__ src_out, int *res) {
    const int n_top = res[R_N_TOP];   // written by k_rb_bfs
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < n4; o += gridDim.x * blockDim.x) {
        const int i = rb_new_index(o, new_of, placed_before, n_top);
        if (i < 0 || i >= n4) { res[R_ERROR] = 1; continue; }
        DNode4 d = in[o];
        for (int k = 0; k < 4; ++k) {
            const int c = d.child[k];
            if (c >= 0 && c != kNode4Empty) d.child[k] = rb_new_index(c, new_of, placed_before, n_top);
            src_out[4 * (size_t)i + k] = src_in[4 * (size_t)o + k];
        }
        out[i] = d;
    }
}

// the leaf-order tables in the new order; absent tables are null.  new_of_old: old leaf index -> new leaf index (for the lights)
struct LeafTables {
    const DTri *tris; const uint8_t *tri_class; const int2 *tri_media; const float4 *tri_uv, *tri_n, *tri_s; const int *corner;
    DTri *tris_out; uint8_t *tri_class_out; int2 *tri_media_out; float4 *tri_uv_out, *tri_n_out, *tri_s_out; int *corner_out;
};
static __global__ void __launch_bounds__(kB) k_rb_permute(int n, const uint32_t *__restrict__ sorted, const int *__restrict__ old_of_prim, LeafTables t, int *__restrict__ new_of_old,
                                                         int *__restrict__ res) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n; li += gridDim.x * blockDim.x) {
        const uint32_t prim = sorted[li];
        if (prim >= (uint32_t)n) { res[R_ERROR] = 1; continue; }
        const int o = old_of_prim[prim];
        if (o < 0 || o >= n) { res[R_ERROR] = 1; continue; }
        new_of_old[o] = li;
        t.tris_out[li] = t.tris[o];
        t.tri_class_out[li] = t.tri_class[o];
        for (int c = 0; c < 3; ++c) t.corner_out[3 * (size_t)li + c] = t.corner[3 * (size_t)o + c];
        if (t.tri_media) t.tri_media_out[li] = t.tri_media[o];
        if (t.tri_uv) for (int c = 0; c < 2; ++c) t.tri_uv_out[2 * (size_t)li + c] = t.tri_uv[2 * (size_t)o + c];
        if (t.tri_n) for (int c = 0; c < 3; ++c) t.tri_n_out[3 * (size_t)li + c] = t.tri_n[3 * (size_t)o + c];
        if (t.tri_s) for (int c = 0; c < 3; ++c) t.tri_s_out[3 * (size_t)li + c] = t.tri_s[3 * (size_t)o + c];
    }
}

static __global__ void __launch_bounds__(kB) k_rb_lights(DLight *__restrict__ lights, int n_lights, int n_tris, const int *__restrict__ new_of_old, int *__restrict__ res) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lights; i += gridDim.x * blockDim.x) {
        const int o = lights[i].tri_leaf;
        if (o < 0) continue;   // not an area light
        if (o >= n_tris) { res[R_ERROR] = 1; continue; }
        lights[i].tri_leaf = new_of_old[o];
    }
}

static __global__ void __launch_bounds__(kB) k_rb_leafcheck(int n_nodes, const DNode *__restrict__ bn, const DTri *__restrict__ tris, int n_tris, int *__restrict__ res) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x) {
        const DNode n = bn[i];
        const int np = (int)(n.meta & 0xffffu);
        if (np > 127) res[R_LEAF_OVER_127] = 1;
        if (np != 1 || n.offset < 0 || n.offset >= n_tris) continue;
        const DTri &t = tris[n.offset];
        const float hi[3] = {n.hi0, n.hi1, n.hi2};
        for (int a = 0; a < 3; ++a) {
            const float lo_v = refit::rmin(refit::rmin(t.p0[a], t.p1[a]), t.p2[a]), hi_v = refit::rmax(refit::rmax(t.p0[a], t.p1[a]), t.p2[a]);
            if (!(lo_v == n.lo[a]) || !(hi_v == hi[a])) res[R_LEAF1_MISMATCH] = 1;
        }
    }
}

}  // namespace rebuild
}  // namespace gnxr
