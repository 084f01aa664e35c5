// bake_kernel.hip.h -- lightmap baking: the texture-space front end of SamplerIntegrator::Li (api_bake.hip.h; the definition, operation
// by operation: include/gnxr.h, "Lightmap baking").
//   k_bake_raster / k_bake_bary      atlas rasterisation: lowest covering triangle per texel centre (atomicMin), then its barycentrics
//   k_bake_leaf_of                   authoring index -> leaf index of the scene's triangles as they stand on the device
//   k_surface_rays                   (triangle, barycentrics, pixel, sample) -> cosine-distributed ray off the surface + sample record
//   k_bake_count / _scan / _scatter  the covered texels as a list in texel order (three small passes; nothing depends on launch order)
//   k_bake_rays / _accum / _finish   a sub-batch of a bake: its rays, the ordered sums of its L, the irradiance image
//   k_bake_mask / k_bake_dilate      gutter dilation, ping-pong between two images and two byte masks
// All of them are streaming kernels with grid-stride loops; every fp32 operation is written once and compiled unfused.
#pragma once
#include "kernels.hip.h"

namespace gnxr {

// ---- atlas rasterisation ----

// (b.u - a.u) * (c.v - a.v) - (b.v - a.v) * (c.u - a.u): the doubled signed area of (a, b, c); with c = P the edge function of a -> b
GX_DEV float bake_edge(float au, float av, float bu, float bv, float cu, float cv) { return (bu - au) * (cv - av) - (bv - av) * (cu - au); }

// One triangle of the lightmap uv set against one texel centre: covered or not, and the three edge values.  The box test is part of the
// definition (in exact arithmetic the edge tests imply it): it is what makes the walk over a triangle's texel box complete.
struct BakeTri {
    float u0, v0, u1, v1, u2, v2, area;
    float umin, umax, vmin, vmax;
    bool ok;   // finite uvs, area != 0
};
GX_DEV BakeTri bake_tri(const float *__restrict__ uv) {
    BakeTri t;
    t.u0 = uv[0]; t.v0 = uv[1]; t.u1 = uv[2]; t.v1 = uv[3]; t.u2 = uv[4]; t.v2 = uv[5];
    t.area = bake_edge(t.u0, t.v0, t.u1, t.v1, t.u2, t.v2);
    t.umin = fminf(t.u0, fminf(t.u1, t.u2)); t.umax = fmaxf(t.u0, fmaxf(t.u1, t.u2));
    t.vmin = fminf(t.v0, fminf(t.v1, t.v2)); t.vmax = fmaxf(t.v0, fmaxf(t.v1, t.v2));
    const bool finite = fabsf(t.u0) < GX_INF && fabsf(t.v0) < GX_INF && fabsf(t.u1) < GX_INF && fabsf(t.v1) < GX_INF && fabsf(t.u2) < GX_INF && fabsf(t.v2) < GX_INF;
    t.ok = finite && fabsf(t.area) < GX_INF && t.area != 0.f;   // (NaN fails every comparison)
    return t;
}
GX_DEV bool bake_covers(const BakeTri &t, float cu, float cv, float *wa, float *wb, float *wc) {
    *wa = bake_edge(t.u1, t.v1, t.u2, t.v2, cu, cv);
    *wb = bake_edge(t.u2, t.v2, t.u0, t.v0, cu, cv);
    *wc = bake_edge(t.u0, t.v0, t.u1, t.v1, cu, cv);
    if (!(cu >= t.umin && cu <= t.umax && cv >= t.vmin && cv <= t.vmax)) return false;
    return t.area > 0.f ? (*wa >= 0.f && *wb >= 0.f && *wc >= 0.f) : (*wa <= 0.f && *wb <= 0.f && *wc <= 0.f);
}
GX_DEV float bake_centre(int x, int W) { return ((float)x + 0.5f) / (float)W; }

// The texel columns (or rows) whose centres can lie in [lo, hi]: one texel of slack on either side covers the rounding of the products
// (W < 2^24), the clamp to the atlas comes first so that the conversion to int is always in range.  Empty: *x0 > *x1.
GX_DEV void bake_span(float lo, float hi, int W, int *x0, int *x1) {
    const float a = fminf(fmaxf(lo * (float)W, 0.f), (float)W), b = fminf(fmaxf(hi * (float)W, 0.f), (float)W);
    *x0 = max(0, (int)floorf(a) - 1);
    *x1 = min(W - 1, (int)ceilf(b) + 1);
    if (!(hi >= 0.f && lo <= 1.f)) { *x0 = 1; *x1 = 0; }   // wholly outside the atlas: centres lie in (0, 1)
}

// A wave per triangle (grid-stride over the triangles), its lanes stride the triangle's clamped texel box: small charts cost one turn,
// a chart that spans the atlas is shared by 64 lanes.  texel_tri is pre-set to 0xffffffff (-1): the unsigned minimum is the lowest index.
static __global__ void __launch_bounds__(kBlock) k_bake_raster(const float *__restrict__ lm_uv, int n_tris, int W, int H, unsigned int *__restrict__ texel_tri) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long tri = wave; tri < n_tris; tri += n_waves) {
        const BakeTri t = bake_tri(lm_uv + 6 * (size_t)tri);
        if (!t.ok) continue;
        int x0, x1, y0, y1;
        bake_span(t.umin, t.umax, W, &x0, &x1);
        bake_span(t.vmin, t.vmax, H, &y0, &y1);
        if (x0 > x1 || y0 > y1) continue;
        const long long bw = x1 - x0 + 1, cells = bw * (long long)(y1 - y0 + 1);
        for (long long c = lane; c < cells; c += 64) {
            const int x = x0 + (int)(c % bw), y = y0 + (int)(c / bw);
            float wa, wb, wc;
            if (bake_covers(t, bake_centre(x, W), bake_centre(y, H), &wa, &wb, &wc)) atomicMin(&texel_tri[(size_t)y * W + x], (unsigned int)tri);
        }
    }
}

// the barycentrics (b1, b2) of the winner at every texel centre; (0, 0) where the texel is empty
static __global__ void __launch_bounds__(kBlock) k_bake_bary(const float *__restrict__ lm_uv, const int *__restrict__ texel_tri, int W, long long n_texels, float2 *__restrict__ bary) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_texels; i += (long long)gridDim.x * blockDim.x) {
        const int tri = texel_tri[i];
        float2 b = make_float2(0.f, 0.f);
        if (tri >= 0) {
            const BakeTri t = bake_tri(lm_uv + 6 * (size_t)tri);
            float wa, wb, wc;
            (void)bake_covers(t, bake_centre((int)(i % W), W), bake_centre((int)(i / W), (int)(n_texels / W)), &wa, &wb, &wc);
            b = make_float2(wb / t.area, wc / t.area);
        }
        bary[i] = b;
    }
}

// ---- surface rays ----

// DScene::tris is in leaf order and DTri::prim names the authoring index: the inverse map, from the tables as they stand on the device
// (a rebuild or a new mesh reorders them there; the host's copy may lag)
static __global__ void __launch_bounds__(kBlock) k_bake_leaf_of(const DTri *__restrict__ tris, int n_tris, int *__restrict__ leaf_of) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int prim = tris[li].prim;
        if (prim >= 0 && prim < n_tris) leaf_of[prim] = li;
    }
}

// The ray of one record: surface_point's p, pError and geometric normal at (b1, b2) of the triangle in leaf slot `leaf`, the cosine-weighted
// direction of Halton dimensions 3 and 4 (pLens: the pair Li never draws) about the normal, the error-bounded origin.  false: degenerate
// triangle (surface_point invalid), nothing written.
GX_DEV bool surface_ray(const DTri *__restrict__ tris, const DSamplerTables &st, int leaf, float b1, float b2, int px, int py, int s, bool flip, float4 *ro, float4 *rd,
                        float4 *pos, float4 *nrm) {
    V3 p0, p1, p2;
    load_tri(tris, leaf, &p0, &p1, &p2);
    TriHit h;
    h.t = 0.f; h.b1 = b1; h.b2 = b2; h.b0 = 1.f - b1 - b2;
    const SurfacePoint sp = surface_point(p0, p1, p2, h, false);
    if (!sp.valid) return false;
    const V3 n = flip ? -sp.n : sp.n;
    const uint32_t index = halton_pixel_offset(st.h, px, py) + (uint32_t)s * (uint32_t)st.h.stride;
    const float u0 = halton_sample(st, index, 3), u1 = halton_sample(st, index, 4);
    const V3 w = cosine_sample_hemisphere(u0, u1);
    V3 ss, ts;
    coordinate_system(n, &ss, &ts);
    const V3 d = ss * w.x + ts * w.y + n * w.z;
    const V3 o = offset_ray_origin(sp.p, sp.pError, n, d);
    *ro = make_float4(o.x, o.y, o.z, GX_INF);
    *rd = make_float4(d.x, d.y, d.z, 0.f);
    *pos = make_float4(sp.p.x, sp.p.y, sp.p.z, 0.f);
    *nrm = make_float4(n.x, n.y, n.z, 0.f);
    return true;
}

// gnxr_surface_rays_device: one record per lane.  A record out of range (triangle, pixel, s < 0) is written as zeros and flagged: *bad keeps
// ~index of the first one (k_camera_rays' convention); a degenerate triangle is written as zeros and not flagged.
static __global__ void __launch_bounds__(kBlock) k_surface_rays(const DTri *__restrict__ tris, const int *__restrict__ leaf_of, int n_tris, DSamplerTables st, int W, int H,
                                                                const int *__restrict__ tri, const float2 *__restrict__ bary, const int *__restrict__ px,
                                                                const int *__restrict__ py, const int *__restrict__ s, long long n, int flip, int medium,
                                                                float4 *__restrict__ rays, int4 *__restrict__ samples, float4 *__restrict__ pn, unsigned long long *bad) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = tri[i], x = px[i], y = py[i], k = s[i];
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 ro = zero, rd = zero, pos = zero, nrm = zero;
        int4 rec = make_int4(0, 0, 0, 0);
        if (t >= 0 && t < n_tris && x >= 0 && x < W && y >= 0 && y < H && k >= 0) {
            const float2 b = bary[i];
            if (surface_ray(tris, st, leaf_of[t], b.x, b.y, x, y, k, flip != 0, &ro, &rd, &pos, &nrm)) rec = make_int4(x, y, k, medium);
            else ro = rd = pos = nrm = zero;
        } else {
            atomicMax(bad, ~(unsigned long long)i);
        }
        rays[2 * (size_t)i] = ro;
        rays[2 * (size_t)i + 1] = rd;
        samples[i] = rec;
        if (pn) { pn[2 * (size_t)i] = pos; pn[2 * (size_t)i + 1] = nrm; }
    }
}

// ---- the covered texels as a list, in texel order ----
// A tile is kBlock consecutive texels.  counts[tile] -> exclusive offsets (offsets[n_tiles] = the total) -> list[offset + rank in tile].

static __global__ void __launch_bounds__(kBlock) k_bake_count(const int *__restrict__ texel_tri, long long n_texels, int n_tiles, int *__restrict__ counts) {
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = (long long)tile * kBlock + threadIdx.x;
        const int c = __syncthreads_count(i < n_texels && texel_tri[i] >= 0);
        if (threadIdx.x == 0) counts[tile] = c;
    }
}

// one block: the running sum over the tiles, kBlock at a time
static __global__ void __launch_bounds__(kBlock) k_bake_scan(const int *__restrict__ counts, int n_tiles, int *__restrict__ offsets) {
    __shared__ int sums[kBlock];
    int carry = 0;
    for (int base = 0; base < n_tiles; base += kBlock) {
        const int i = base + threadIdx.x;
        const int c = i < n_tiles ? counts[i] : 0;
        sums[threadIdx.x] = c;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {   // inclusive scan in place
            const int add = threadIdx.x >= d ? sums[threadIdx.x - d] : 0;
            __syncthreads();
            sums[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n_tiles) offsets[i] = carry + sums[threadIdx.x] - c;
        carry += sums[kBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n_tiles] = carry;
}

static __global__ void __launch_bounds__(kBlock) k_bake_scatter(const int *__restrict__ texel_tri, long long n_texels, int n_tiles, const int *__restrict__ offsets,
                                                                int *__restrict__ list) {
    __shared__ int wave_count[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = (long long)tile * kBlock + threadIdx.x;
        const bool covered = i < n_texels && texel_tri[i] >= 0;
        const unsigned long long m = __ballot(covered);
        if (lane == 0) wave_count[wave] = __popcll(m);
        __syncthreads();
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += wave_count[w];
        if (covered) list[offsets[tile] + rank] = (int)i;
        __syncthreads();
    }
}

// ---- a sub-batch of a bake: samples [s0, s0 + ns) of the covered texels list[k0 .. k0 + nk) ----
// Record j of the batch is sample s0 + j / nk of texel list[k0 + j % nk].

// Its rays and sample records, as k_surface_rays writes them with px = x, py = y.  A texel on a degenerate triangle gets the zero-length
// ray k_raygen_rays gives a rejected record (it can hit nothing) with a valid sample record, and _pad = 1 marks it for k_bake_accum.
static __global__ void __launch_bounds__(kBlock) k_bake_rays(const DTri *__restrict__ tris, const int *__restrict__ leaf_of, DSamplerTables st, int W,
                                                             const int *__restrict__ texel_tri, const float2 *__restrict__ bary, const int *__restrict__ list, int k0, int nk,
                                                             int s0, long long n, int flip, int medium, float4 *__restrict__ rays, int4 *__restrict__ samples) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const int texel = list[k0 + (int)(j % nk)], s = s0 + (int)(j / nk);
        const int x = texel % W, y = texel / W;
        const float2 b = bary[texel];
        float4 ro, rd, pos, nrm;
        if (!surface_ray(tris, st, leaf_of[texel_tri[texel]], b.x, b.y, x, y, s, flip != 0, &ro, &rd, &pos, &nrm)) {
            ro = make_float4(0.f, 0.f, 0.f, 0.f);
            rd = make_float4(0.f, 0.f, 1.f, 1.f);
        }
        rays[2 * (size_t)j] = ro;
        rays[2 * (size_t)j + 1] = rd;
        samples[j] = make_int4(x, y, s, medium);
    }
}

// out[texel].rgb += L of the batch's samples, in sample order (the batches of a texel arrive in sample order too: the stream orders them)
static __global__ void __launch_bounds__(kBlock) k_bake_accum(const float4 *__restrict__ L, const float4 *__restrict__ rays, const int *__restrict__ list, int k0, int nk,
                                                              int ns, float4 *__restrict__ out) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nk; k += gridDim.x * blockDim.x) {
        const int texel = list[k0 + k];
        float4 acc = out[texel];
        for (int j = 0; j < ns; ++j) {
            const size_t r = (size_t)j * nk + k;
            if (rays[2 * r + 1].w != 0.f) continue;   // degenerate triangle: no radiance arrives
            const float4 l = L[r];
            acc.x += l.x; acc.y += l.y; acc.z += l.z;
        }
        out[texel] = acc;
    }
}

// sums -> irradiance: ((sum / spp) * pi, 1) where the texel is covered, (0, 0, 0, 0) elsewhere
static __global__ void __launch_bounds__(kBlock) k_bake_finish(const int *__restrict__ texel_tri, long long n_texels, int spp, float4 *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_texels; i += (long long)gridDim.x * blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (texel_tri[i] >= 0) {
            const float4 a = out[i];
            v = make_float4((a.x / (float)spp) * GX_PI, (a.y / (float)spp) * GX_PI, (a.z / (float)spp) * GX_PI, 1.f);
        }
        out[i] = v;
    }
}

// ---- gutter dilation ----

static __global__ void __launch_bounds__(kBlock) k_bake_mask(const float4 *__restrict__ img, long long n_texels, unsigned char *__restrict__ mask) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_texels; i += (long long)gridDim.x * blockDim.x) mask[i] = img[i].w > 0.f ? 1 : 0;
}

// One pass: reads (src, src_mask) only.  A filled texel is copied; an unfilled one with filled 8-neighbours takes the mean of their rgb,
// added in (dy, dx) ascending order and divided by their count, keeps its alpha and becomes filled.
static __global__ void __launch_bounds__(kBlock) k_bake_dilate(const float4 *__restrict__ src, const unsigned char *__restrict__ src_mask, int W, int H,
                                                               float4 *__restrict__ dst, unsigned char *__restrict__ dst_mask) {
    const long long n_texels = (long long)W * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_texels; i += (long long)gridDim.x * blockDim.x) {
        float4 v = src[i];
        unsigned char filled = src_mask[i];
        if (!filled) {
            const int x = (int)(i % W), y = (int)(i / W);
            float r = 0.f, g = 0.f, b = 0.f;
            int count = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx, yy = y + dy;
                    if ((dx == 0 && dy == 0) || xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                    const long long q = (long long)yy * W + xx;
                    if (!src_mask[q]) continue;
                    const float4 nb = src[q];
                    r += nb.x; g += nb.y; b += nb.z;
                    ++count;
                }
            if (count > 0) {
                v = make_float4(r / (float)count, g / (float)count, b / (float)count, v.w);
                filled = 1;
            }
        }
        dst[i] = v;
        dst_mask[i] = filled;
    }
}

}  // namespace gnxr
