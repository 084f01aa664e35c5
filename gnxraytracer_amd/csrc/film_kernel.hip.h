// film_kernel.hip.h -- the film: pixel reconstruction filters on device memory (the definition: include/gnxr.h, "Film").
//
// Two kernels, both pure image operations:
//   k_film_add<HALTON>   the gather form of pbrt-v3's Film::AddSample: one lane per DESTINATION pixel, which keeps its (Sr, Sg, Sb, Wt) in
//                        registers, loops over the sample layers and, per layer, over the source pixels whose sample can reach it, in the
//                        order the definition fixes -- layer, then source row, then source column, ascending.  No atomics, and a pixel's sum
//                        does not depend on how the image is tiled or the layers are batched.
//                        A work-group is a 16 x 16 tile of destinations.  Per layer it stages the source records of the tile and of the
//                        halo around it (ceil(r + 0.5) pixels per side: 26 x 26 records at radius 4) in LDS: (L.r, L.g, L.b, dx) and dy,
//                        dx = (qx + ux) - 0.5 being the sample's continuous film position.  A source outside the view's image, or a sample
//                        whose offset is outside [0, 1] or NaN, is staged with dx = NaN: every tap on it fails the window test, so nothing
//                        crosses from one view into another and the lanes' loops need no clipping.  The 16 x 16 filter table sits in LDS too.
//                        HALTON = false: the film offsets come from caller memory (gnxr_film_add_device).  HALTON = true: they are
//                        dimensions 0 and 1 of the render's Halton sample, computed with device_sampler.h while the tile is loaded
//                        (gnxr_render_filtered_device): the path state carries no per-path film position.
//   k_film_resolve       one lane per pixel: S / Wt, 0 where Wt == 0 or the quotient is negative.
// The window test: the definition's x0 <= x < x1 with x0 = (int)ceilf(dx - rx), x1 = (int)floorf(dx + rx) + 1 is, for an integer x,
// dx - rx <= (float)x <= dx + rx on the same rounded sums (x >= ceil(t) <=> x >= t; x <= floor(u) <=> x <= u), and false for a NaN.
// Every operation is a single fp32 operation in the order gnxr.h writes (the library is built with -ffp-contract=off).
#pragma once
#include "kernels.hip.h"

namespace gnxr {

constexpr int kFilmTile = 16, kFilmMaxHalo = 5, kFilmTileMax = kFilmTile + 2 * kFilmMaxHalo;
constexpr int kFilmRecsPerLane = (kFilmTileMax * kFilmTileMax + kBlock - 1) / kBlock;
static_assert(kFilmTile * kFilmTile == kBlock, "a work-group is one tile: thread t is pixel (t % 16, t / 16) of it, and loads entry t of the 256-entry table");

struct FilmImage {
    int W, H;
    long long npix;      // n_views * W * H: the stride of a layer
    long long n_tiles;   // n_views * tiles_y * tiles_x
    int tiles_x, tiles_y;
};
struct FilmFilter {
    float rx, ry, inv_rx, inv_ry;   // inv = 1.f / r
    int hx, hy;                     // halo: ceil(r + 0.5) source pixels per side
};
struct FilmTable { float v[256]; };   // travels as a kernel argument: no allocation, nothing to order on the stream

template <bool HALTON>
__global__ void __launch_bounds__(kBlock) k_film_add(FilmImage im, FilmFilter f, FilmTable tab, const float4 *__restrict__ L, const float2 *__restrict__ offsets,
                                                      DSamplerTables st, int s0, int n_layers, float4 *accum) {
    __shared__ float s_table[256];
    __shared__ float4 s_rec[kFilmTileMax * kFilmTileMax];   // (L.r, L.g, L.b, dx)
    __shared__ float s_dy[kFilmTileMax * kFilmTileMax];
    s_table[threadIdx.x] = tab.v[threadIdx.x];
    const int lx = threadIdx.x & (kFilmTile - 1), ly = threadIdx.x / kFilmTile;
    const int W = im.W, H = im.H, tw = kFilmTile + 2 * f.hx, th = kFilmTile + 2 * f.hy, n_rec = tw * th;
    const float qnan = __uint_as_float(0x7fc00000u);
    for (long long t = blockIdx.x; t < im.n_tiles; t += gridDim.x) {
        const int tx = (int)(t % im.tiles_x);
        const long long tr = t / im.tiles_x;
        const int ty = (int)(tr % im.tiles_y);
        const long long view = tr / im.tiles_y;
        const int x = tx * kFilmTile + lx, y = ty * kFilmTile + ly;
        const long long base = view * H * (long long)W;   // pixel 0 of the view: no record of the tile comes from outside [base, base + W * H)
        const bool inside = x < W && y < H;
        const long long p = base + (long long)y * W + x;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inside) a = accum[p];
        // the records this lane stages in every layer: tile entry threadIdx.x + k * kBlock
        long long rq[kFilmRecsPerLane];      // its pixel, -1 outside the image
        float rqx[kFilmRecsPerLane], rqy[kFilmRecsPerLane];
        uint32_t roff[kFilmRecsPerLane];     // HALTON: the pixel's first Halton index
#pragma unroll
        for (int k = 0; k < kFilmRecsPerLane; ++k) {
            const int i = threadIdx.x + k * kBlock;
            const int iy = i / tw, ix = i - iy * tw;
            const int qx = tx * kFilmTile - f.hx + ix, qy = ty * kFilmTile - f.hy + iy;
            const bool in = i < n_rec && qx >= 0 && qx < W && qy >= 0 && qy < H;
            rq[k] = in ? base + (long long)qy * W + qx : -1;
            rqx[k] = (float)qx; rqy[k] = (float)qy;
            roff[k] = (HALTON && in) ? halton_pixel_offset(st.h, qx, qy) : 0u;
        }
        const float fxp = (float)x, fyp = (float)y;
        for (int j = 0; j < n_layers; ++j) {
            __syncthreads();   // the taps of the previous layer (or tile) are done
#pragma unroll
            for (int k = 0; k < kFilmRecsPerLane; ++k) {
                const int i = threadIdx.x + k * kBlock;
                if (i >= n_rec) continue;
                float4 rec = make_float4(0.f, 0.f, 0.f, qnan);
                float dy = qnan;
                if (rq[k] >= 0) {
                    const size_t src = (size_t)j * (size_t)im.npix + (size_t)rq[k];
                    const float4 l = L[src];
                    float ux, uy;
                    if (HALTON) {
                        const uint32_t index = roff[k] + (uint32_t)(s0 + j) * (uint32_t)st.h.stride;
                        ux = halton_sample(st, index, 0);
                        uy = halton_sample(st, index, 1);
                    } else {
                        const float2 u = offsets[src];
                        ux = u.x; uy = u.y;
                    }
                    if (ux >= 0.f && ux <= 1.f && uy >= 0.f && uy <= 1.f) {   // (a NaN fails)
                        rec = make_float4(l.x, l.y, l.z, (rqx[k] + ux) - 0.5f);
                        dy = (rqy[k] + uy) - 0.5f;
                    }
                }
                s_rec[i] = rec;
                s_dy[i] = dy;
            }
            __syncthreads();
            if (!inside) continue;
            // the lane's own record is entry (lx + hx, ly + hy): its window is the (2 hx + 1) x (2 hy + 1) entries from (lx, ly) on
            for (int iy = ly; iy <= ly + 2 * f.hy; ++iy) {
                const int row = iy * tw;
                for (int ix = lx; ix <= lx + 2 * f.hx; ++ix) {
                    const float dy = s_dy[row + ix];
                    const float4 r = s_rec[row + ix];
                    const float dx = r.w;
                    if (!(fxp >= dx - f.rx && fxp <= dx + f.rx && fyp >= dy - f.ry && fyp <= dy + f.ry)) continue;
                    const float fx = fabsf((fxp - dx) * f.inv_rx * 16.f), fy = fabsf((fyp - dy) * f.inv_ry * 16.f);
                    const int ifx = min((int)floorf(fx), 15), ify = min((int)floorf(fy), 15);
                    const float w = s_table[ify * 16 + ifx];
                    a.x = a.x + r.x * w; a.y = a.y + r.y * w; a.z = a.z + r.z * w;
                    a.w = a.w + w;
                }
            }
        }
        if (inside) accum[p] = a;
    }
}

// out = (c(Sr), c(Sg), c(Sb), 1), c(S) = 0 where Wt == 0, else S / Wt -- 0 where that is negative; a NaN stays
GX_DEV float film_channel(float s, float wt) {
    if (wt == 0.f) return 0.f;
    const float t = s / wt;
    return t < 0.f ? 0.f : t;
}
// (every lane reads its own pixel before it writes it: `out` may be `accum`)
static __global__ void __launch_bounds__(kBlock) k_film_resolve(const float4 *accum, long long npix, float4 *out) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const float4 a = accum[p];
        out[p] = make_float4(film_channel(a.x, a.w), film_channel(a.y, a.w), film_channel(a.z, a.w), 1.f);
    }
}

}  // namespace gnxr
