// denoise_kernel.hip.h -- the edge-avoiding a-trous wavelet filter of gnxr_denoise_device (the definition: include/gnxr.h).
//
// Two kernels, both pure image operations on device memory:
//   k_denoise_prepare   one lane per pixel: reads the colour share(s) and the guides once, demodulates by the albedo and writes the 16-byte
//                       work record (c.rgb, v) -- (0, 0, 0, -1) for an invalid pixel -- and the 16-byte guide record (n.xyz, depth)
//   k_denoise_atrous    one launch per iteration i (step s = 2^i), templated on <second image, normal term, depth term>: the 3 x 3 variance
//                       window at distance 1 (second image only), the 25 taps at distance s, the new record -- or, in the last iteration,
//                       the remodulated pixel straight into d_rgba_out
// A work-group is 64 x 4 pixels and its wave w covers 64 consecutive pixels of row 4 ty + w, so every tap of every step is one contiguous
// 1 KB dwordx4 load per record and wave whatever the step is.  The kernel is bound by the latency of those loads, not by their bytes
// (DESIGN.md section 4): steps 1 and 2 read their taps from a tile in LDS (the tile and 2 s pixels around it, 17 and 27 KB), the wider
// steps issue the ten loads of a tap row together before they weigh them; the reuse across rows is left to L1 and L2.  The records of
// a whole call (48 bytes per pixel) stay in the Infinity Cache up to 5.5 M pixels.
// Every operation is a single fp32 operation in the order gnxr.h writes (the library is built with -ffp-contract=off); a pixel is invalid
// exactly while the w of its work record is negative: a variance is a square, or a quotient of sums of squares, and never is.
#pragma once
#include "kernels.hip.h"

namespace gnxr {

constexpr int kDenoiseTileW = 64, kDenoiseTileH = 4;
static_assert(kDenoiseTileW * kDenoiseTileH == kBlock && kDenoiseTileW == 64, "a work-group is one tile: thread t is pixel (t % 64, t / 64) of it, a wave one row");

struct DenoiseImage {
    int W, H;
    long long n_tiles;   // n_views * tiles_y * tiles_x
    int tiles_x, tiles_y;
};

GX_DEV float denoise_lum(float r, float g, float b) { return (0.212671f * r + 0.715160f * g) + 0.072169f * b; }
// div = max(albedo + (1 - coverage), 1/1024) per channel, a NaN giving 1/1024; 1 without an albedo buffer
GX_DEV void denoise_divisor(const float4 *__restrict__ albedo, long long p, float *dr, float *dg, float *db) {
    *dr = *dg = *db = 1.f;
    if (!albedo) return;
    const float4 al = albedo[p];
    const float miss = 1.f - al.w, lo = 1.f / 1024.f;
    const float r = al.x + miss, g = al.y + miss, b = al.z + miss;
    *dr = r > lo ? r : lo; *dg = g > lo ? g : lo; *db = b > lo ? b : lo;
}

static __global__ void __launch_bounds__(kBlock) k_denoise_prepare(const float4 *a, const float4 *b, const float4 *__restrict__ albedo, const float4 *__restrict__ normal,
                                                                    const float *__restrict__ depth, long long npix, float4 *__restrict__ work, float4 *__restrict__ guide) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        float dr, dg, db;
        denoise_divisor(albedo, p, &dr, &dg, &db);
        const float4 ca = a[p];
        float cr, cg, cb, v = 0.f;
        if (b) {
            const float4 cb4 = b[p];
            cr = (ca.x + cb4.x) / dr; cg = (ca.y + cb4.y) / dg; cb = (ca.z + cb4.z) / db;
            const float d = denoise_lum(ca.x / dr, ca.y / dg, ca.z / db) - denoise_lum(cb4.x / dr, cb4.y / dg, cb4.z / db);
            v = d * d;
        } else {
            cr = ca.x / dr; cg = ca.y / dg; cb = ca.z / db;
        }
        const bool ok = gx_finite(cr) && gx_finite(cg) && gx_finite(cb) && gx_finite(v);
        work[p] = ok ? make_float4(cr, cg, cb, v) : make_float4(0.f, 0.f, 0.f, -1.f);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (normal) { const float4 n = normal[p]; g.x = n.x; g.y = n.y; g.z = n.z; }
        if (depth) g.w = depth[p];
        guide[p] = g;
    }
}

struct DenoiseStep {
    int step;            // 2^i
    int use_color;       // sigma_color > 0
    int last;            // the last iteration: remodulate into `out`
    float sigma_color;   // second image: inv_c = 1 / (sigma_color * sqrt(vbar) + 1e-6f)
    float inv_sc_i;      // no second image: inv_sc * 4^i
    float inv_sn;
    float sigma_z_step;  // sigma_depth * (float)step
};

// `a`, `b` and `out` are only touched in the last iteration, each at the lane's own pixel and read before written: `out` may be `a` or `b`.
// S == 0: every tap is a load from global memory, whatever the step is.  S == 1, 2: the kernel of step S keeps the records of its tile and
// of the 2 S pixels around it in LDS -- a pixel outside the image as an invalid record, which the taps skip as they skip it there.
template <bool B, bool N, bool Z, int S>
__global__ void __launch_bounds__(kBlock) k_denoise_atrous(DenoiseImage im, DenoiseStep st, const float4 *__restrict__ src, const float4 *__restrict__ guide,
                                                            float4 *__restrict__ dst, const float4 *a, const float4 *b, const float4 *__restrict__ albedo, float4 *out) {
    constexpr int kHalo = 2 * S, kTW = kDenoiseTileW + 2 * kHalo, kTH = kDenoiseTileH + 2 * kHalo;
    __shared__ float4 s_work[S ? kTW * kTH : 1];
    __shared__ float4 s_guide[S && (N || Z) ? kTW * kTH : 1];
    const int lx = threadIdx.x & (kDenoiseTileW - 1), ly = threadIdx.x / kDenoiseTileW;
    const int W = im.W, H = im.H, s = S ? S : st.step;
    for (long long t = blockIdx.x; t < im.n_tiles; t += gridDim.x) {
        const int tx = (int)(t % im.tiles_x);
        const long long tr = t / im.tiles_x;
        const int ty = (int)(tr % im.tiles_y);
        const long long view = tr / im.tiles_y;
        const int x = tx * kDenoiseTileW + lx, y = ty * kDenoiseTileH + ly;
        const long long base = view * H * (long long)W;   // pixel 0 of the view: no tap leaves [base, base + W * H)
        if (S) {
            __syncthreads();   // the taps of the block's previous tile are done
            for (int i = threadIdx.x; i < kTW * kTH; i += kBlock) {
                const int iy = i / kTW, ix = i - iy * kTW;
                const int qx = tx * kDenoiseTileW - kHalo + ix, qy = ty * kDenoiseTileH - kHalo + iy;
                const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const long long q = base + (long long)qy * W + qx;
                s_work[i] = in ? src[q] : make_float4(0.f, 0.f, 0.f, -1.f);
                if (N || Z) s_guide[i] = in ? guide[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __syncthreads();
        }
        if (x >= W || y >= H) continue;
        const int c0 = (ly + kHalo) * kTW + lx + kHalo;   // the lane's own record in the tile
        const long long p = base + (long long)y * W + x;
        const float4 cp = S ? s_work[c0] : src[p];
        const bool p_ok = !(cp.w < 0.f);
        float4 gp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (N || Z) gp = S ? s_guide[c0] : guide[p];
        const bool color = st.use_color != 0 && p_ok;
        float inv_c = 0.f, lum_p = 0.f, inv_z = 0.f;
        if (B && color) {
            float sgv = 0.f, sg = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    float vq;
                    if (S) {
                        vq = s_work[c0 + dy * kTW + dx].w;
                    } else {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        vq = src[base + (long long)qy * W + qx].w;
                    }
                    if (vq < 0.f) continue;
                    const float g = (dy == 0 ? 0.25f : 0.125f) * (dx == 0 ? 1.f : 0.5f);
                    sgv += g * vq;
                    sg += g;
                }
            }
            const float vbar = sg > 0.f ? sgv / sg : 0.f;
            inv_c = 1.f / (st.sigma_color * gx_sqrt(vbar) + 1e-6f);
            lum_p = denoise_lum(cp.x, cp.y, cp.z);
        }
        if (Z) inv_z = 1.f / (st.sigma_z_step * gp.w + 1e-20f);
        float sr = 0.f, sgc = 0.f, sb = 0.f, sw = 0.f, sv = 0.f;
        // one valid tap q: its weight and its share of the sums
        auto tap = [&](const float4 cq, const float4 gq, float h) {
            float xc = 0.f, xn = 0.f, xz = 0.f;
            if (color) {
                if (B) {
                    xc = fabsf(lum_p - denoise_lum(cq.x, cq.y, cq.z)) * inv_c;
                } else {
                    const float er = cp.x - cq.x, eg = cp.y - cq.y, eb = cp.z - cq.z;
                    xc = ((er * er + eg * eg) + eb * eb) * st.inv_sc_i;
                }
            }
            if (N) {
                const float ex = gp.x - gq.x, ey = gp.y - gq.y, ez = gp.z - gq.z;
                xn = ((ex * ex + ey * ey) + ez * ez) * st.inv_sn;
            }
            if (Z) xz = fabsf(gp.w - gq.w) * inv_z;
            const float w = h * gx_exp(-((xc + xn) + xz));
            if (!(w > 0.f)) return;
            sr += w * cq.x; sgc += w * cq.y; sb += w * cq.z;
            sw += w;
            sv += (w * w) * cq.w;
        };
        if (S) {
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
                const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int q = c0 + S * dy * kTW + S * dx;
                    const float4 cq = s_work[q];
                    if (cq.w < 0.f) continue;
                    tap(cq, N || Z ? s_guide[q] : gp, ky * (dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f)));
                }
            }
        } else {
            for (int dy = -2; dy <= 2; ++dy) {
                const int qy = y + s * dy;
                if (qy < 0 || qy >= H) continue;
                const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
                const long long row = base + (long long)qy * W;
                // the row's ten loads first, at addresses clamped into the row, so that they are in flight together; then its taps
                float4 cq[5], gq[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int cx = min(max(x + s * (k - 2), 0), W - 1);
                    cq[k] = src[row + cx];
                    if (N || Z) gq[k] = guide[row + cx];
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int qx = x + s * (k - 2);
                    if (qx < 0 || qx >= W || cq[k].w < 0.f) continue;
                    tap(cq[k], N || Z ? gq[k] : gp, ky * (k == 2 ? 0.375f : (k == 1 || k == 3 ? 0.25f : 0.0625f)));
                }
            }
        }
        float4 r = cp;
        if (sw > 0.f) r = make_float4(sr / sw, sgc / sw, sb / sw, sv / (sw * sw));
        if (!st.last) { dst[p] = r; continue; }
        const float4 ca = a[p];
        float4 o;
        if (!(r.w < 0.f)) {
            float dr, dg, db;
            denoise_divisor(albedo, p, &dr, &dg, &db);
            o = make_float4(r.x * dr, r.y * dg, r.z * db, ca.w);
        } else if (B) {
            const float4 cb = b[p];
            o = make_float4(ca.x + cb.x, ca.y + cb.y, ca.z + cb.z, ca.w);
        } else {
            o = ca;
        }
        out[p] = o;
    }
}

}  // namespace gnxr
