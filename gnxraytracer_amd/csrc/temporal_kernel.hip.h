// temporal_kernel.hip.h -- temporal accumulation (the definition: include/gnxr.h, "Temporal accumulation"): where every pixel's surface
// point was on the previous frame's film (gnxr_motion_device) and the validated, reprojected blend of a frame into its history
// (gnxr_temporal_accumulate_device).
//
//   k_motion<0>   one lane per pixel: the ray through the pixel centre -- camera_ray's operations for the film sample (0.5, 0.5) of a
//                 pinhole, no sampler table read -- as a gnxr_ray record, 32 bytes, with the leaf code "nothing" (-1) in its pad word
//   k_trace4      the 4-wide walk in its closest-hit query form (closest_hit_codes, api_query.hip.h), exactly as gnxr_trace_closest_device
//                 drives it.  As for the feature buffers (aov_kernel.hip.h) its one-int-per-32-bytes result array is handed the address
//                 of ray 0's pad word: every ray's leaf code lands in that ray's own record, and a ray is the whole scratch of a pixel
//   k_motion<1>   one lane per pixel: the hit rebuilt from the leaf code the way k_query_finish does (tri_hit_recompute / sphere_test, then
//                 hit_record: the bits of gnxr_trace_closest_device), the hit triangle's previous corners through the refit's corner ->
//                 vertex table, the projection with the previous camera's WorldToRaster, the expected previous depth
//   k_temporal_accumulate   one lane per pixel, a pure image operation: up to four history taps, each validated against this frame's
//                 primitive, depth and normal, then the blend.  Every record is one dwordx4 (the primitive ids one dword); a wave covers
//                 64 consecutive pixels of a row, so its current-frame loads and its stores are contiguous 1 KB rows and the four taps of
//                 neighbouring lanes fall into the same cache lines: per pixel 52 B of history, 52 B of this frame and 32 B of output are
//                 unique.  The loads of a pixel's four taps are issued together, before any of them is weighed.
// Every operation is a single fp32 operation in the order gnxr.h writes (the library is built with -ffp-contract=off; division and sqrt
// are IEEE).
#pragma once
#include "query_kernel.hip.h"

namespace gnxr {

// one view of a gnxr_motion_device call: this frame's camera and what the projection needs of the previous frame's
struct MotionView {
    DCamera cam;
    float w2r[16];       // WorldToRaster of the previous camera (gnxr_camera_matrices)
    float eye[3];        // E' = (c2w'[3], c2w'[7], c2w'[11])
    int32_t prev_ortho;
};

struct MotionOut {
    float4 *motion, *guide;
    int *prim;
};

// camera_ray (kernels.hip.h) for the film sample (fx, fy) = (0.5, 0.5) and lens_radius taken as 0: the same operations in the same order,
// without the sampler.  tMax is the caller's (+inf).
GX_DEV void camera_ray_centre(const DCamera &cam, int px, int py, V3 *o, V3 *d) {
    const float pfx = (float)px + 0.5f, pfy = (float)py + 0.5f;
    V3 pCamera = xform_point(cam.r2c, V3(pfx, pfy, 0));
    V3 dir = normalize(V3(pCamera.x, pCamera.y, pCamera.z));
    V3 oc(0, 0, 0), dc = dir;
    if (cam.ortho) { oc = pCamera; dc = V3(0, 0, 1); }
    const float *m = cam.c2w;
    float x = oc.x, y = oc.y, z = oc.z;
    float xp = (m[0] * x + m[1] * y) + (m[2] * z + m[3]);
    float yp = (m[4] * x + m[5] * y) + (m[6] * z + m[7]);
    float zp = (m[8] * x + m[9] * y) + (m[10] * z + m[11]);
    float wp = (m[12] * x + m[13] * y) + (m[14] * z + m[15]);
    float xAbs = (fabsf(m[0] * x) + fabsf(m[1] * y) + fabsf(m[2] * z) + fabsf(m[3]));
    float yAbs = (fabsf(m[4] * x) + fabsf(m[5] * y) + fabsf(m[6] * z) + fabsf(m[7]));
    float zAbs = (fabsf(m[8] * x) + fabsf(m[9] * y) + fabsf(m[10] * z) + fabsf(m[11]));
    V3 oError = GX_GAMMA(3) * V3(xAbs, yAbs, zAbs);
    V3 ow = (wp == 1) ? V3(xp, yp, zp) : V3((1.f / wp) * xp, (1.f / wp) * yp, (1.f / wp) * zp);
    V3 dw = xform_vector(m, dc);
    float lengthSquared = length_sq(dw);
    if (lengthSquared > 0) {
        float dt = dot(vabs(dw), oError) / lengthSquared;
        ow = ow + dw * dt;
    }
    *o = ow; *d = dw;
}

// STEP 0: rays[2 lp], rays[2 lp + 1] = (o.xyz, +inf), (d.xyz, leaf code -1) for pixel lp = (view * H + y) * W + x.
// STEP 1: the three channels of pixel lp from its ray and the leaf code the traversal left in the ray's pad word.  corner: 3 authored
// vertices per leaf-order triangle (CompiledScene::corner_vertex); prev_xyz: the vertex array of one frame ago, or nullptr.
template <int STEP>
__global__ void __launch_bounds__(kBlock) k_motion(DScene sc, const MotionView *__restrict__ views, int W, int H, int npix, float4 *rays, const int *__restrict__ corner,
                                                   const float *__restrict__ prev_xyz, MotionOut out) {
    const int wh = W * H;
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < npix; lp += gridDim.x * blockDim.x) {
        const int view = lp / wh, p = lp - view * wh;
        const int py = p / W, px = p - py * W;
        const MotionView &mv = views[view];
        if (STEP == 0) {
            V3 o, d;
            camera_ray_centre(mv.cam, px, py, &o, &d);
            rays[2 * (size_t)lp] = make_float4(o.x, o.y, o.z, GX_INF);
            rays[2 * (size_t)lp + 1] = make_float4(d.x, d.y, d.z, __int_as_float(-1));
            continue;
        }
        const float4 o4 = rays[2 * (size_t)lp], d4 = rays[2 * (size_t)lp + 1];
        const V3 ro(o4.x, o4.y, o4.z), rd(d4.x, d4.y, d4.z);
        const int code = __float_as_int(d4.w);   // a leaf-order triangle, -1 nothing, -2 - i sphere i
        // (t, b0, b1, b2) as k_query_finish recomputes them
        TriHit h = {0.f, 0.f, 0.f, 0.f};
        if (code >= 0) {
            V3 p0, p1, p2;
            load_tri(sc.tris, code, &p0, &p1, &p2);
            tri_hit_recompute(p0, p1, p2, ro, rd, &h);
        } else if (code < -1) {
            (void)sphere_test(sc.spheres[-2 - code], ro, rd, o4.w, &h.t);
        }
        const gnxr_hit rec = hit_record(sc, ro, rd, code, h);
        if (out.guide) out.guide[lp] = make_float4(rec.n[0], rec.n[1], rec.n[2], rec.t);   // (hit_record leaves a miss at zeros)
        if (out.prim) out.prim[lp] = rec.prim;
        if (!out.motion) continue;
        const V3 eye(mv.eye[0], mv.eye[1], mv.eye[2]);
        const bool miss = code == -1;
        V3 q;   // P': where the surface point was one frame ago
        if (miss) {
            q = mv.cam.ortho ? ro : V3(eye.x + rd.x, eye.y + rd.y, eye.z + rd.z);
        } else if (code >= 0 && prev_xyz) {
            const int v0 = corner[3 * (size_t)code], v1 = corner[3 * (size_t)code + 1], v2 = corner[3 * (size_t)code + 2];
            const float *a = prev_xyz + 3 * (size_t)v0, *b = prev_xyz + 3 * (size_t)v1, *c = prev_xyz + 3 * (size_t)v2;
            q = V3((rec.b0 * a[0] + rec.b1 * b[0]) + rec.b2 * c[0], (rec.b0 * a[1] + rec.b1 * b[1]) + rec.b2 * c[1], (rec.b0 * a[2] + rec.b1 * b[2]) + rec.b2 * c[2]);
        } else {
            q = V3(ro.x + rec.t * rd.x, ro.y + rec.t * rd.y, ro.z + rec.t * rd.z);
        }
        const float *m = mv.w2r;
        const float xr = (m[0] * q.x + m[1] * q.y) + (m[2] * q.z + m[3]);
        const float yr = (m[4] * q.x + m[5] * q.y) + (m[6] * q.z + m[7]);
        const float zr = (m[8] * q.x + m[9] * q.y) + (m[10] * q.z + m[11]);
        const float w = (m[12] * q.x + m[13] * q.y) + (m[14] * q.z + m[15]);
        float xq = xr, yq = yr;
        if (!(w == 1.f)) { xq = xr / w; yq = yr / w; }
        float tq = 0.f;   // the distance the previous frame's guide holds there if it saw the same point
        if (!miss) {
            if (mv.prev_ortho) {
                tq = zr * 10.f;
            } else {
                const V3 e(q.x - eye.x, q.y - eye.y, q.z - eye.z);
                tq = gx_sqrt((e.x * e.x + e.y * e.y) + e.z * e.z);
            }
        }
        const bool ok = w > 0.f && gx_finite(xq) && gx_finite(yq) && gx_finite(tq);
        out.motion[lp] = ok ? make_float4(xq, yq, tq, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

struct TemporalArrays {
    const float4 *color, *motion, *guide;
    const int *prim;
    const float4 *hist_color, *hist_stat, *hist_guide;   // all null on the first frame
    const int *hist_prim;
    float4 *out_color, *out_stat;
};
struct TemporalParams {
    int W, H;
    long long npix;       // n_views * H * W
    float max_history;    // (float)max_history
    float depth_tol, normal_cos;
};

// one history tap, loaded whether it will count or not (from the lane's own pixel when it lies outside the image: `inside` says so)
struct TemporalTap {
    float4 c, s, g;
    int prim;
    float b;
    bool inside;
};
GX_DEV TemporalTap temporal_tap(const TemporalArrays &a, long long view_base, long long own, int W, int H, int qx, int qy, float b) {
    TemporalTap t;
    t.inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
    const long long q = t.inside ? view_base + (long long)qy * W + qx : own;
    t.s = a.hist_stat[q];
    t.prim = a.hist_prim[q];
    t.c = a.hist_color[q];
    t.g = a.hist_guide[q];
    t.b = b;
    return t;
}
struct TemporalSums { float sw, cr, cg, cb, s1, s2, sN; };
GX_DEV void temporal_weigh(const TemporalTap &t, int prim, float4 g, float tq, const TemporalParams &tp, TemporalSums *s) {
    bool ok = t.b > 0.f && t.inside && t.s.z > 0.f && t.prim == prim;
    ok = ok && gx_finite(t.c.x) && gx_finite(t.c.y) && gx_finite(t.c.z) && gx_finite(t.s.x) && gx_finite(t.s.y);
    if (prim >= 0) {
        ok = ok && fabsf(t.g.w - tq) <= tp.depth_tol * tq;
        ok = ok && ((g.x * t.g.x + g.y * t.g.y) + g.z * t.g.z) >= tp.normal_cos;
    }
    if (!ok) return;
    s->sw += t.b;
    s->cr += t.b * t.c.x; s->cg += t.b * t.c.y; s->cb += t.b * t.c.z;
    s->s1 += t.b * t.s.x;
    s->s2 += t.b * t.s.y;
    s->sN += t.b * t.s.z;
}
GX_DEV float temporal_variance(float m1, float m2) {
    const float v = m2 - m1 * m1;
    return v > 0.f ? v : 0.f;
}

static __global__ void __launch_bounds__(kBlock) k_temporal_accumulate(TemporalArrays a, TemporalParams tp) {
    const int W = tp.W, H = tp.H;
    const long long wh = (long long)W * H;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < tp.npix; p += (long long)gridDim.x * blockDim.x) {
        const float4 c = a.color[p];
        const float l = (0.212671f * c.x + 0.715160f * c.y) + 0.072169f * c.z;
        const bool cur_ok = gx_finite(c.x) && gx_finite(c.y) && gx_finite(c.z);
        TemporalSums s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.hist_color) {   // uniform
            const float4 mo = a.motion[p];
            if (mo.w != 0.f) {
                float fx = mo.x - 0.5f, fy = mo.y - 0.5f;
                const float rx = rintf(fx), ry = rintf(fy);
                if (fabsf(fx - rx) <= 0.00390625f) fx = rx;
                if (fabsf(fy - ry) <= 0.00390625f) fy = ry;
                // in float, before any conversion: NaN, inf and 1e30 fail here and never become an index
                if (fx >= -1.f && fx < (float)W && fy >= -1.f && fy < (float)H) {
                    const float4 g = a.guide[p];
                    const int prim = a.prim[p];
                    const long long view = p / wh, base = view * wh;
                    const float x0 = floorf(fx), y0 = floorf(fy);
                    const float ax = fx - x0, ay = fy - y0;
                    const float bx = 1.f - ax, by = 1.f - ay;
                    const int ix = (int)x0, iy = (int)y0;
                    const TemporalTap t00 = temporal_tap(a, base, p, W, H, ix, iy, bx * by);
                    const TemporalTap t10 = temporal_tap(a, base, p, W, H, ix + 1, iy, ax * by);
                    const TemporalTap t01 = temporal_tap(a, base, p, W, H, ix, iy + 1, bx * ay);
                    const TemporalTap t11 = temporal_tap(a, base, p, W, H, ix + 1, iy + 1, ax * ay);
                    temporal_weigh(t00, prim, g, mo.z, tp, &s);
                    temporal_weigh(t10, prim, g, mo.z, tp, &s);
                    temporal_weigh(t01, prim, g, mo.z, tp, &s);
                    temporal_weigh(t11, prim, g, mo.z, tp, &s);
                }
            }
        }
        float4 oc = make_float4(0.f, 0.f, 0.f, c.w), os = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s.sw > 0.f) {
            const float hr = s.cr / s.sw, hg = s.cg / s.sw, hb = s.cb / s.sw;
            const float M1 = s.s1 / s.sw, M2 = s.s2 / s.sw, N = s.sN / s.sw;
            if (cur_ok) {
                const float n1 = N + 1.f;
                const float Nn = n1 < tp.max_history ? n1 : tp.max_history;
                const float alpha = 1.f / Nn;
                oc.x = hr + alpha * (c.x - hr); oc.y = hg + alpha * (c.y - hg); oc.z = hb + alpha * (c.z - hb);
                const float m1 = M1 + alpha * (l - M1), m2 = M2 + alpha * (l * l - M2);
                os = make_float4(m1, m2, Nn, temporal_variance(m1, m2));
            } else {
                oc.x = hr; oc.y = hg; oc.z = hb;
                os = make_float4(M1, M2, N, temporal_variance(M1, M2));
            }
        } else if (cur_ok) {
            oc.x = c.x; oc.y = c.y; oc.z = c.z;
            os = make_float4(l, l * l, 1.f, 0.f);
        }
        a.out_color[p] = oc;
        a.out_stat[p] = os;
    }
}

}  // namespace gnxr
