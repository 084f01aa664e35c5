"""numpy restatement of lightmap baking (include/gnxr.h, "Lightmap baking"): atlas rasterisation by brute force, the surface rays, the
ordered reduction and the gutter dilation, each operation a single fp32 operation in the written order.  The device results are compared
with these on bits."""
import numpy as np

f32 = np.float32
PI = f32(3.14159265358979323846)
PI_OVER_2 = f32(1.57079632679489661923)
PI_OVER_4 = f32(0.78539816339744830961)
MACH_EPS = f32(2.0 ** -24)
GAMMA7 = (f32(7) * MACH_EPS) / (f32(1) - f32(7) * MACH_EPS)


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------- atlas rasterisation
def edge(au, av, bu, bv, cu, cv):
    return (bu - au) * (cv - av) - (bv - av) * (cu - au)


def rasterise(lm_uv, W, H):
    """(tri [H, W] int32, bary [H, W, 2] float32): every triangle against every texel centre, lowest index first"""
    lm_uv = np.asarray(lm_uv, f32).reshape(-1, 6)
    cu = ((np.arange(W, dtype=f32) + f32(0.5)) / f32(W))[None, :]
    cv = ((np.arange(H, dtype=f32) + f32(0.5)) / f32(H))[:, None]
    tri = np.full((H, W), -1, np.int32)
    bary = np.zeros((H, W, 2), f32)
    with np.errstate(all="ignore"):
        for t, (u0, v0, u1, v1, u2, v2) in enumerate(lm_uv):
            area = edge(u0, v0, u1, v1, u2, v2)
            if not (np.isfinite([u0, v0, u1, v1, u2, v2]).all() and np.isfinite(area) and area != 0):
                continue
            wa, wb, wc = edge(u1, v1, u2, v2, cu, cv), edge(u2, v2, u0, v0, cu, cv), edge(u0, v0, u1, v1, cu, cv)
            box = (cu >= min(u0, u1, u2)) & (cu <= max(u0, u1, u2)) & (cv >= min(v0, v1, v2)) & (cv <= max(v0, v1, v2))
            inside = (wa >= 0) & (wb >= 0) & (wc >= 0) if area > 0 else (wa <= 0) & (wb <= 0) & (wc <= 0)
            won = box & inside & (tri < 0)
            tri[won] = t
            bary[..., 0][won] = (wb / area)[won]
            bary[..., 1][won] = (wc / area)[won]
    return tri, bary


def grid_atlas(n_triangles, cells):
    """Chart c = triangles (2c, 2c + 1): the square cell c of a cells x cells grid over [0, 1]^2, split along its diagonal, so that
    neighbouring charts share edges.  Triangles beyond the grid get a zero-area uv (they bake nothing)."""
    uv = np.zeros((n_triangles, 6), f32)
    for t in range(min(n_triangles, 2 * cells * cells)):
        c = t // 2
        x0, y0 = f32(c % cells) / f32(cells), f32(c // cells) / f32(cells)
        x1, y1 = f32(c % cells + 1) / f32(cells), f32(c // cells + 1) / f32(cells)
        uv[t] = (x0, y0, x1, y0, x1, y1) if t % 2 == 0 else (x0, y0, x1, y1, x0, y1)
    return uv


# ---------------------------------------------------------------- dilation
def dilate(img, iterations):
    img = np.array(img, f32)
    H, W = img.shape[:2]
    filled = img[..., 3] > 0
    for _ in range(iterations):
        src, src_filled = img.copy(), filled.copy()
        for y in range(H):
            for x in range(W):
                if src_filled[y, x]:
                    continue
                rgb, count = np.zeros(3, f32), 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        xx, yy = x + dx, y + dy
                        if (dx == 0 and dy == 0) or xx < 0 or xx >= W or yy < 0 or yy >= H or not src_filled[yy, xx]:
                            continue
                        rgb = rgb + src[yy, xx, :3]
                        count += 1
                if count:
                    img[y, x, :3] = rgb / f32(count)
                    filled[y, x] = True
    return img


# ---------------------------------------------------------------- surface rays
def _cross(a, b):   # double products, one rounding (core/Geometry.h:925-931)
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def _length_sq(a):
    return a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]


def _div(a, s):   # Vector3 / float: a multiplication by the reciprocal (core/Geometry.h:206-210)
    return a * (f32(1) / s)[:, None]


def _next_up(v):
    v = np.where(v == 0, f32(0), v).astype(f32)
    ui = v.view(np.uint32).copy()
    ui = np.where(v >= 0, ui + np.uint32(1), ui - np.uint32(1)).astype(np.uint32)
    return np.where(np.isposinf(v), v, ui.view(f32))


def _next_down(v):
    v = np.where(v == 0, f32(-0.0), v).astype(f32)
    ui = v.view(np.uint32).copy()
    ui = np.where(v > 0, ui - np.uint32(1), ui + np.uint32(1)).astype(np.uint32)
    return np.where(np.isneginf(v), v, ui.view(f32))


def surface_rays(p0, p1, p2, bary, u, sincos, flip=False):
    """p0, p1, p2: (n, 3) world-space corners; bary: (n, 2) = b1, b2; u: (n, 2) = Halton dimensions 3 and 4; sincos(theta) -> (sin, cos)
    with the library's bits.  Returns (o [n, 3], d [n, 3], p [n, 3], normal [n, 3], valid [n])."""
    p0, p1, p2, bary, u = (np.asarray(a, f32) for a in (p0, p1, p2, bary, u))
    with np.errstate(all="ignore"):
        b1, b2 = bary[:, 0], bary[:, 1]
        b0 = f32(1) - b1 - b2
        dp02, dp12 = p0 - p2, p1 - p2
        # surface_point with the default uvs: dpdu = ((-1) * dp02 - (-1) * dp12) * 1, dpdv = ((-0) * dp02 + (-1) * dp12) * 1
        dpdu, dpdv = (f32(-1) * dp02 - f32(-1) * dp12) * f32(1), (f32(-0.0) * dp02 + f32(-1) * dp12) * f32(1)
        valid = ~((_length_sq(_cross(dpdu, dpdv)) == 0) & (_length_sq(_cross(p2 - p0, p1 - p0)) == 0))
        ab = [np.abs(b0[:, None] * p0), np.abs(b1[:, None] * p1), np.abs(b2[:, None] * p2)]
        p_error = GAMMA7 * (ab[0] + ab[1] + ab[2])
        p = b0[:, None] * p0 + b1[:, None] * p1 + b2[:, None] * p2
        ng = _cross(dp02, dp12)
        n = _div(ng, np.sqrt(_length_sq(ng)))
        if flip:
            n = -n
        # CosineSampleHemisphere over ConcentricSampleDisk
        ox, oy = f32(2) * u[:, 0] - f32(1), f32(2) * u[:, 1] - f32(1)
        x_big = np.abs(ox) > np.abs(oy)
        q = np.where(x_big, oy, ox) / np.where(x_big, ox, oy)
        r = np.where(x_big, ox, oy)
        theta = np.where(x_big, PI_OVER_4 * q, PI_OVER_2 - PI_OVER_4 * q).astype(f32)
        centre = (ox == 0) & (oy == 0)
        st, ct = sincos(np.where(centre, f32(0), theta).astype(f32))
        dx, dy = np.where(centre, f32(0), r * ct).astype(f32), np.where(centre, f32(0), r * st).astype(f32)
        wz = np.sqrt(np.maximum(f32(0), f32(1) - dx * dx - dy * dy))
        # CoordinateSystem(n)
        n_big = np.abs(n[:, 0]) > np.abs(n[:, 1])
        a = np.where(n_big, n[:, 0], n[:, 1])
        zero = np.zeros_like(a)
        num = np.where(n_big[:, None], np.stack([-n[:, 2], zero, n[:, 0]], axis=1), np.stack([zero, n[:, 2], -n[:, 1]], axis=1))
        ss = _div(num, np.sqrt(a * a + n[:, 2] * n[:, 2]))
        ts = _cross(n, ss)
        d = (ss * dx[:, None] + ts * dy[:, None]) + n * wz[:, None]
        # OffsetRayOrigin(p, pError, n, d)
        na = np.abs(n)
        dd = na[:, 0] * p_error[:, 0] + na[:, 1] * p_error[:, 1] + na[:, 2] * p_error[:, 2]
        offset = dd[:, None] * n
        w_dot_n = d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2]
        offset = np.where((w_dot_n < 0)[:, None], -offset, offset)
        po = p + offset
        o = np.where(offset > 0, _next_up(po), np.where(offset < 0, _next_down(po), po)).astype(f32)
    for arr in (o, d, p, n):
        arr[~valid] = 0
    return o, d.astype(f32), p.astype(f32), n.astype(f32), valid


# ---------------------------------------------------------------- the reduction
def reduce_lightmap(tri, L, spp):
    """tri: (H, W) winners; L: (spp, n_covered, 3+) Li per sample and covered texel (texel order).  rgb = ((0 + L_0 + L_1 ...) / spp) * pi."""
    H, W = tri.shape
    img = np.zeros((H, W, 4), f32)
    acc = np.zeros((L.shape[1], 3), f32)
    for s in range(spp):
        acc = acc + np.asarray(L[s, :, :3], f32)
    covered = tri >= 0
    img[covered, :3] = (acc / f32(spp)) * PI
    img[covered, 3] = 1
    return img
