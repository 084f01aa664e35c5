"""gnxr_denoise_device restated in numpy float32 (the definition: include/gnxr.h): sequential and simple.

Every line is one float32 operation on whole images; the 25 taps are shifted slices, taken in the definition's order, and the views are
looped, so no tap can cross from one view into the next.  `expf` is a parameter -- np.exp on float32 is NOT glibc's expf -- that maps
a float32 array to a float32 array of the same shape: GPU tests pass lambda x: gx.eval_libm("exp", x), CPU tests glibc_expf below.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
K = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
LUM = (F(0.212671), F(0.715160), F(0.072169))


def glibc_expf(x):
    """expf of the C library this process runs on, element by element"""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = libm.expf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    x = np.asarray(x, dtype=np.float32)
    return np.array([f(float(v)) for v in x.ravel()], dtype=np.float32).reshape(x.shape)


def lum(x):
    return (LUM[0] * x[..., 0] + LUM[1] * x[..., 1]) + LUM[2] * x[..., 2]


def _shift(H, W, oy, ox):
    """(slices of the pixels p whose tap q = p + (ox, oy) lies in the image, slices of those q), or None"""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _denoise_view(a, b, albedo, normal, depth, iterations, sigma_color, sigma_normal, sigma_depth, expf):
    H, W = a.shape[:2]
    sc, sn, sd = F(sigma_color), F(sigma_normal), F(sigma_depth)
    if albedo is not None:
        t = albedo[..., :3] + (F(1) - albedo[..., 3])[..., None]
        div = np.where(t > F(1.0 / 1024.0), t, F(1.0 / 1024.0)).astype(F)
    else:
        div = np.ones((H, W, 3), F)
    if b is not None:
        c = (a[..., :3] + b[..., :3]) / div
        d = lum(a[..., :3] / div) - lum(b[..., :3] / div)
        v = d * d
    else:
        c = a[..., :3] / div
        v = np.zeros((H, W), F)
    valid = np.isfinite(c).all(axis=-1) & np.isfinite(v)
    c = np.where(valid[..., None], c, F(0)).astype(F)
    v = np.where(valid, v, F(-1)).astype(F)
    use_c = sc > 0
    use_n = normal is not None and sn > 0
    use_z = depth is not None and sd > 0
    n = normal[..., :3] if use_n else None
    inv_sn = F(1) / (sn * sn) if use_n else None
    inv_sc = F(1) / (sc * sc) if use_c else None
    for i in range(iterations):
        s = 1 << i
        if use_c and b is not None:
            sgv, sg = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    sh = _shift(H, W, dy, dx)
                    if sh is None:
                        continue
                    p, q = sh
                    g = F(1.0 / 4.0) if (dx, dy) == (0, 0) else F(1.0 / 8.0) if dx == 0 or dy == 0 else F(1.0 / 16.0)
                    sgv[p] = np.where(valid[q], sgv[p] + g * v[q], sgv[p])
                    sg[p] = np.where(valid[q], sg[p] + g, sg[p])
            vbar = np.where(sg > 0, sgv / sg, F(0)).astype(F)
            inv_c = F(1) / (sc * np.sqrt(vbar) + F(1e-6))
            lum_c = lum(c)
        if use_z:
            inv_z = F(1) / ((sd * F(s)) * depth + F(1e-20))
        sum_c, sum_w, sum_v = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                sh = _shift(H, W, s * dy, s * dx)
                if sh is None:
                    continue
                p, q = sh
                h = K[abs(dy)] * K[abs(dx)]
                x_c = np.zeros(valid[p].shape, F)
                x_n, x_z = x_c, x_c
                if use_c:
                    if b is not None:
                        x_c = np.abs(lum_c[p] - lum_c[q]) * inv_c[p]
                    else:
                        dc = c[p] - c[q]
                        x_c = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * (inv_sc * F(4 ** i))
                    x_c = np.where(valid[p], x_c, F(0)).astype(F)
                if use_n:
                    dn = n[p] - n[q]
                    x_n = ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * inv_sn
                if use_z:
                    x_z = np.abs(depth[p] - depth[q]) * inv_z[p]
                arg = np.ascontiguousarray(-((x_c + x_n) + x_z), dtype=F)
                w = h * np.asarray(expf(arg), dtype=F).reshape(arg.shape)
                take = valid[q] & (w > 0)
                sum_c[p] = np.where(take[..., None], sum_c[p] + w[..., None] * c[q], sum_c[p])
                sum_w[p] = np.where(take, sum_w[p] + w, sum_w[p])
                sum_v[p] = np.where(take, sum_v[p] + (w * w) * v[q], sum_v[p])
        ok = sum_w > 0
        c = np.where(ok[..., None], sum_c / sum_w[..., None], c).astype(F)
        v = np.where(ok, sum_v / (sum_w * sum_w), v).astype(F)
        valid = valid | ok
    out = np.empty((H, W, 4), F)
    raw = a[..., :3] + b[..., :3] if b is not None else a[..., :3]
    out[..., :3] = np.where(valid[..., None], c * div, raw)
    out[..., 3] = a[..., 3]
    return out


def denoise_reference(color, color_b=None, albedo=None, normal=None, depth=None, iterations=5, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.01, expf=glibc_expf):
    """gx.denoise on numpy arrays: (H, W, 4) or (V, H, W, 4) float32, depth (H, W) or (V, H, W)"""
    arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (color, color_b, albedo, normal, depth)]
    single = arrs[0].ndim == 3
    if single:
        arrs = [None if x is None else x[None] for x in arrs]
    with np.errstate(all="ignore"):
        out = np.stack([_denoise_view(*[None if x is None else x[v] for x in arrs], iterations, sigma_color, sigma_normal, sigma_depth, expf)
                        for v in range(arrs[0].shape[0])])
    return out[0] if single else out
