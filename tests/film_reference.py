"""The film of include/gnxr.h ("Film: pixel reconstruction filters"), restated in numpy fp32: what gnxr_film_add_device and
gnxr_film_resolve_device compute, bit for bit.

Vectorised over the destination pixels; the loops run over the layers j and then over the offsets (qy - y, qx - x) of the source pixel
from the destination, both ascending -- so every destination receives its contributions in the order (j, qy, qx) the definition
fixes.  Every numpy operation on float32 arrays is one fp32 operation, rounded on its own.  The table is an argument: the image tests
pass the one the library returns (gnxr_film_filter_table), so they do not depend on expf; the restatements of the table itself live
in test_film.py."""
import math

import numpy as np

f32 = np.float32


def film_add_reference(table, rx, ry, L, offsets, accum):
    """table: 256 floats; rx, ry: the radii; L (n, V, H, W, 4); offsets (n, V, H, W, 2); accum (V, H, W, 4) = (Sr, Sg, Sb, Wt).
    Returns the new accumulator; the arguments are not changed."""
    table = np.ascontiguousarray(table, f32).reshape(256)
    rx, ry = f32(rx), f32(ry)
    L, offsets = np.asarray(L, f32), np.asarray(offsets, f32)
    acc = np.array(accum, dtype=f32, copy=True)
    n, V, H, W = L.shape[:4]
    assert L.shape == (n, V, H, W, 4) and offsets.shape == (n, V, H, W, 2) and acc.shape == (V, H, W, 4)
    inv_rx, inv_ry = f32(1) / rx, f32(1) / ry
    # one pixel more than |q - p| <= ceil(r + 0.5), the window gnxr.h asks a kernel to cover: a tap out there adds nothing
    hx, hy = int(math.ceil(float(rx) + 0.5)) + 1, int(math.ceil(float(ry) + 0.5)) + 1
    xs, ys = np.arange(W), np.arange(H)
    with np.errstate(all="ignore"):
        for j in range(n):
            for oy in range(-hy, hy + 1):
                y0, y1 = max(0, -oy), min(H, H - oy)   # destination rows whose source row y + oy lies inside the image
                if y0 >= y1:
                    continue
                for ox in range(-hx, hx + 1):
                    x0, x1 = max(0, -ox), min(W, W - ox)
                    if x0 >= x1:
                        continue
                    src = (slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    dst = (slice(None), slice(y0, y1), slice(x0, x1))
                    ux, uy = offsets[j][src + (0,)], offsets[j][src + (1,)]
                    valid = (ux >= 0) & (ux <= 1) & (uy >= 0) & (uy <= 1)   # (a NaN fails)
                    ux, uy = np.where(valid, ux, f32(0)), np.where(valid, uy, f32(0))
                    qx = (xs[x0:x1] + ox).astype(f32)[None, None, :]
                    qy = (ys[y0:y1] + oy).astype(f32)[None, :, None]
                    dx, dy = (qx + ux) - f32(0.5), (qy + uy) - f32(0.5)
                    wx0, wx1 = np.ceil(dx - rx).astype(np.int64), np.floor(dx + rx).astype(np.int64) + 1
                    wy0, wy1 = np.ceil(dy - ry).astype(np.int64), np.floor(dy + ry).astype(np.int64) + 1
                    x, y = xs[x0:x1][None, None, :], ys[y0:y1][None, :, None]
                    hit = valid & (wx0 <= x) & (x < wx1) & (wy0 <= y) & (y < wy1)
                    fx = np.abs(((x.astype(f32) - dx) * inv_rx) * f32(16))
                    fy = np.abs(((y.astype(f32) - dy) * inv_ry) * f32(16))
                    ifx = np.minimum(np.floor(fx).astype(np.int64), 15)
                    ify = np.minimum(np.floor(fy).astype(np.int64), 15)
                    w = table[np.where(hit, ify * 16 + ifx, 0)]
                    Lq = L[j][src]
                    a = acc[dst]
                    new = a.copy()
                    for c in range(3):
                        new[..., c] = a[..., c] + Lq[..., c] * w
                    new[..., 3] = a[..., 3] + w
                    acc[dst] = np.where(hit[..., None], new, a)
    return acc


def film_resolve_reference(accum):
    """(c(Sr), c(Sg), c(Sb), 1): c(S) = 0 where Wt == 0, else S / Wt -- 0 where that is negative; a NaN stays"""
    acc = np.asarray(accum, f32)
    out = np.ones_like(acc)
    wt = acc[..., 3]
    with np.errstate(all="ignore"):
        for c in range(3):
            t = acc[..., c] / wt
            out[..., c] = np.where(wt == 0, f32(0), np.where(t < 0, f32(0), t))
    return out
