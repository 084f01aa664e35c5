"""The display stage restated in numpy float32 (the definition: include/gnxr.h, "Display stage"): gnxr_luminance_histogram_device,
gnxr_exposure_device and gnxr_tonemap_device, sequential and simple.

Every line is one float32 operation.  `exp` and `pow` are parameters -- numpy's are NOT glibc's expf and powf -- that map float32 arrays
to a float32 array of the same shape: GPU tests pass lambda x: gx.eval_libm("exp", x) and lambda a, b: gx.eval_libm("pow", a, b), CPU
tests the C library of the process (glibc_expf, glibc_powf below).
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
LUM = (F(0.212671), F(0.715160), F(0.072169))
WORDS = 260
BELOW, ABOVE, NOT_FINITE = 256, 257, 258
CURVES = ("linear", "reference", "reinhard", "aces")


def _libm(name, nargs):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = getattr(libm, name)
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * nargs
    return f


def glibc_expf(x):
    """expf of the C library this process runs on, element by element"""
    f = _libm("expf", 1)
    x = np.asarray(x, dtype=F)
    return np.array([f(float(v)) for v in x.ravel()], dtype=F).reshape(x.shape)


def glibc_powf(x, y):
    """powf of the C library this process runs on, element by element"""
    f = _libm("powf", 2)
    x, y = np.broadcast_arrays(np.asarray(x, dtype=F), np.asarray(y, dtype=F))
    return np.array([f(float(a), float(b)) for a, b in zip(x.ravel(), y.ravel())], dtype=F).reshape(x.shape)


def biteq(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def lum(x):
    with np.errstate(all="ignore"):
        return (LUM[0] * x[..., 0] + LUM[1] * x[..., 1]) + LUM[2] * x[..., 2]


def raw_bin(l, min_log2):
    """k = (int)(bits >> 19) - ((min_log2 + 127) << 4) of a positive finite luminance: below 0 and above 255 are out of range"""
    bits = np.asarray(l, dtype=F).view(np.uint32)
    return (bits >> 19).astype(np.int64) - ((int(min_log2) + 127) << 4)


def word(l, min_log2):
    """the word of the histogram that a pixel of luminance l counts in"""
    l = np.asarray(l, dtype=F)
    bits = l.view(np.uint32)
    k = raw_bin(l, min_log2)
    with np.errstate(invalid="ignore"):
        positive = l > 0
    ranged = np.where(k < 0, BELOW, np.where(k > 255, ABOVE, k))
    return np.where((bits & 0x7f800000) == 0x7f800000, NOT_FINITE, np.where(positive, ranged, BELOW))


def images(color):
    """(V, H, W, 4) of an (H, W, 4) or (V, H, W, 4) image"""
    color = np.ascontiguousarray(color, dtype=F)
    return color[None] if color.ndim == 3 else color


def histogram(color, min_log2=-12):
    """(V, 260) int64"""
    c = images(color)
    w = word(lum(c), min_log2)
    return np.stack([np.bincount(w[v].ravel(), minlength=WORDS) for v in range(c.shape[0])]).astype(np.int64).reshape(c.shape[0], WORDS)


def exposure(hist, prev=None, key=0.18, low=0.5, high=0.95, rate=1.0, min_exposure=2.0 ** -8, max_exposure=2.0 ** 8, min_log2=-12, pow=glibc_powf):
    """(V, 4) float32: (exposure, target, L, kept weight) per view.  prev: None or a (V, 4) float32 array"""
    hist = np.asarray(hist)
    out = np.zeros((hist.shape[0], 4), F)
    key, low, high, rate, lo_e, hi_e = F(key), F(low), F(high), F(rate), F(min_exposure), F(max_exposure)
    for v in range(hist.shape[0]):
        h = hist[v]
        total = F(int(h[:256].astype(np.int64).sum()))
        skip = total * low
        keep = total * high - skip
        sw, sx = F(0), F(0)
        for k in range(256):
            c = F(int(h[k]))
            s = min(c, skip)
            c = c - s
            skip = skip - s
            t = min(c, keep)
            keep = keep - t
            sw = sw + t
            sx = sx + t * (F(k) + F(0.5))
        pv = F(prev[v][0]) if prev is not None else F(0)
        prev_ok = bool(pv > 0) and bool(np.isfinite(pv))
        if sw > 0:
            m = sx / sw
            L = F(min_log2) + m * F(0.0625)
            p = pow(np.array([2.0], F), np.array([-L], F))[0]
            with np.errstate(over="ignore"):
                target = np.fmin(np.fmax(key * F(p), lo_e), hi_e)
        else:
            L = F(0)
            target = pv if prev_ok else F(1)
        e = pv + (target - pv) * rate if prev_ok else target
        out[v] = (e, target, L, sw)
    return out


def curve_value(x, curve, white, exp):
    """y of the definition before the clamp, for x already scaled, cleaned and limited"""
    one = F(1)
    if curve == "linear":
        return x
    if curve == "reference":
        return one - exp((-x / F(0.25)).astype(F))
    if curve == "reinhard":
        ww = F(white) * F(white)
        return (x * (one + x / ww)) / (one + x)
    if curve == "aces":
        return (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
    raise ValueError(curve)


def tonemap(color, E=1.0, curve="aces", white=4.0, srgb=True, round=True, exp=glibc_expf, pow=glibc_powf):
    """uint8 array of color's shape.  E: a number, or one float per view"""
    c = images(color)
    V = c.shape[0]
    E = np.broadcast_to(np.asarray(E, dtype=F).reshape(-1), (V,)).reshape(V, 1, 1, 1)
    with np.errstate(all="ignore"):
        x = c[..., :3] * E
        x = np.where(x > 0, x, F(0)).astype(F)
        x = np.minimum(x, F(65504))
        y = curve_value(x, curve, white, exp).astype(F)
        y = np.fmin(np.fmax(y, F(0)), F(1))
        z = y
        if srgb:
            z = F(12.92) * y
            hi = y > F(0.0031308)
            z[hi] = F(1.055) * pow(y[hi], np.full(int(hi.sum()), F(1) / F(2.4), F)) - F(0.055)
        z255 = z * F(255)
        b = (z255 + F(0.5)) if round else z255
    out = np.full(c.shape, 255, np.uint8)
    out[..., :3] = b.astype(np.int32).astype(np.uint8)
    return out.reshape(np.shape(color))
