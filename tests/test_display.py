"""The display stage (include/gnxr.h, "Display stage"): the ABI and the refusals that need no device, the numpy restatement
(tests/display_reference.py) against closed forms -- then on the GPU the three calls against the restatement on seeded inputs that reach
every branch, the REFERENCE curve against gnxr_framebuffer_update, Display.present against the chain of public calls, stream order
and the refusals that need a device.  Every comparison is on bits or bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import display_reference as dr
import scenes
from conftest import ROOT

ERR_INVALID, ERR_NO_DEVICE = -1, -2
f32 = np.float32
NAMES = ("gnxr_luminance_histogram_device", "gnxr_exposure_device", "gnxr_tonemap_device")
DEV = "cuda:0"
BIG = (1, 613, 1031)   # 632,003 pixels: more than the 524,288 lanes of the largest grid, every grid-stride loop takes a second turn (the histogram's more)


# ---------------------------------------------------------------- CPU: the ABI
def test_display_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(gx.lib(), name) and name in gx._abi.PROTOTYPES, name
    # no record joins gnxr_abi_sizeof's list, the version stays
    assert gx.lib().gnxr_abi_version() == 5 and gx.lib().gnxr_abi_sizeof(13) > 0 and gx.lib().gnxr_abi_sizeof(14) == -1
    A = gx._abi
    assert C.sizeof(A.HistogramParams) == 20 and C.sizeof(A.ExposureParams) == 40 and C.sizeof(A.TonemapParams) == 32
    assert re.search(r"struct gnxr_histogram_params \{ int32_t struct_size, width, height, n_views, min_log2; \}", hdr)
    assert re.search(r"struct gnxr_exposure_params \{ int32_t struct_size, n_views, min_log2, pad;\s*float key, low, high, rate, min_exposure, max_exposure; \}", hdr)
    assert re.search(r"struct gnxr_tonemap_params \{ int32_t struct_size, width, height, n_views, curve; uint32_t flags;\s*float exposure, white; \}", hdr)
    assert re.search(r"#define GNXR_HISTOGRAM_WORDS 260\b", hdr) and A.HISTOGRAM_WORDS == 260 == dr.WORDS
    assert re.search(r"GNXR_TONEMAP_LINEAR = 0, GNXR_TONEMAP_REFERENCE = 1, GNXR_TONEMAP_REINHARD = 2, GNXR_TONEMAP_ACES = 3", hdr)
    assert (A.TONEMAP_LINEAR, A.TONEMAP_REFERENCE, A.TONEMAP_REINHARD, A.TONEMAP_ACES) == (0, 1, 2, 3)
    assert re.search(r"#define GNXR_TONEMAP_SRGB\s+1u", hdr) and re.search(r"#define GNXR_TONEMAP_ROUND\s+2u", hdr) and (A.TONEMAP_SRGB, A.TONEMAP_ROUND) == (1, 2)
    assert tuple(gx.TONEMAP_CURVES[k] for k in dr.CURVES) == (0, 1, 2, 3)
    for name in ("luminance_histogram", "auto_exposure", "tonemap", "Display"):
        assert callable(getattr(gx, name))
    assert callable(gx.Display.present) and callable(gx.Display.reset)


# ---------------------------------------------------------------- CPU: the refusals
def test_display_calls_refuse_malformed_arguments_before_any_device(gx):
    L, A = gx.lib(), gx._abi
    buf = (C.c_float * 8192)()
    base = (C.addressof(buf) + 15) & ~15   # host memory that passes every argument check: the device is asked last
    vp = C.c_void_p
    err = lambda: L.gnxr_last_error()

    def hist(W=8, H=8, V=1, lo=-12, size=20, rgba=base, out=base + 16384, params=True):
        p = A.HistogramParams(size, W, H, V, lo)
        return L.gnxr_luminance_histogram_device(C.byref(p) if params else None, vp(rgba) if rgba else None, vp(out) if out else None, None)

    assert hist(params=False) == ERR_INVALID and b"null" in err() and b"params" in err()
    assert hist(rgba=0) == ERR_INVALID and b"d_rgba" in err()
    assert hist(out=0) == ERR_INVALID and b"d_hist" in err()
    assert hist(size=24) == ERR_INVALID and b"struct_size" in err()
    assert hist(W=0) == ERR_INVALID and b"width" in err() and hist(H=0) == ERR_INVALID and b"height" in err() and hist(V=-1) == ERR_INVALID and b"n_views" in err()
    assert hist(lo=-127) == ERR_INVALID and b"min_log2" in err() and hist(lo=112) == ERR_INVALID and b"min_log2" in err()
    assert hist(rgba=base + 4) == ERR_INVALID and b"d_rgba is not 16-byte aligned" in err()
    assert hist(out=base + 16384 + 8) == ERR_INVALID and b"d_hist is not 16-byte aligned" in err()
    assert hist(out=base + 512) == ERR_INVALID and b"overlaps" in err()
    assert hist(W=32768, H=32768, V=2) == ERR_INVALID and b"path indexing" in err()
    assert hist(V=0) == 0

    def expo(V=1, lo=-12, key=0.18, low=0.5, high=0.95, rate=1.0, emin=2.0 ** -8, emax=2.0 ** 8, size=40, h=base, prev=0, out=base + 4096, params=True):
        p = A.ExposureParams(size, V, lo, 0, key, low, high, rate, emin, emax)
        return L.gnxr_exposure_device(C.byref(p) if params else None, vp(h) if h else None, vp(prev) if prev else None, vp(out) if out else None, None)

    nan, inf = float("nan"), float("inf")
    assert expo(params=False) == ERR_INVALID and b"null" in err()
    assert expo(h=0) == ERR_INVALID and b"d_hist" in err() and expo(out=0) == ERR_INVALID and b"d_exposure" in err()
    assert expo(size=36) == ERR_INVALID and b"struct_size" in err()
    assert expo(V=-1) == ERR_INVALID and b"n_views" in err()
    assert expo(lo=-127) == ERR_INVALID and expo(lo=112) == ERR_INVALID and b"min_log2" in err()
    assert expo(low=0.5, high=0.5) == ERR_INVALID and b"low" in err() and expo(low=0.9, high=0.2) == ERR_INVALID and b"low" in err()
    assert expo(low=-0.1) == ERR_INVALID and b"low" in err() and expo(high=1.5) == ERR_INVALID and b"high" in err()
    assert expo(rate=0.0) == ERR_INVALID and b"rate" in err() and expo(rate=nan) == ERR_INVALID and b"rate" in err() and expo(rate=1.5) == ERR_INVALID and b"rate" in err()
    assert expo(key=0.0) == ERR_INVALID and b"key" in err() and expo(key=inf) == ERR_INVALID and b"key" in err()
    assert expo(emin=0.0) == ERR_INVALID and b"min_exposure" in err() and expo(emin=2.0, emax=1.0) == ERR_INVALID and b"min_exposure" in err()
    assert expo(emax=inf) == ERR_INVALID and b"finite" in err() and expo(low=nan) == ERR_INVALID and expo(high=nan) == ERR_INVALID
    assert expo(h=base + 4) == ERR_INVALID and b"d_hist is not 16-byte aligned" in err()
    assert expo(out=base + 4096 + 8) == ERR_INVALID and b"d_exposure is not 16-byte aligned" in err()
    assert expo(prev=base + 8192 + 4) == ERR_INVALID and b"d_prev_exposure is not 16-byte aligned" in err()
    assert expo(out=base + 16) == ERR_INVALID and b"overlaps d_hist" in err()
    assert expo(V=2, prev=base + 4096 + 16) == ERR_INVALID and b"overlaps d_prev_exposure" in err()          # a partial overlap; the same address is in place
    assert expo(V=0) == 0 and expo(V=0, prev=base + 4096) == 0

    def tone(W=8, H=8, V=1, curve=3, flags=3, e=1.0, white=4.0, size=32, rgba=base, ex=0, out=base + 16384, params=True):
        p = A.TonemapParams(size, W, H, V, curve, flags, e, white)
        return L.gnxr_tonemap_device(C.byref(p) if params else None, vp(rgba) if rgba else None, vp(ex) if ex else None, vp(out) if out else None, None)

    assert tone(params=False) == ERR_INVALID and b"null" in err()
    assert tone(rgba=0) == ERR_INVALID and b"d_rgba" in err() and tone(out=0) == ERR_INVALID and b"d_rgba8_out" in err()
    assert tone(size=28) == ERR_INVALID and b"struct_size" in err()
    assert tone(W=0) == ERR_INVALID and tone(H=0) == ERR_INVALID and tone(V=-1) == ERR_INVALID and b"n_views" in err()
    assert tone(curve=4) == ERR_INVALID and b"curve" in err() and tone(curve=-1) == ERR_INVALID and b"curve" in err()
    assert tone(flags=4) == ERR_INVALID and b"flags" in err() and tone(flags=0x80000001) == ERR_INVALID and b"flags" in err()
    assert tone(e=-1.0) == ERR_INVALID and b"exposure" in err() and tone(e=nan) == ERR_INVALID and tone(e=inf) == ERR_INVALID and b"exposure" in err()
    for curve in range(4):   # read for REINHARD only, validated always
        assert tone(curve=curve, white=0.0) == ERR_INVALID and b"white" in err()
    assert tone(white=1e-4) == ERR_INVALID and tone(white=70000.0) == ERR_INVALID and tone(white=nan) == ERR_INVALID and b"white" in err()
    assert tone(rgba=base + 8) == ERR_INVALID and b"d_rgba is not 16-byte aligned" in err()
    assert tone(ex=base + 8192 + 4) == ERR_INVALID and b"d_exposure is not 16-byte aligned" in err()
    assert tone(out=base + 16384 + 2) == ERR_INVALID and b"d_rgba8_out is not 4-byte aligned" in err()
    assert tone(out=base + 16384 + 4) != ERR_INVALID or b"aligned" not in err()                              # 4 bytes are enough for the bytes
    assert tone(out=base + 1020) == ERR_INVALID and b"overlaps d_rgba" in err()
    assert tone(ex=base + 16384 + 240) == ERR_INVALID and b"overlaps d_exposure" in err()
    assert tone(W=32768, H=32768, V=2) == ERR_INVALID and b"path indexing" in err()
    assert tone(V=0) == 0
    # arguments that pass every check need the runtime: no CPU fallback
    if not torch.cuda.is_available():
        assert hist() == ERR_NO_DEVICE and expo() == ERR_NO_DEVICE and expo(prev=base + 4096) == ERR_NO_DEVICE and tone() == ERR_NO_DEVICE
    del buf


def test_python_argument_errors_need_no_device(gx):
    cpu = torch.zeros((4, 4, 4))
    for call in (lambda: gx.luminance_histogram(cpu), lambda: gx.luminance_histogram(np.zeros((4, 4, 4), f32)), lambda: gx.tonemap(cpu), lambda: gx.tonemap("image"),
                 lambda: gx.auto_exposure(torch.zeros((1, 260), dtype=torch.int32)), lambda: gx.auto_exposure(None),
                 lambda: gx.Display(0, 4), lambda: gx.Display(4, 0), lambda: gx.Display(4, 4, 0), lambda: gx.Display(4, 4, gamma=2.2), lambda: gx.Display(4, 4, min_log2=200),
                 lambda: gx.Display(4, 4).present(cpu)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------- CPU: the restatement against closed forms
def grey(l, shape=(1, 1, 1)):
    """pixels (0, 0, b) whose luminance is fl(0.072169f * b): b = l -> a known single product"""
    c = np.zeros(shape + (4,), f32)
    c[..., 2] = l
    return c


def test_restated_bins_from_the_definition_text():
    below = lambda x: np.nextafter(f32(x), f32(0))
    k = lambda x: int(dr.raw_bin(f32(x), -12))
    assert k(2.0 ** -12) == 0 and k(below(2.0 ** -12)) == -1 and k(1.0) == 192 and k(0.18) == 151 and k(below(16.0)) == 255 and k(16.0) == 256
    # sixteen bins per octave, each a sixteenth of the mantissa range
    for e in (-12, -3, 0, 3):
        for j in range(16):
            lo = f32(2.0 ** e * (1 + j / 16))
            assert k(lo) == 16 * (e + 12) + j and k(below(lo)) == 16 * (e + 12) + j - 1
    # the coordinate of a bin is a piecewise-linear log2, within -0.12 / +0.03 stop of the true one over the bin
    x = np.exp2(np.random.default_rng(1).uniform(-12, 4, 20000)).astype(f32)
    d = -12 + (dr.raw_bin(x, -12) + 0.5) / 16 - np.log2(x.astype(np.float64))
    assert -0.12 <= d.min() and d.max() <= 1 / 32, (d.min(), d.max())      # (+0.03: half a bin)
    # the words outside the bins
    w = lambda x: int(dr.word(f32(x), -12))
    assert w(below(2.0 ** -12)) == 256 and w(0.0) == 256 and w(-0.0) == 256 and w(-3.0) == 256 and w(1e-40) == 256
    assert w(16.0) == 257 and w(3e38) == 257 and w(np.nan) == 258 and w(np.inf) == 258 and w(-np.inf) == 258
    assert int(dr.word(f32(1e-40), -126)) == 256 and int(dr.word(f32(2.0 ** -126), -126)) == 0       # subnormals are below every range
    h = dr.histogram(np.array([[[1, 1, 1, 0], [0, 0, 0, 1], [np.nan, 0, 0, 1], [100, 100, 100, 1]]], f32))
    assert h.shape == (1, 260) and h.sum() == 4 and h[0, 256] == 1 and h[0, 257] == 1 and h[0, 258] == 1 and h[0, 259] == 0 and h[0, :256].sum() == 1


def test_restated_exposure_of_a_constant_image_and_its_limits():
    c = np.full((1, 32, 32, 4), 0.18, f32)
    h = dr.histogram(c)
    l = dr.lum(c)[0, 0, 0]
    assert h[0, int(dr.raw_bin(l, -12))] == 1024 and int(dr.raw_bin(l, -12)) == 151
    e = dr.exposure(h, key=0.18, low=0.5, high=0.95)
    assert e[0, 2] == f32(-2.53125)                                        # m = 151.5 exactly: L = -12 + 151.5 / 16
    assert e[0, 3] == f32(1024) * f32(0.95) - f32(1024) * f32(0.5)         # the kept weight
    assert abs(float(e[0, 1]) - 1.0405) < 5e-5 and e[0, 0] == e[0, 1]      # 0.18 * 2^2.53125; no previous value: the target at once
    assert abs(float(e[0, 1]) - 0.18 * 2.0 ** 2.53125) < 1e-6
    # rate = 1 reaches the target in one step from any previous value, rate = 0.125 takes an eighth of the way
    prev = np.array([[4.0, 0, 0, 0]], f32)
    assert dr.exposure(h, prev=prev, rate=1.0)[0, 0] == e[0, 1]
    assert dr.exposure(h, prev=prev, rate=0.125)[0, 0] == f32(4) + (e[0, 1] - f32(4)) * f32(0.125)
    # the clamps
    assert dr.exposure(h, min_exposure=2.0)[0, 1] == 2 and dr.exposure(h, max_exposure=0.5)[0, 1] == 0.5
    # a previous value of 0, NaN or inf is no previous value
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert dr.biteq(dr.exposure(h, prev=np.array([[bad, 9, 9, 9]], f32), rate=0.125), e)


def test_restated_black_and_out_of_range_histograms_hold_the_previous_exposure():
    black = dr.histogram(np.zeros((1, 5, 7, 4), f32))
    assert black[0, 256] == 35 and black[0, :256].sum() == 0
    outside = np.zeros((1, 260), np.int64)
    outside[0, 256:259] = (5, 6, 7)
    for h in (black, outside, np.zeros((1, 260), np.int64)):
        assert dr.biteq(dr.exposure(h, prev=np.array([[3.5, 1, 1, 1]], f32), rate=0.125), np.array([[3.5, 3.5, 0, 0]], f32))
        assert dr.biteq(dr.exposure(h), np.array([[1, 1, 0, 0]], f32))
        assert dr.biteq(dr.exposure(h, prev=np.array([[np.nan, 1, 1, 1]], f32)), np.array([[1, 1, 0, 0]], f32))


def test_restated_quantiles_skip_and_keep_by_weight():
    """100 pixels in bin 10, 100 in bin 200: low = 0.5 skips the dark half, high = 1 keeps the bright one; low = 0, high = 0.5 the reverse;
    the whole range weighs them equally"""
    h = np.zeros((1, 260), np.int64)
    h[0, 10] = h[0, 200] = 100
    L = lambda **kw: float(dr.exposure(h, **kw)[0, 2])
    assert L(low=0.5, high=1.0) == -12 + 200.5 / 16 and L(low=0.0, high=0.5) == -12 + 10.5 / 16 and L(low=0.0, high=1.0) == -12 + 105.5 / 16
    assert float(dr.exposure(h, low=0.25, high=0.75)[0, 3]) == 100.0


def test_restated_tonemap_branch_point_rounding_and_cleaning():
    px = lambda *v: np.array([[list(v) + [0.0]]], f32)
    edge = f32(0.0031308)
    up = np.nextafter(edge, f32(1))
    # the sRGB branch point: y <= 0.0031308f is linear, the float above takes the power
    lin = dr.tonemap(px(edge, up, 0), curve="linear", srgb=True, round=False)
    z_lo = f32(12.92) * edge
    z_hi = f32(1.055) * dr.glibc_powf(up, f32(1) / f32(2.4)) - f32(0.055)
    assert tuple(lin[0, 0]) == (int(z_lo * f32(255)), int(z_hi * f32(255)), 0, 255)
    assert abs(float(z_lo) - float(z_hi)) < 1e-6                         # the two pieces meet there
    # truncate against round on a value whose z * 255 lies within 1e-3 below an integer
    v = np.nextafter(f32(100 / 255), f32(0))
    assert 0 < 100 - float(v * f32(255)) < 1e-3
    assert dr.tonemap(px(v, v, v), curve="linear", srgb=False, round=False)[0, 0, 0] == 99
    assert dr.tonemap(px(v, v, v), curve="linear", srgb=False, round=True)[0, 0, 0] == 100
    # NaN, negatives and -inf are 0, +inf is 65504 -> 255 under every curve; alpha is 255 whatever the image holds
    wild = np.array([[[np.nan, -1, -np.inf, np.nan], [np.inf, 1e-40, 0, -5]]], f32)
    for curve in dr.CURVES:
        got = dr.tonemap(wild, curve=curve, white=1000.0)
        assert tuple(got[0, 0]) == (0, 0, 0, 255) and got[0, 1, 0] == 255 and tuple(got[0, 1, 1:]) == (0, 0, 255), curve
    # closed forms: reinhard maps white to 1, the reference curve is FrameBuffer's 1 - exp(-4x), E scales the input
    assert dr.tonemap(px(4, 4, 4), curve="reinhard", white=4.0, srgb=False)[0, 0, 0] == 255
    x = f32(0.3)
    assert dr.tonemap(px(x, x, x), curve="reference", srgb=False, round=False)[0, 0, 0] == int((f32(1) - dr.glibc_expf(-x / f32(0.25))) * f32(255))
    assert dr.tonemap(px(0.25, 0.25, 0.25), E=2.0, curve="linear", srgb=False)[0, 0, 0] == 128
    two = dr.tonemap(np.full((2, 1, 1, 4), 0.25, f32), E=np.array([1.0, 4.0], f32), curve="linear", srgb=False)
    assert two[0, 0, 0, 0] == 64 and two[1, 0, 0, 0] == 255


# ---------------------------------------------------------------- seeded inputs
def lum_pixel(target):
    """an rgb triple (r, g, 0) whose luminance is exactly `target`: r brings the first product within a few ulps below it, a small g adds
    the rest"""
    target = f32(target)
    r = f32(np.float64(target) / np.float64(dr.LUM[0]))
    for _ in range(8):
        rest = target - dr.LUM[0] * r          # exact: the two are within a few ulps of each other
        rgb = np.array([r, f32(np.float64(rest) / np.float64(dr.LUM[1])), 0], f32)
        if rest >= 0 and dr.lum(rgb) == target:
            return [float(x) for x in rgb]
        r = np.nextafter(r, f32(0))
    raise AssertionError(f"no pixel of this form has the luminance {target!r}")


def edge_pixels(min_log2=-12):
    """for a few bin edges: pixels whose luminance is the edge, the float below it and the float above it"""
    out = []
    for k in (0, 1, 17, 151, 152, 192, 255, 256):
        edge = np.array([(k + ((min_log2 + 127) << 4)) << 19], np.uint32).view(f32)[0]
        out += [lum_pixel(edge), lum_pixel(np.nextafter(edge, f32(0))), lum_pixel(np.nextafter(edge, f32(np.inf)))]
    return out


def hist_inputs(V, H, W):
    """log-uniform luminances over 2^-14 .. 2^6, with exact bin edges and the floats either side of them, 0, -0, negatives, a subnormal,
    NaN and +-inf placed among them (as many as the image has room for)"""
    rng = np.random.default_rng([20261021, V, H, W])
    n = V * H * W
    c = (np.exp2(rng.uniform(-14, 6, (n, 1))) * rng.uniform(0.6, 1.4, (n, 4))).astype(f32)
    nan, inf = np.nan, np.inf
    special = edge_pixels() + [[0, 0, 0], [-0.0, -0.0, -0.0], [-1, -2, -3], [-1, 0.1, 0], [1e-40, 1e-40, 1e-40], [nan, 1, 1], [1, inf, 1], [1, 1, -inf], [inf, -inf, 0]]
    at = rng.permutation(n)[:len(special)]
    c[at, :3] = np.array(special, f32)[:len(at)]
    return c.reshape(V, H, W, 4)


HIST_SHAPES = [(2, 23, 37), (1, 1, 1), (3, 7, 300), BIG]


def constant_image():
    c = np.empty((2, 23, 37, 4), f32)
    c[0], c[1] = 0.18, 3.0
    return c


_hist_cache = {}


def hist_case(name):
    """(image, its histogram by the restatement), computed once"""
    if name not in _hist_cache:
        c = constant_image() if name == "constant" else hist_inputs(*name)
        _hist_cache[name] = (c, dr.histogram(c))
    return _hist_cache[name]


def test_histogram_inputs_reach_every_word_by_the_restatement_alone():
    c, h = hist_case((2, 23, 37))
    assert (h.sum(1) == 23 * 37).all() and (h[:, 256:259].sum(0) > 0).all() and (h[:, 259] == 0).all() and h[:, 0].sum() > 0 and h[:, 255].sum() > 0
    l = dr.lum(c).ravel()
    for k in (0, 1, 17, 151, 152, 192, 255, 256):
        edge = np.array([(k + (115 << 4)) << 19], np.uint32).view(f32)[0]
        for t in (edge, np.nextafter(edge, f32(0)), np.nextafter(edge, f32(np.inf))):
            assert (l == t).any(), (k, t)
    bits = l.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any() and (l < 0).any() and ((l > 0) & (l < 1.2e-38)).any()
    assert np.isnan(l).any() and np.isposinf(l).any() and np.isneginf(l).any()
    c3, _ = hist_case((3, 7, 300))
    assert (7 * 300) % 256 != 0     # 2100 pixels a view: a block of 256 pixels straddles a view's end


def first_float(pred):
    """the smallest positive float x with pred(x) -- pred is false below a threshold and true above it, up to the last bits -- and the
    float below it: a bisection over bit patterns, which order the positive floats"""
    lo, hi = 0, int(np.array([65504], f32).view(np.uint32)[0])
    assert not pred(np.array([lo], np.uint32).view(f32)[0]) and pred(np.array([hi], np.uint32).view(f32)[0])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(np.array([mid], np.uint32).view(f32)[0]) else (mid, hi)
    return np.array([lo, hi], np.uint32).view(f32)


_placed = {}
STEPS = (1, 2, 37, 128, 200, 254)   # (255 is out of reach with sRGB and truncation: 1.055f - 0.055f is below 1)


def placed_values(curve, white):
    """pairs of neighbouring floats between which a result changes, found with the restatement itself: y on the two sides of 0.0031308,
    and for every combination of flags a few bytes that step by one"""
    if (curve, white) not in _placed:
        px = lambda x: np.array([[[x, 0, 0, 0]]], f32)
        out = [first_float(lambda x: dr.curve_value(np.array([x], f32), curve, white, dr.glibc_expf)[0] > f32(0.0031308))]
        for srgb in (False, True):
            for rnd in (False, True):
                out += [first_float(lambda x: dr.tonemap(px(x), curve=curve, white=white, srgb=srgb, round=rnd)[0, 0, 0] >= n) for n in STEPS]
        _placed[(curve, white)] = np.concatenate(out)
    return _placed[(curve, white)]


def tone_inputs(V, H, W, curve, white=4.0):
    rng = np.random.default_rng([20261021, V, H, W, dr.CURVES.index(curve)])
    c = np.exp2(rng.uniform(-12, 10, (V * H * W, 4))).astype(f32)
    special = np.concatenate([np.array([0, -0.0, -1, np.nan, np.inf, -np.inf, 1e-40, 65504, 1e30], f32), placed_values(curve, white)])
    flat = c.reshape(-1)
    at = rng.permutation(flat.size)[:len(special)]
    flat[at] = special[:len(at)]
    return flat.reshape(V, H, W, 4)


def test_tonemap_inputs_straddle_the_branch_point_and_byte_steps_by_the_restatement_alone():
    for curve in dr.CURVES:
        v = placed_values(curve, 4.0)
        assert len(v) == 2 * (1 + 4 * len(STEPS)) and (v[1::2] == np.nextafter(v[0::2], f32(np.inf))).all()
        y = np.fmin(np.fmax(dr.curve_value(v[:2], curve, 4.0, dr.glibc_expf), f32(0)), f32(1))
        assert y[0] <= f32(0.0031308) < y[1], curve
        img = np.zeros((1, 1, len(v), 4), f32)
        img[0, 0, :, 0] = v
        pairs = iter(range(2, len(v), 2 * len(STEPS)))
        for srgb in (False, True):
            for rnd in (False, True):
                b = dr.tonemap(img, curve=curve, srgb=srgb, round=rnd)[0, 0, :, 0].astype(int)
                k = next(pairs)
                assert (b[k:k + 2 * len(STEPS):2] == np.array(STEPS) - 1).all() and (b[k + 1:k + 2 * len(STEPS):2] == STEPS).all(), (curve, srgb, rnd)
        # and they are in the seeded image
        c = tone_inputs(2, 23, 37, curve)
        assert np.isin(v, c).all() and np.isnan(c).any() and np.isinf(c).any() and (c < 0).any() and (c == 0).any()


# ---------------------------------------------------------------- GPU helpers
def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def device_pow(gx):
    return lambda a, b: gx.eval_libm("pow", a, b)


def device_exp(gx):
    return lambda x: gx.eval_libm("exp", x)


# ---------------------------------------------------------------- GPU 1: the histogram
@pytest.mark.gpu
@pytest.mark.parametrize("name", HIST_SHAPES + ["constant"], ids=str)
def test_histogram_equals_the_restatement_in_all_260_counters(gpu, name):
    c, want = hist_case(name)
    V, H, W = c.shape[:3]
    got = gpu.luminance_histogram(dev(c))
    assert tuple(got.shape) == (V, 260) and got.dtype == torch.int32
    g = host(got).astype(np.int64)
    print(f"histogram {name}: {int((g != want).sum())} of {g.size} counters differ; out of range per view {g[:, 256:259].tolist()}")
    assert (g == want).all(), np.argwhere(g != want)[:8]
    assert (g.sum(1) == H * W).all() and (g[:, 259] == 0).all()
    if V == 1:   # a 3-dimensional tensor is one view; a preallocated output is overwritten, not added to
        out = torch.full((1, 260), 77, dtype=torch.int32, device=DEV)
        assert gpu.luminance_histogram(dev(c[0]), out=out) is out and (host(out) == want).all()
    # another range: the same pixels, binned from 2^-3
    assert (host(gpu.luminance_histogram(dev(c), min_log2=-3)) == dr.histogram(c, -3)).all()


# ---------------------------------------------------------------- GPU 2: the exposure
def exposure_histograms():
    """the histograms of the images above, an all-zero one and one with everything out of range: (N, 260)"""
    hs = [hist_case(name)[1] for name in HIST_SHAPES + ["constant"]]
    outside = np.zeros((1, 260), np.int64)
    outside[0, 256:259] = (11, 12, 13)
    return np.concatenate(hs + [np.zeros((1, 260), np.int64), outside]).astype(np.int32)


@pytest.mark.gpu
def test_exposure_equals_the_restatement_on_bits(gpu):
    h = exposure_histograms()
    N = h.shape[0]
    assert N == 11
    rng = np.random.default_rng(20261021)
    prev = np.exp2(rng.uniform(-4, 4, (N, 4))).astype(f32)
    prev[2, 0], prev[3, 0], prev[4, 0], prev[5, 0] = 0.0, np.nan, np.inf, -2.0       # each counts as no previous value
    dh = dev(h)
    pw = device_pow(gpu)
    n = 0
    for kw in (dict(), dict(rate=0.125), dict(min_exposure=4.0), dict(max_exposure=0.25, rate=0.125), dict(key=0.5, low=0.1, high=0.6), dict(low=0.0, high=1.0, rate=0.5)):
        for mode in ("none", "prev", "in place"):
            want = dr.exposure(h, prev=None if mode == "none" else prev, pow=pw, **kw)
            if mode == "none":
                got = gpu.auto_exposure(dh, **kw)
            elif mode == "prev":
                got = gpu.auto_exposure(dh, prev=dev(prev), **kw)
            else:
                rec = dev(prev)
                got = gpu.auto_exposure(dh, prev=rec, out=rec, **kw)
                assert got is rec
            g = host(got)
            assert tuple(got.shape) == (N, 4) and dr.biteq(g, want), (kw, mode, g, want)
            n += 1
            # what the case is there for
            black = want[:, 3] == 0
            assert black[-2:].all() and not black[:-2].any()
            if "min_exposure" in kw:
                assert (want[~black, 1] == 4).any() and (want[~black, 1] >= 4).all()
            if "max_exposure" in kw:
                assert (want[~black, 1] == 0.25).any() and (want[~black, 1] <= 0.25).all()
            if mode != "none":
                assert (want[-2:, 0] == prev[-2:, 0]).all()                              # held
                assert (want[2:6, 0] == want[2:6, 1]).all()                              # no valid previous value: the target at once
                if kw.get("rate", 1.0) != 1.0:
                    assert (want[6:9, 0] != want[6:9, 1]).all()                          # on the way
            else:
                assert (want[-2:, 0] == 1).all()
    print(f"exposure: {n} calls over {N} histograms equal the restatement on bits")
    # and against the C library's powf where this machine has one that agrees with the device (glibc): the default of the restatement
    assert dr.biteq(dr.exposure(h, prev=prev), dr.exposure(h, prev=prev, pow=pw))


# ---------------------------------------------------------------- GPU 3: the tone map
def check_tonemap(gpu, c, curve, srgb, rnd, white=4.0):
    V = c.shape[0]
    dc = dev(c)
    ex, pw = device_exp(gpu), device_pow(gpu)
    worst = 0
    for E in (0.7, np.exp2(np.linspace(-1.5, 2.0, V)).astype(f32)):
        if np.ndim(E) == 0:
            got = gpu.tonemap(dc, exposure=E, curve=curve, white=white, srgb=srgb, round=rnd)
        else:
            rec = np.full((V, 4), 9.0, f32)        # only the first float of a record is read
            rec[:, 0] = E
            got = gpu.tonemap(dc, exposure=dev(rec), curve=curve, white=white, srgb=srgb, round=rnd)
        want = dr.tonemap(c, E=E, curve=curve, white=white, srgb=srgb, round=rnd, exp=ex, pow=pw)
        assert got.dtype == torch.uint8 and tuple(got.shape) == c.shape
        g = host(got)
        bad = g != want
        worst = max(worst, int(bad.sum()))
        assert not bad.any(), (curve, srgb, rnd, np.argwhere(bad)[:8], g[bad][:8], want[bad][:8])
        assert (g[..., 3] == 255).all()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("rnd", [False, True], ids=["truncate", "round"])
@pytest.mark.parametrize("srgb", [False, True], ids=["plain", "srgb"])
@pytest.mark.parametrize("curve", dr.CURVES)
def test_tonemap_equals_the_restatement_in_bytes(gpu, curve, srgb, rnd):
    c = tone_inputs(2, 23, 37, curve)
    check_tonemap(gpu, c, curve, srgb, rnd)
    if curve == "reinhard":
        check_tonemap(gpu, c, curve, srgb, rnd, white=1.5)


@pytest.mark.gpu
def test_tonemap_beyond_one_grid_of_lanes(gpu):
    check_tonemap(gpu, tone_inputs(*BIG, "aces"), "aces", True, True)


@pytest.mark.gpu
def test_reference_curve_equals_framebuffer_update(gpu):
    """code that is not under test: gnxr_framebuffer_update's kernel on a zero running mean and frame_count = 1"""
    rng = np.random.default_rng(7)
    frame = (np.exp2(rng.uniform(-10, 3, (23, 37, 4)))).astype(f32)
    frame[rng.random((23, 37)) < 0.1] = 0
    frame[..., 3] = rng.normal(size=(23, 37))          # any alpha: both write 255
    want = gpu.framebuffer_update(np.zeros((23, 37, 4), f32), frame, 1)
    got = host(gpu.tonemap(dev(frame), exposure=1, curve="reference", srgb=False, round=False))
    assert got.shape == want.shape and (got == want).all() and len(np.unique(want[..., :3])) > 100


# ---------------------------------------------------------------- GPU 4: Display
@pytest.mark.gpu
def test_display_present_equals_the_chain_of_public_calls(gpu):
    W, H = 48, 32
    scene = gpu.Scene(scenes.cornell())
    img = torch.zeros((H, W, 4), dtype=torch.float32, device=DEV)
    gpu.PathIntegrator(5, 1.0, "spatial").RenderDevice(scene, img.data_ptr(), W, H, 4, stream=torch.cuda.current_stream().cuda_stream)
    bright = img.clone()
    bright[..., :3] *= 8
    frames = [img, bright, img]
    kw = dict(rate=0.25, key=0.2, curve="reinhard", white=3.0)
    display = gpu.Display(W, H, **kw)

    def chain():
        rec, out = None, []
        for c in frames:
            hist = gpu.luminance_histogram(c)
            rec = gpu.auto_exposure(hist, prev=rec, rate=0.25, key=0.2)
            out.append((gpu.tonemap(c, exposure=rec, curve="reinhard", white=3.0), rec, hist))
        return out

    want = chain()
    for attempt in range(2):
        for k, c in enumerate(frames):
            got = display.present(c)
            assert sorted(got) == ["exposure", "hist", "rgba8"]
            assert got["rgba8"].dtype == torch.uint8 and tuple(got["rgba8"].shape) == (H, W, 4)
            assert torch.equal(got["hist"], want[k][2]) and torch.equal(got["exposure"].view(torch.int32), want[k][1].view(torch.int32)), (attempt, k)
            assert torch.equal(got["rgba8"], want[k][0]), (attempt, k)
        display.reset()      # after a reset the first frame's result recurs
    e = [host(w[1])[0] for w in want]
    print(f"display: exposure {e[0][0]:.4f} -> {e[1][0]:.4f} -> {e[2][0]:.4f}, targets {e[0][1]:.4f}, {e[1][1]:.4f}, {e[2][1]:.4f}")
    assert e[0][0] == e[0][1] and e[1][1] < e[0][1] / 4 and e[1][1] < e[1][0] < e[0][0] and e[1][0] < e[2][0] < e[2][1]
    assert len(torch.unique(want[0][0][..., :3])) > 20
    with pytest.raises(ValueError):
        display.present(torch.zeros((H, W + 1, 4), device=DEV))
    scene.close()


# ---------------------------------------------------------------- GPU 5: streams, Python checks and refusals that need a device
@pytest.mark.gpu
def test_display_calls_are_ordered_on_a_side_stream(gpu):
    c = hist_inputs(2, 23, 37)
    src = dev(c)
    want_h = gpu.luminance_histogram(src)
    want_e = gpu.auto_exposure(want_h)
    want_b = gpu.tonemap(src, exposure=want_e)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        work = torch.zeros_like(src)
        for _ in range(20):          # the image arrives late on the side stream: a call on another stream would read zeros
            work.copy_(src * 0.5)
        work.copy_(src)
    h = gpu.luminance_histogram(work, stream=side)
    e = gpu.auto_exposure(h, stream=side)
    b = gpu.tonemap(work, exposure=e, stream=side.cuda_stream)      # a raw handle is a stream too
    present = gpu.Display(37, 23, 2).present(work, stream=side)
    side.synchronize()
    assert torch.equal(h, want_h) and torch.equal(e.view(torch.int32), want_e.view(torch.int32)) and torch.equal(b, want_b) and torch.equal(present["rgba8"], want_b)


@pytest.mark.gpu
def test_display_python_checks(gpu):
    c = dev(hist_inputs(2, 5, 6))
    h = gpu.luminance_histogram(c)
    e = gpu.auto_exposure(h)
    for call in (lambda: gpu.luminance_histogram(c[..., :3]), lambda: gpu.luminance_histogram(c.double()), lambda: gpu.luminance_histogram(c, min_log2=-127),
                 lambda: gpu.luminance_histogram(c, min_log2=112), lambda: gpu.luminance_histogram(c, out=torch.zeros((2, 260), device=DEV)),
                 lambda: gpu.luminance_histogram(c, out=torch.zeros((1, 260), dtype=torch.int32, device=DEV)),
                 lambda: gpu.auto_exposure(h.float()), lambda: gpu.auto_exposure(h[:, :256]), lambda: gpu.auto_exposure(h, prev=e[:1]), lambda: gpu.auto_exposure(h, prev=e.cpu()),
                 lambda: gpu.auto_exposure(h, low=0.5, high=0.5), lambda: gpu.auto_exposure(h, low=-0.1), lambda: gpu.auto_exposure(h, high=1.1), lambda: gpu.auto_exposure(h, rate=0),
                 lambda: gpu.auto_exposure(h, rate=float("nan")), lambda: gpu.auto_exposure(h, key=0), lambda: gpu.auto_exposure(h, min_exposure=0),
                 lambda: gpu.auto_exposure(h, min_exposure=2, max_exposure=1), lambda: gpu.auto_exposure(h, max_exposure=float("inf")), lambda: gpu.auto_exposure(h, min_log2=300),
                 lambda: gpu.auto_exposure(h, out=torch.zeros((2, 3), device=DEV)),
                 lambda: gpu.tonemap(c, curve="filmic"), lambda: gpu.tonemap(c, white=0), lambda: gpu.tonemap(c, white=1e5), lambda: gpu.tonemap(c, exposure=-1),
                 lambda: gpu.tonemap(c, exposure=float("nan")), lambda: gpu.tonemap(c, exposure="bright"), lambda: gpu.tonemap(c, exposure=e[:1]), lambda: gpu.tonemap(c, exposure=e.double()),
                 lambda: gpu.tonemap(c, out=torch.zeros((2, 5, 6, 4), device=DEV)), lambda: gpu.tonemap(c, out=torch.zeros((2, 5, 6, 3), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            call()
    out = torch.zeros((2, 5, 6, 4), dtype=torch.uint8, device=DEV)
    assert gpu.tonemap(c, exposure=e, out=out) is out and torch.equal(out, gpu.tonemap(c, exposure=e))
    empty = torch.zeros((0, 5, 6, 4), device=DEV)
    assert tuple(gpu.luminance_histogram(empty).shape) == (0, 260) and tuple(gpu.tonemap(empty).shape) == (0, 5, 6, 4)


@pytest.mark.gpu
def test_display_device_refusals(gpu):
    L, A = gpu.lib(), gpu._abi
    V, H, W = 1, 16, 16
    c = dev(hist_inputs(V, H, W))
    hist = torch.zeros((V, 260), dtype=torch.int32, device=DEV)
    rec = torch.ones((V, 4), device=DEV)
    out = torch.zeros((V, H, W, 4), dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    err = lambda: L.gnxr_last_error()
    hp, ep, tp = A.HistogramParams(20, W, H, V, -12), A.ExposureParams(40, V, -12, 0, 0.18, 0.5, 0.95, 1.0, 2.0 ** -8, 2.0 ** 8), A.TonemapParams(32, W, H, V, 3, 3, 1.0, 4.0)
    assert L.gnxr_luminance_histogram_device(C.byref(hp), ptr(c), ptr(hist), None) == 0
    # host memory where device memory belongs
    hostbuf = np.zeros((H * W, 4), f32)
    hp_ = C.c_void_p(hostbuf.ctypes.data)
    assert hostbuf.ctypes.data % 16 == 0
    assert L.gnxr_luminance_histogram_device(C.byref(hp), hp_, ptr(hist), None) == ERR_INVALID and b"d_rgba is not device memory" in err()
    assert L.gnxr_luminance_histogram_device(C.byref(hp), ptr(c), hp_, None) == ERR_INVALID and b"d_hist is not device memory" in err()
    assert L.gnxr_exposure_device(C.byref(ep), hp_, None, ptr(rec), None) == ERR_INVALID and b"d_hist is not device memory" in err()
    assert L.gnxr_exposure_device(C.byref(ep), ptr(hist), hp_, ptr(rec), None) == ERR_INVALID and b"d_prev_exposure is not device memory" in err()
    assert L.gnxr_exposure_device(C.byref(ep), ptr(hist), None, hp_, None) == ERR_INVALID and b"d_exposure is not device memory" in err()
    assert L.gnxr_tonemap_device(C.byref(tp), hp_, None, ptr(out), None) == ERR_INVALID and b"d_rgba is not device memory" in err()
    assert L.gnxr_tonemap_device(C.byref(tp), ptr(c), hp_, ptr(out), None) == ERR_INVALID and b"d_exposure is not device memory" in err()
    assert L.gnxr_tonemap_device(C.byref(tp), ptr(c), None, hp_, None) == ERR_INVALID and b"d_rgba8_out is not device memory" in err()
    # an output that overlaps the input
    assert L.gnxr_tonemap_device(C.byref(tp), ptr(c), None, ptr(c), None) == ERR_INVALID and b"overlaps d_rgba" in err()
    assert L.gnxr_tonemap_device(C.byref(tp), ptr(c), None, C.c_void_p(c.data_ptr() + 16 * H * W - 4), None) == ERR_INVALID and b"overlaps d_rgba" in err()
    assert L.gnxr_luminance_histogram_device(C.byref(hp), ptr(c), ptr(c), None) == ERR_INVALID and b"overlaps" in err()
    assert L.gnxr_exposure_device(C.byref(ep), ptr(hist), None, ptr(hist), None) == ERR_INVALID and b"overlaps d_hist" in err()
    # a buffer shorter than V * H * W: an allocation of exactly 4096 bytes is 256 pixels, 260 are asked for
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))      # the runtime this process already runs on
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), 4096) == 0
    try:
        short = A.HistogramParams(20, 26, 10, 1, -12)
        assert L.gnxr_luminance_histogram_device(C.byref(short), small, ptr(hist), None) == ERR_INVALID and b"d_rgba" in err() and b"past the end of its allocation" in err()
        tshort = A.TonemapParams(32, 26, 10, 1, 3, 3, 1.0, 4.0)
        assert L.gnxr_tonemap_device(C.byref(tshort), small, None, ptr(out), None) == ERR_INVALID and b"d_rgba" in err() and b"past the end of its allocation" in err()
        # 1025 pixels of bytes do not fit 4096 bytes either; 1024 views of records do not fit them as histograms
        big_in = torch.zeros((1025, 4), device=DEV)
        bshort = A.TonemapParams(32, 1025, 1, 1, 3, 3, 1.0, 4.0)
        assert L.gnxr_tonemap_device(C.byref(bshort), ptr(big_in), None, small, None) == ERR_INVALID and b"d_rgba8_out" in err() and b"past the end" in err()
        eshort = A.ExposureParams(40, 4, -12, 0, 0.18, 0.5, 0.95, 1.0, 2.0 ** -8, 2.0 ** 8)
        recs = torch.ones((4, 4), device=DEV)
        assert L.gnxr_exposure_device(C.byref(eshort), small, None, ptr(recs), None) == ERR_INVALID and b"d_hist" in err() and b"past the end" in err()
    finally:
        assert hip.hipFree(small) == 0
    torch.cuda.synchronize()
    assert (host(hist).sum(1) == H * W).all()          # the refused calls queued nothing: the first call's histogram stands
