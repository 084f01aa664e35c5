"""The film (include/gnxr.h, "Film: pixel reconstruction filters"): gnxr_film_filter_table against numpy fp32 restatements, film_add +
film_resolve on synthetic samples against tests/film_reference.py, RenderFiltered against the composition camera_rays_device + Li +
sample_halton + the restatement, box 0.5 against Render, and the refusals.  Every comparison is on bits."""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import scenes
from conftest import ROOT
from film_reference import film_add_reference, film_resolve_reference

ERR_INVALID = -1
f32 = np.float32
KINDS = ("box", "triangle", "gaussian", "mitchell", "table")
TABLE_RADII = [(2.0, 2.0), (0.5, 3.0), (2.3, 1.1)]
ADD_RADII = [(0.5, 0.5), (1.5, 1.5), (2.0, 2.0), (4.0, 4.0), (0.5, 3.0), (2.3, 1.1)]
ADD_SIZES = [(1, 1, 1), (1, 3, 2), (1, 37, 23), (3, 19, 17)]   # (V, W, H)


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def caller_table():
    """a table no built-in kind produces: signs, a zero row and a huge entry"""
    t = (np.sin(np.arange(256, dtype=np.float64) * 0.37) * 2.0).astype(f32)
    t[32:48] = 0
    t[5] = f32(3e20)
    return t


def make_filter(gx, kind, radius):
    return gx.film_filter(kind, radius, alpha=1.5, B=0.4, C=0.3, table=caller_table() if kind == "table" else None)


# ---------------------------------------------------------------- the table, restated
def libm_expf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    return lambda v: f32(libm.expf(C.c_float(float(v))))


def mitchell_1d(t, B, Cc):
    x = np.abs(f32(2) * t)
    if x > 1:
        c3, c2 = -B - f32(6) * Cc, f32(6) * B + f32(30) * Cc
        c1, c0 = f32(-12) * B - f32(48) * Cc, f32(8) * B + f32(24) * Cc
        return (((((c3 * x) * x) * x + ((c2 * x) * x)) + (c1 * x)) + c0) * (f32(1) / f32(6))
    d3, d2, d0 = (f32(12) - f32(9) * B) - f32(6) * Cc, (f32(-18) + f32(12) * B) + f32(6) * Cc, f32(6) - f32(2) * B
    return (((((d3 * x) * x) * x) + ((d2 * x) * x)) + d0) * (f32(1) / f32(6))


def table_restated(kind, rx, ry, a, b, table):
    rx, ry, a, b = f32(rx), f32(ry), f32(a), f32(b)
    expf = libm_expf()
    out = np.zeros((16, 16), f32)
    zero = f32(0)
    if kind == "gaussian":
        expX, expY = expf(((-a) * rx) * rx), expf(((-a) * ry) * ry)
    for y in range(16):
        for x in range(16):
            px, py = ((f32(x) + f32(0.5)) * rx) / f32(16), ((f32(y) + f32(0.5)) * ry) / f32(16)
            if kind == "box":
                v = f32(1)
            elif kind == "triangle":
                v = max(zero, rx - np.abs(px)) * max(zero, ry - np.abs(py))
            elif kind == "gaussian":
                v = max(zero, expf(((-a) * px) * px) - expX) * max(zero, expf(((-a) * py) * py) - expY)
            elif kind == "mitchell":
                v = mitchell_1d(px / rx, a, b) * mitchell_1d(py / ry, a, b)
            else:
                v = table[y * 16 + x]
            out[y, x] = v
    return out


# ---------------------------------------------------------------- CPU
def test_film_entry_points_declared_exported_and_bound(gx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnxr.h")).read(), flags=re.S)
    for name in ("gnxr_film_filter_table", "gnxr_film_add_device", "gnxr_film_resolve_device", "gnxr_render_filtered_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(gx.lib(), name) and name in gx._abi.PROTOTYPES, name
    assert C.sizeof(gx._abi.FilmFilter) == 32
    for cls in (gx.PathIntegrator, gx.VolPathIntegrator, gx.WhittedIntegrator, gx.DirectLightingIntegrator):
        assert cls.RenderFiltered is gx.PathIntegrator.RenderFiltered


@pytest.mark.parametrize("radius", TABLE_RADII)
@pytest.mark.parametrize("kind", KINDS)
def test_filter_table_against_the_restatement(gx, kind, radius):
    f = make_filter(gx, kind, radius)
    got = gx.film_filter_table(f)
    want = table_restated(kind, radius[0], radius[1], f.a, f.b, caller_table())
    assert got.shape == (16, 16) and got.dtype == np.float32
    assert biteq(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    assert np.isfinite(got).all() and got.any()
    if kind in ("triangle", "gaussian", "mitchell"):   # not a constant, falling off along x
        assert got[0, 0] > got[0, 15]


def test_filter_tables_differ_by_kind_and_radius(gx):
    for r in TABLE_RADII:
        tabs = [gx.film_filter_table(make_filter(gx, k, r)).tobytes() for k in KINDS]
        assert len(set(tabs)) == len(tabs), r
    for k in ("triangle", "gaussian"):   # (Mitchell is a function of the offset over the radius: its table is the same at every radius)
        tabs = [gx.film_filter_table(make_filter(gx, k, r)).tobytes() for r in TABLE_RADII]
        assert len(set(tabs)) == len(tabs), k
    g2, g3 = gx.film_filter_table(gx.film_filter("gaussian", 2.0, alpha=2.0)), gx.film_filter_table(gx.film_filter("gaussian", 2.0, alpha=3.0))
    assert not biteq(g2, g3)


def raw_filter(gx, kind=0, rx=2.0, ry=2.0, size=None, table=None):
    return gx._abi.FilmFilter(C.sizeof(gx._abi.FilmFilter) if size is None else size, kind, rx, ry, 2.0, 0.0, table)


def bad_filters(gx):
    nan = float("nan")
    return {"mis-sized": raw_filter(gx, size=28), "kind 5": raw_filter(gx, kind=5), "kind -1": raw_filter(gx, kind=-1), "rx 0.4": raw_filter(gx, rx=0.4),
            "ry 4.5": raw_filter(gx, ry=4.5), "rx nan": raw_filter(gx, rx=nan), "ry nan": raw_filter(gx, ry=nan), "table null": raw_filter(gx, kind=4)}


def test_refusals_that_need_no_device(gx):
    """a bad record is refused by every entry point before a device is looked for; the output stays untouched"""
    lib = gx.lib()
    out = np.full(256, 7.0, f32)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.gnxr_film_filter_table(None, po) == ERR_INVALID
    assert lib.gnxr_film_filter_table(C.byref(raw_filter(gx)), None) == ERR_INVALID
    for what, f in bad_filters(gx).items():
        assert lib.gnxr_film_filter_table(C.byref(f), po) == ERR_INVALID, what
        # (the pointers are never read: the record is checked first)
        assert lib.gnxr_film_add_device(C.byref(f), 4, 4, 1, 1, None, None, None, None) == ERR_INVALID, what
    assert (out == 7.0).all()
    ok = raw_filter(gx)
    assert lib.gnxr_film_add_device(None, 4, 4, 1, 1, None, None, None, None) == ERR_INVALID
    for w, h, v, n in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, -1, 1), (4, 4, 1, -1), (1 << 16, 1 << 16, 1, 1)):
        assert lib.gnxr_film_add_device(C.byref(ok), w, h, v, n, None, None, None, None) == ERR_INVALID, (w, h, v, n)
    for w, h, v in ((0, 4, 1), (4, -1, 1), (4, 4, -2), (1 << 16, 1 << 16, 1)):
        assert lib.gnxr_film_resolve_device(w, h, v, None, None, None) == ERR_INVALID, (w, h, v)
    # null arrays and misaligned ones are found before the device too
    assert lib.gnxr_film_add_device(C.byref(ok), 4, 4, 1, 1, None, None, None, None) == ERR_INVALID
    assert lib.gnxr_film_add_device(C.byref(ok), 4, 4, 1, 1, C.c_void_p(4096), C.c_void_p(4096 + 4), C.c_void_p(8192), None) == ERR_INVALID
    assert lib.gnxr_film_resolve_device(4, 4, 1, C.c_void_p(4096 + 8), C.c_void_p(8192), None) == ERR_INVALID
    # no-ops
    assert lib.gnxr_film_add_device(C.byref(ok), 4, 4, 0, 1, None, None, None, None) == 0
    assert lib.gnxr_film_add_device(C.byref(ok), 4, 4, 1, 0, None, None, None, None) == 0
    assert lib.gnxr_film_resolve_device(4, 4, 0, None, None, None) == 0
    assert lib.gnxr_render_filtered_device(None, None, C.byref(ok), None, None, 1, None, None, 0, None, None) == ERR_INVALID


def test_python_argument_errors(gx):
    for args, kw in ((("boxy", 2.0), {}), (("box", 0.4), {}), (("box", (2.0, 4.5)), {}), (("box", float("nan")), {}), (("box", (1.0, 2.0, 3.0)), {}), (("box", "wide"), {}),
                     (("table", 2.0), {}), (("table", 2.0), {"table": np.zeros(255)}), (("box", 2.0), {"table": np.zeros(256)}), (("gaussian", 2.0), {"alpha": float("nan")})):
        with pytest.raises(ValueError):
            gx.film_filter(*args, **kw)
    f = gx.film_filter("gaussian", (0.5, 4.0))
    assert (f.kind, f.radius_x, f.radius_y, f.a) == (2, 0.5, 4.0, 2.0)
    m = gx.film_filter("mitchell", 2)
    assert (m.a, m.b) == (f32(1 / 3), f32(1 / 3))
    with pytest.raises(ValueError):
        gx.film_filter_table("gaussian")
    acc = torch.zeros((4, 4, 4))
    with pytest.raises(ValueError):   # host tensors
        gx.film_add(f, torch.zeros((1, 4, 4, 4)), torch.zeros((1, 4, 4, 2)), acc)
    with pytest.raises(ValueError):
        gx.film_resolve(acc)
    with pytest.raises(ValueError):
        gx.film_resolve(np.zeros((4, 4, 4), f32))
    integ = gx.PathIntegrator(5, 1.0, "spatial")
    for kw in (dict(filter="gaussian"), dict(filter=f, media=[-1]), dict(filter=f, resume=True), dict(filter=f, shard_index=1), dict(filter=f, cameras=["cam"])):
        with pytest.raises(ValueError):
            integ.RenderFiltered(None, 8, 8, 4, **kw)
    with pytest.raises(ValueError):
        integ.RenderFiltered(None, 0, 8, 4, f)


def test_reference_box_is_the_plain_mean():
    """the restatement itself: with every weight 1 and radius 0.5 a sample with an offset inside (0, 1) reaches its own pixel only"""
    rng = np.random.default_rng(5)
    L = rng.random((3, 1, 5, 7, 4)).astype(f32)
    off = (rng.random((3, 1, 5, 7, 2)) * 0.98 + 0.01).astype(f32)
    acc = film_add_reference(np.ones(256, f32), 0.5, 0.5, L, off, np.zeros((1, 5, 7, 4), f32))
    want = (L[0] + L[1]) + L[2]
    assert biteq(acc[..., :3], want[..., :3]) and (acc[..., 3] == 3).all()
    assert biteq(film_resolve_reference(acc)[..., :3], want[..., :3] / f32(3))
    # an offset of exactly 0 also reaches the pixel to the left
    off[0, 0, 2, 3] = (0.0, 0.5)
    acc = film_add_reference(np.ones(256, f32), 0.5, 0.5, L, off, np.zeros((1, 5, 7, 4), f32))
    assert acc[0, 2, 2, 3] == 4 and acc[0, 2, 3, 3] == 3 and acc[0, 2, 4, 3] == 3
    r = film_resolve_reference(np.array([[0, 1, -1, 0], [2, -4, np.nan, 2], [1, 1, 1, -1]], f32))
    assert biteq(r, np.array([[0, 0, 0, 1], [1, 0, np.nan, 1], [0, 0, 0, 1]], f32))


# ---------------------------------------------------------------- GPU: film_add + film_resolve on synthetic samples
def synthetic(V, W, H, n, seed):
    """n layers of samples with the awkward entries the definition names, and a non-zero starting accumulator"""
    rng = np.random.default_rng(seed)
    L = (rng.standard_normal((n, V, H, W, 4)) * 3).astype(f32)        # negative values included
    off = rng.random((n, V, H, W, 2)).astype(f32)
    flatL, flato = L.reshape(-1, 4), off.reshape(-1, 2)
    m = flato.shape[0]
    # spread over the layers; an image of a few pixels keeps its first sample plain and takes the entries that fit, the later ones winning
    at = lambda k: (k * 7919) % m if m >= 64 else 1 + k % (m - 1)
    flato[at(1)] = (0.0, 0.3); flato[at(2)] = (0.6, 0.0); flato[at(3)] = (0.0, 0.0)
    one_m = f32(1) - f32(2.0 ** -24)
    flato[at(4)] = (one_m, 0.5); flato[at(5)] = (0.5, one_m); flato[at(6)] = (one_m, one_m); flato[at(7)] = (1.0, 1.0)
    flato[at(8)] = (-0.25, 0.5); flato[at(9)] = (0.5, 1.5); flato[at(10)] = (np.nan, 0.5); flato[at(11)] = (0.5, np.nan); flato[at(12)] = (-0.0, 0.5)
    flatL[at(13), :3] = (3e37, -3e37, 1e30)
    flatL[at(14), 0] = np.nan; flatL[at(15), 1] = np.inf; flatL[at(16), 2] = -np.inf
    flatL[at(8), 0] = np.nan   # a NaN on a sample that adds nothing poisons nothing
    acc0 = rng.random((V, H, W, 4)).astype(f32)
    acc0[..., 3] += f32(0.5)
    return L, off, acc0


@pytest.mark.gpu
@pytest.mark.parametrize("radius", ADD_RADII)
@pytest.mark.parametrize("size", ADD_SIZES)
def test_film_add_and_resolve_against_the_restatement(gpu, size, radius):
    """1 and 5 layers on a non-zero accumulator, 5 layers against 2 + 3, and the in-place resolve on a side stream"""
    V, W, H = size
    kind = KINDS[(ADD_SIZES.index(size) + ADD_RADII.index(radius)) % len(KINDS)]
    f = make_filter(gpu, kind, radius)
    table = gpu.film_filter_table(f)
    L, off, acc0 = synthetic(V, W, H, 5, seed=W * 100 + H)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dL, doff = dev(L), dev(off)
    shape = (V, H, W, 4) if V > 1 else (H, W, 4)
    lay = lambda t, n0, n1: t[n0:n1].reshape((n1 - n0,) + shape[:-1] + (t.shape[-1],)).contiguous()
    want1 = film_add_reference(table, radius[0], radius[1], L[:1], off[:1], acc0)
    want5 = film_add_reference(table, radius[0], radius[1], L, off, acc0)
    assert W * H < 100 or (not biteq(want1, acc0) and not biteq(want5, want1))   # (a single pixel may meet a zero of the table)
    a1 = dev(acc0).reshape(shape)
    assert gpu.film_add(f, lay(dL, 0, 1), lay(doff, 0, 1), a1) is a1
    a5 = dev(acc0).reshape(shape)
    gpu.film_add(f, lay(dL, 0, 5), lay(doff, 0, 5), a5)
    a23 = dev(acc0).reshape(shape)
    gpu.film_add(f, lay(dL, 0, 2), lay(doff, 0, 2), a23)
    gpu.film_add(f, lay(dL, 2, 5), lay(doff, 2, 5), a23)
    img = gpu.film_resolve(a5)
    side = torch.cuda.Stream()
    aside = dev(acc0).reshape(shape)
    torch.cuda.synchronize()
    gpu.film_add(f, lay(dL, 0, 5), lay(doff, 0, 5), aside, stream=side)
    assert gpu.film_resolve(aside, out=aside, stream=side) is aside
    side.synchronize()
    torch.cuda.synchronize()
    got = lambda t: t.cpu().numpy().reshape(V, H, W, 4)
    nan_px = int(np.isnan(want5).any(axis=-1).sum())
    print(f"{kind} {radius} {V}x{W}x{H}: {nan_px} poisoned pixels of {V * W * H}")
    assert biteq(got(a1), want1)
    assert biteq(got(a5), want5)
    assert biteq(got(a23), want5)
    want_img = film_resolve_reference(want5)
    assert biteq(got(img), want_img) and (got(img)[..., 3] == 1).all()
    assert biteq(got(aside), want_img)
    if W * H > 100:   # the NaN / Inf samples poison some pixels and not all
        assert 0 < nan_px < V * W * H


@pytest.mark.gpu
def test_film_add_keeps_views_apart(gpu):
    """samples of one view alone: the other views' accumulators keep their bits"""
    V, W, H = 3, 19, 17
    f = make_filter(gpu, "gaussian", 4.0)
    L, off, acc0 = synthetic(V, W, H, 2, seed=3)
    off[:, 0] = np.nan; off[:, 2] = np.nan
    a = torch.from_numpy(acc0).cuda()
    gpu.film_add(f, torch.from_numpy(L).cuda(), torch.from_numpy(off).cuda(), a)
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    assert biteq(got[0], acc0[0]) and biteq(got[2], acc0[2]) and not biteq(got[1], acc0[1])
    assert biteq(got, film_add_reference(gpu.film_filter_table(f), 4.0, 4.0, L, off, acc0))


# ---------------------------------------------------------------- GPU: RenderFiltered against the composition
def integrator(gx, kind):
    return {"path": lambda: gx.PathIntegrator(5, 1.0, "spatial"), "volpath": lambda: gx.VolPathIntegrator(5, 1.0, "spatial"),
            "whitted": lambda: gx.WhittedIntegrator(5), "direct": lambda: gx.DirectLightingIntegrator("all", 5)}[kind]()


def builder(kind):
    return scenes.volume_cornell() if kind == "volpath" else scenes.cornell()


def samples_of(gpu, integ, scene, W, H, B, cam=None):
    """(L[s, y, x, 4], offsets[s, y, x, 2]) of the composition: integrator.Li on camera_rays_device rays, sample_halton dimensions 0 and 1"""
    s, py, px = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij"))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    rays, samples = gpu.camera_rays_device(cam if cam is not None else gpu.camera(), W, H, dev(px), dev(py), dev(s))
    L, _ = integ.Li(scene, rays, samples, W, H, B)
    torch.cuda.synchronize()
    off = np.stack([gpu.sample_halton(W, H, px, py, s, np.full(len(px), d)) for d in (0, 1)], axis=-1)
    return L.cpu().numpy().reshape(B, H, W, 4).copy(), off.reshape(B, H, W, 2).astype(f32)


def composed(gpu, f, L, off, s0=0, s1=None, acc=None):
    """the accumulator (V, H, W, 4) after samples [s0, s1) of L / off (B, V, H, W, .)"""
    acc = np.zeros(L.shape[1:4] + (4,), f32) if acc is None else acc
    return film_add_reference(gpu.film_filter_table(f), f.radius_x, f.radius_y, L[s0:s1], off[s0:s1], acc)


def rendered(integ, scene, W, H, B, f, **kw):
    img, st = integ.RenderFiltered(scene, W, H, B, f, **kw)
    torch.cuda.synchronize()
    return img.cpu().numpy(), st


@pytest.mark.gpu
@pytest.mark.parametrize("kind,radius", [("gaussian", 2.0), ("mitchell", 2.0)])
def test_render_filtered_cornell_against_the_composition(gpu, kind, radius):
    W, H, B = 16, 12, 4
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter(kind, radius)
    L, off = samples_of(gpu, integ, scene, W, H, B)
    want = composed(gpu, f, L[:, None], off[:, None])
    acc = torch.full((H, W, 4), 5.0, device="cuda")   # not resumed: zeroed first
    img, st = rendered(integ, scene, W, H, B, f, accum=acc)
    assert biteq(acc.cpu().numpy(), want[0])
    assert biteq(img, film_resolve_reference(want[0])) and img[..., :3].any()
    assert st["camera_samples"] == W * H * B
    plain, _ = integ.Render(scene, W, H, B)
    assert not biteq(img, plain)
    img2, _ = rendered(integ, scene, W, H, B, f)   # the accumulator inside the library
    assert biteq(img2, img)
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["path", "volpath", "whitted", "direct"])
def test_render_filtered_all_integrators(gpu, kind):
    W, H, B = 12, 9, 8
    integ = integrator(gpu, kind)
    scene = gpu.Scene(builder(kind))
    f = gpu.film_filter("gaussian", (2.0, 1.5))
    L, off = samples_of(gpu, integ, scene, W, H, B)
    want = film_resolve_reference(composed(gpu, f, L[:, None], off[:, None])[0])
    img, _ = rendered(integ, scene, W, H, B, f)
    assert biteq(img, want) and img[..., :3].any()
    scene.close()


@pytest.mark.gpu
def test_render_filtered_does_not_depend_on_the_pass_plan(gpu):
    """samples_per_pass = 3 of 8 spp (ragged sub-passes) x passes_in_flight 1 and 4, against the automatic plan: equal bits"""
    W, H, B = 12, 9, 8
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter("mitchell", 2.0)
    base, _ = rendered(integ, scene, W, H, B, f)
    assert base[..., :3].any()
    for spp_pass in (3, 0):
        for in_flight in (1, 4):
            img, st = rendered(integ, scene, W, H, B, f, samples_per_pass=spp_pass, passes_in_flight=in_flight)
            assert biteq(img, base), (spp_pass, in_flight)
            if spp_pass == 3:
                assert st["passes"] == 3
    wh = integrator(gpu, "whitted")
    a, _ = rendered(wh, scene, W, H, B, f)
    b, st = rendered(wh, scene, W, H, B, f, samples_per_pass=3)
    assert biteq(a, b) and st["passes"] == 3
    scene.close()


@pytest.mark.gpu
def test_render_filtered_views_do_not_bleed(gpu):
    """three cameras at 11 x 7: the call equals the three single-view calls, and view 1 the composition through its camera"""
    W, H, B = 11, 7, 4
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter("gaussian", 3.0)
    cams = [gpu.camera(), gpu.camera(eye=(1.5, 0.5, 5), look=(0, -0.5, 0)), gpu.camera(eye=(-2, 1, 4), fov=70.0)]
    acc = torch.zeros((3, H, W, 4), device="cuda")
    img, st = rendered(integ, scene, W, H, B, f, cameras=cams, accum=acc)
    assert img.shape == (3, H, W, 4) and st["camera_samples"] == 3 * W * H * B
    for v, cam in enumerate(cams):
        acc1 = torch.zeros((1, H, W, 4), device="cuda")
        one, _ = rendered(integ, scene, W, H, B, f, cameras=[cam], accum=acc1)
        assert biteq(one[0], img[v]) and biteq(acc1.cpu().numpy()[0], acc.cpu().numpy()[v]), v
    assert not biteq(img[0], img[1]) and not biteq(img[0], img[2])
    own, _ = rendered(integ, scene, W, H, B, f)   # the scene's own camera is view 0's
    assert biteq(own, img[0])
    L, off = samples_of(gpu, integ, scene, W, H, B, cam=cams[1])
    assert biteq(img[1], film_resolve_reference(composed(gpu, f, L[:, None], off[:, None])[0]))
    scene.close()


@pytest.mark.gpu
def test_render_filtered_resumed(gpu):
    """[0, 3) followed by [3, 8) resumed leaves the accumulator and the image of [0, 8)"""
    W, H, B = 12, 9, 8
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter("gaussian", 2.0)
    full = torch.zeros((H, W, 4), device="cuda")
    img_full, _ = rendered(integ, scene, W, H, B, f, accum=full)
    part = torch.full((H, W, 4), 9.0, device="cuda")
    img_a, _ = rendered(integ, scene, W, H, B, f, accum=part, spp_begin=0, spp_end=3)
    after_a = part.cpu().numpy().copy()
    img_b, _ = rendered(integ, scene, W, H, B, f, accum=part, resume=True, spp_begin=3, spp_end=8)
    assert biteq(part.cpu().numpy(), full.cpu().numpy()) and biteq(img_b, img_full)
    assert not biteq(after_a, full.cpu().numpy()) and not biteq(img_a, img_full)
    L, off = samples_of(gpu, integ, scene, W, H, B)
    assert biteq(after_a, composed(gpu, f, L[:, None], off[:, None], 0, 3)[0])
    scene.close()


# ---------------------------------------------------------------- GPU: box 0.5 meets Render
@pytest.mark.gpu
def test_box_half_meets_render(gpu):
    W, H, B = 16, 12, 4
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter("box", 0.5)
    acc = torch.zeros((H, W, 4), device="cuda")
    img, _ = rendered(integ, scene, W, H, B, f, accum=acc)
    plain, _ = integ.Render(scene, W, H, B)
    wt = acc.cpu().numpy()[..., 3]
    own = wt == B
    print("pixels with Wt == spp:", int(own.sum()), "of", W * H, "| Wt values:", sorted(set(wt.reshape(-1).tolist())))
    assert biteq(img[own], plain[own]) and plain[..., :3].any()
    L, off = samples_of(gpu, integ, scene, W, H, B)
    assert biteq(img, film_resolve_reference(composed(gpu, f, L[:, None], off[:, None])[0]))
    assert own.sum() >= 0.8 * W * H
    scene.close()


# ---------------------------------------------------------------- GPU: refusals leave the outputs untouched
@pytest.mark.gpu
def test_device_refusals_leave_the_outputs_untouched(gpu):
    lib = gpu.lib()
    W, H = 8, 6
    ok = raw_filter(gpu)
    acc = torch.full((H, W, 4), 3.0, device="cuda")
    out = torch.full((H, W, 4), 4.0, device="cuda")
    L = torch.ones((2, H, W, 4), device="cuda")
    off = torch.full((2, H, W, 2), 0.5, device="cuda")
    host = np.zeros((2, H, W, 4), f32)
    p = lambda t, d=0: C.c_void_p(t.data_ptr() + d)
    hp = C.c_void_p(host.ctypes.data)
    add = lambda f, n, l, o, a: lib.gnxr_film_add_device(f, W, H, 1, n, l, o, a, None)
    for what, rc in {"bad record": [add(C.byref(f), 2, p(L), p(off), p(acc)) for f in bad_filters(gpu).values()],
                     "null record": [add(None, 2, p(L), p(off), p(acc))],
                     "negative layers": [add(C.byref(ok), -1, p(L), p(off), p(acc))],
                     "null arrays": [add(C.byref(ok), 2, None, p(off), p(acc)), add(C.byref(ok), 2, p(L), None, p(acc)), add(C.byref(ok), 2, p(L), p(off), None)],
                     "misaligned": [add(C.byref(ok), 1, p(L, 8), p(off), p(acc)), add(C.byref(ok), 1, p(L), p(off, 4), p(acc)), add(C.byref(ok), 1, p(L), p(off), p(out, 8))],
                     "host memory": [add(C.byref(ok), 2, hp, p(off), p(acc)), add(C.byref(ok), 2, p(L), hp, p(acc)), add(C.byref(ok), 2, p(L), p(off), hp)],
                     "overlap": [add(C.byref(ok), 1, p(L), p(off), p(L, 16))],
                     "resolve": [lib.gnxr_film_resolve_device(W, H, 1, hp, p(out), None), lib.gnxr_film_resolve_device(W, H, 1, p(acc), hp, None),
                                 lib.gnxr_film_resolve_device(W, H, 1, p(acc, 4), p(out), None), lib.gnxr_film_resolve_device(W, H, 1, p(acc), None, None),
                                 lib.gnxr_film_resolve_device(W, H, 1, p(L), p(L, 16), None)]}.items():
        assert rc and all(r == ERR_INVALID for r in rc), (what, rc)
    # the render
    integ = integrator(gpu, "path")
    scene = gpu.Scene(builder("path"))
    f = gpu.film_filter("gaussian", 2.0)
    st = gpu.Stats()
    cams = (gpu.Camera * 2)(gpu.camera(), gpu.camera())

    def render(filt=f, cameras=None, media=None, n_views=1, d_out=p(out), d_acc=p(acc), flags=0, **kw):
        params = integ.params(W, H, 4, **kw)
        return lib.gnxr_render_filtered_device(scene._h, C.byref(params), C.byref(filt) if filt is not None else None, cameras, media, n_views, d_out, d_acc, flags, None, C.byref(st))

    bad_media = (C.c_int32 * 2)(-1, 7)
    rcs = {"bad records": [render(filt=b) for b in bad_filters(gpu).values()], "null record": [render(filt=None)],
           "views without cameras": [render(n_views=2)], "negative views": [render(cameras=cams, n_views=-1)], "no output": [render(d_out=None, d_acc=None)],
           "misaligned": [render(d_out=p(out, 8)), render(d_acc=p(acc, 4))], "host memory": [render(d_out=hp), render(d_acc=hp)],
           "flags": [render(flags=2), render(flags=0x80000001)],
           "shards": [render(shard_index=1, shard_count=2), render(shard_count=2), render(shard_rows=4)],
           "samples": [render(spp_begin=4), render(spp_end=5), render(spp_begin=3, spp_end=2)], "media": [render(cameras=cams, media=bad_media, n_views=2)],
           "the same buffer twice": [render(d_out=p(acc))]}
    for what, rc in rcs.items():
        assert rc and all(r == ERR_INVALID for r in rc), (what, rc)
    torch.cuda.synchronize()
    assert (acc == 3.0).all() and (out == 4.0).all() and (L == 1.0).all()
    # no-ops
    assert render(cameras=cams, n_views=0) == 0 and add(C.byref(ok), 0, p(L), p(off), p(acc)) == 0
    torch.cuda.synchronize()
    assert (acc == 3.0).all() and (out == 4.0).all()
    # and an accepted call writes both; the accumulator alone is enough
    assert render() == 0 and render(d_out=None) == 0
    torch.cuda.synchronize()
    assert not (acc == 3.0).all() and not (out == 4.0).all()
    scene.close()
