"""The arrays of the twelve entry points on device memory that take no scene (include/gnxr.h): one table row per entry point -- how to
call it, its arrays in the order the call lists them, their byte extents and alignments, its message prefix -- and the same checks for
every row.  Without a device: a misaligned array is refused by name, an output that overlaps an input it must not is refused, the empty
call returns 0 and arguments that pass every check ask for the runtime.  On the GPU: every call succeeds once on device memory, a host
array in any position and an allocation shorter than the call's extent are refused by name, and the refused calls queue nothing."""
import ctypes as C

import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

ERR_INVALID, ERR_NO_DEVICE = -1, -2
DEV = "cuda:0"


def vp(address):
    return C.c_void_p(address) if address else None


# ---------------------------------------------------------------- the calls: p maps an array's name to its address (0: not given), s is the shape
def call_camera_rays(L, A, p, s):
    cam = A.Camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 0.0, 1.0, 0)
    return L.gnxr_camera_rays_device(C.byref(cam), -1, 8, 8, vp(p["d_px"]), vp(p["d_py"]), vp(p["d_s"]), s["n"], vp(p["d_rays"]), vp(p["d_samples"]), None)


def call_sh_project(L, A, p, s):
    return L.gnxr_sh_project_device(vp(p["d_rays"]), vp(p["d_L"]), s["P"], s["S"], vp(p["d_sh_sum"]), 0, None)


def call_sh_irradiance(L, A, p, s):
    return L.gnxr_sh_irradiance_device(vp(p["d_sh"]), s["P"], vp(p["d_probe"]), vp(p["d_normals"]), s["n"], vp(p["d_E"]), None)


def call_film_add(L, A, p, s):
    f = A.FilmFilter(C.sizeof(A.FilmFilter), A.FILTER_BOX, 0.5, 0.5, 0.0, 0.0, None)
    return L.gnxr_film_add_device(C.byref(f), s["W"], s["H"], s["V"], 1, vp(p["d_L"]), vp(p["d_offsets"]), vp(p["d_accum"]), None)


def call_film_resolve(L, A, p, s):
    return L.gnxr_film_resolve_device(s["W"], s["H"], s["V"], vp(p["d_accum"]), vp(p["d_rgba_out"]), None)


def call_denoise(L, A, p, s):
    dp = A.DenoiseParams(C.sizeof(A.DenoiseParams), s["W"], s["H"], s["V"], 1, 1.0, 1.0, 1.0)
    db = A.DenoiseBuffers(C.sizeof(A.DenoiseBuffers), 0, *(p[w] or None for w in ("d_color", "d_color_b", "d_albedo", "d_normal", "d_depth")))
    return L.gnxr_denoise_device(C.byref(dp), C.byref(db), vp(p["d_rgba_out"]), None)


TEMPORAL = ("d_color", "d_motion", "d_guide", "d_prim", "d_hist_color", "d_hist_stat", "d_hist_guide", "d_hist_prim", "d_out_color", "d_out_stat")


def call_temporal(L, A, p, s):
    tp = A.TemporalParams(C.sizeof(A.TemporalParams), s["W"], s["H"], s["V"], 8, 0.1, 0.9)
    tb = A.TemporalBuffers(C.sizeof(A.TemporalBuffers), 0, *(p[w] or None for w in TEMPORAL))
    return L.gnxr_temporal_accumulate_device(C.byref(tp), C.byref(tb), None)


def call_histogram(L, A, p, s):
    hp = A.HistogramParams(C.sizeof(A.HistogramParams), s["W"], s["H"], s["V"], -12)
    return L.gnxr_luminance_histogram_device(C.byref(hp), vp(p["d_rgba"]), vp(p["d_hist"]), None)


def call_exposure(L, A, p, s):
    ep = A.ExposureParams(C.sizeof(A.ExposureParams), s["V"], -12, 0, 0.18, 0.5, 0.95, 1.0, 2.0 ** -8, 2.0 ** 8)
    return L.gnxr_exposure_device(C.byref(ep), vp(p["d_hist"]), vp(p["d_prev_exposure"]), vp(p["d_exposure"]), None)


def call_tonemap(L, A, p, s):
    tp = A.TonemapParams(C.sizeof(A.TonemapParams), s["W"], s["H"], s["V"], A.TONEMAP_ACES, A.TONEMAP_SRGB | A.TONEMAP_ROUND, 1.0, 4.0)
    return L.gnxr_tonemap_device(C.byref(tp), vp(p["d_rgba"]), vp(p["d_exposure"]), vp(p["d_rgba8_out"]), None)


def call_dilate(L, A, p, s):
    return L.gnxr_bake_dilate_device(s["W"], s["H"], 1, vp(p["d_rgba"]), None)


def call_skin(L, A, p, s):
    sp = A.SkinParams(C.sizeof(A.SkinParams), s["V"], s["B"], s["M"])
    return L.gnxr_skin_vertices_device(C.byref(sp), vp(p["d_rest"]), vp(p["d_bone_index"]), vp(p["d_bone_weight"]), vp(p["d_bones"]), vp(p["d_morph_delta"]),
                                       vp(p["d_morph_weight"]), vp(p["d_out"]), None)


# ---------------------------------------------------------------- the table
# arrays(s): (name, bytes, alignment, contents) in the order of the call's own list.  Contents on the GPU: "f" floats in [0.1, 1), "h" the
#   same in the first half and 0 after it (a dilation needs filled and unfilled texels), "0" zeros (indices that are in range, outputs).
# prefix: what every message of the call starts with; hint: what follows "is not device memory".
# named: the call has one alignment message per array, "<prefix><what> is not <k>-byte aligned" (else one message that names several).
# overlaps: (output, input, in place allowed) -- the same address is refused as well unless the call allows the output to BE that input.
# after_walk: the overlap test comes after the arrays were found on a device, so its rows need one.
# small / big / empty: the smallest shape with every array, one where the arrays of `past` need more than 4096 bytes, the empty call.
# past: an input and an output that are tried on an allocation of 4096 bytes.
IMAGE, BIG_IMAGE, NO_VIEWS = dict(W=8, H=8, V=1), dict(W=40, H=32, V=1), dict(W=8, H=8, V=0)


def px(s):
    return s["W"] * s["H"] * s["V"]


ENTRIES = [
    dict(name="gnxr_camera_rays_device", call=call_camera_rays, prefix=b"", hint=b" (host arrays go through gnxr_camera_rays)", named=False,
         arrays=lambda s: [("d_px", 4 * s["n"], 4, "0"), ("d_py", 4 * s["n"], 4, "0"), ("d_s", 4 * s["n"], 4, "0"), ("d_rays", 32 * s["n"], 16, "0"), ("d_samples", 16 * s["n"], 16, "0")],
         overlaps=(), small=dict(n=4), big=dict(n=2048), empty=dict(n=0), past=("d_px", "d_rays")),
    dict(name="gnxr_sh_project_device", call=call_sh_project, prefix=b"gnxr_sh_project_device: ", hint=b"", named=False,
         arrays=lambda s: [("d_sh_sum", 144 * s["P"], 16, "0"), ("d_rays", 32 * s["P"] * s["S"], 16, "f"), ("d_L", 16 * s["P"] * s["S"], 16, "f")],
         overlaps=(), small=dict(P=2, S=2), big=dict(P=32, S=16), empty=dict(P=0, S=2), past=("d_L", "d_sh_sum")),
    dict(name="gnxr_sh_irradiance_device", call=call_sh_irradiance, prefix=b"gnxr_sh_irradiance_device: ", hint=b"", named=False,
         arrays=lambda s: [("d_E", 16 * s["n"], 16, "0"), ("d_probe", 4 * s["n"], 4, "0"), ("d_normals", 12 * s["n"], 4, "f"), ("d_sh", 144 * s["P"], 16, "f")],
         overlaps=(), small=dict(P=2, n=4), big=dict(P=32, n=2048), empty=dict(P=2, n=0), past=("d_probe", "d_E")),
    dict(name="gnxr_film_add_device", call=call_film_add, prefix=b"film_add: ", hint=b"", named=True,
         arrays=lambda s: [("d_accum", 16 * px(s), 16, "f"), ("d_L", 16 * px(s), 16, "f"), ("d_offsets", 8 * px(s), 8, "f")],
         overlaps=(("d_accum", "d_L", False), ("d_accum", "d_offsets", False)), after_walk=True, small=IMAGE, big=BIG_IMAGE, empty=NO_VIEWS, past=("d_offsets", "d_accum")),
    dict(name="gnxr_film_resolve_device", call=call_film_resolve, prefix=b"film_resolve: ", hint=b"", named=True,
         arrays=lambda s: [("d_accum", 16 * px(s), 16, "f"), ("d_rgba_out", 16 * px(s), 16, "0")],
         overlaps=(("d_rgba_out", "d_accum", True),), after_walk=True, small=IMAGE, big=BIG_IMAGE, empty=NO_VIEWS, past=("d_accum", "d_rgba_out")),
    dict(name="gnxr_denoise_device", call=call_denoise, prefix=b"denoise: ", hint=b"", named=True,
         arrays=lambda s: [("d_color", 16 * px(s), 16, "f"), ("d_color_b", 16 * px(s), 16, "f"), ("d_albedo", 16 * px(s), 16, "f"), ("d_normal", 16 * px(s), 16, "f"),
                           ("d_depth", 4 * px(s), 4, "f"), ("d_rgba_out", 16 * px(s), 16, "0")],
         overlaps=(("d_rgba_out", "d_color", True), ("d_rgba_out", "d_color_b", True), ("d_rgba_out", "d_albedo", False), ("d_rgba_out", "d_normal", False),
                   ("d_rgba_out", "d_depth", False)),
         small=IMAGE, big=BIG_IMAGE, empty=NO_VIEWS, past=("d_depth", "d_rgba_out")),
    dict(name="gnxr_temporal_accumulate_device", call=call_temporal, prefix=b"temporal accumulate: ", hint=b"", named=True,
         arrays=lambda s: [(w, (4 if w.endswith("prim") else 16) * px(s), 4 if w.endswith("prim") else 16, "0" if w.endswith("prim") or w.startswith("d_out") else "f") for w in TEMPORAL],
         overlaps=tuple(("d_out_color", w, False) for w in TEMPORAL[:8]) + tuple(("d_out_stat", w, False) for w in TEMPORAL[:9]),
         small=IMAGE, big=BIG_IMAGE, empty=NO_VIEWS, past=("d_prim", "d_out_stat")),
    dict(name="gnxr_luminance_histogram_device", call=call_histogram, prefix=b"luminance histogram: ", hint=b"", named=True,
         arrays=lambda s: [("d_rgba", 16 * px(s), 16, "f"), ("d_hist", 1040 * s["V"], 16, "0")],
         overlaps=(("d_hist", "d_rgba", False),), small=IMAGE, big=dict(W=40, H=32, V=4), empty=NO_VIEWS, past=("d_rgba", "d_hist")),
    dict(name="gnxr_exposure_device", call=call_exposure, prefix=b"exposure: ", hint=b"", named=True,
         arrays=lambda s: [("d_hist", 1040 * s["V"], 16, "0"), ("d_prev_exposure", 16 * s["V"], 16, "f"), ("d_exposure", 16 * s["V"], 16, "0")],
         overlaps=(("d_exposure", "d_hist", False), ("d_exposure", "d_prev_exposure", True)), small=dict(V=2), big=dict(V=257), empty=dict(V=0), past=("d_hist", "d_exposure")),
    dict(name="gnxr_tonemap_device", call=call_tonemap, prefix=b"tonemap: ", hint=b"", named=True,
         arrays=lambda s: [("d_rgba", 16 * px(s), 16, "f"), ("d_exposure", 16 * s["V"], 16, "f"), ("d_rgba8_out", 4 * px(s), 4, "0")],
         overlaps=(("d_rgba8_out", "d_rgba", False), ("d_rgba8_out", "d_exposure", False)), small=IMAGE, big=BIG_IMAGE, empty=NO_VIEWS, past=("d_rgba", "d_rgba8_out")),
    dict(name="gnxr_bake_dilate_device", call=call_dilate, prefix=b"gnxr_bake_dilate_device: ", hint=b"", named=True,
         arrays=lambda s: [("d_rgba", 16 * s["W"] * s["H"], 16, "h")],
         overlaps=(), small=dict(W=8, H=8), big=dict(W=40, H=32), empty=None, past=("d_rgba",)),   # an atlas is at least 1 x 1: no empty call
    dict(name="gnxr_skin_vertices_device", call=call_skin, prefix=b"skin vertices: ", hint=b"", named=True,
         arrays=lambda s: [("d_rest", 12 * s["V"], 4, "f"), ("d_bone_index", 16 * s["V"], 16, "0"), ("d_bone_weight", 16 * s["V"], 16, "f"), ("d_bones", 48 * s["B"], 16, "f"),
                           ("d_morph_delta", 12 * s["M"] * s["V"], 4, "f"), ("d_morph_weight", 4 * s["M"], 4, "f"), ("d_out", 12 * s["V"], 4, "0")],
         overlaps=tuple(("d_out", w, False) for w in ("d_rest", "d_bone_index", "d_bone_weight", "d_bones", "d_morph_delta", "d_morph_weight")),
         small=dict(V=4, B=1, M=1), big=dict(V=512, B=1, M=1), empty=dict(V=0, B=1, M=1), past=("d_rest", "d_out")),
]
every_entry = pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
SLACK = 256   # bytes between two arrays of a layout, and before the first: room to move one without touching its neighbours


def layout(arrays, base):
    """Every array in a slot of its own from a 256-byte aligned base: name -> address, and the bytes the slots take."""
    slot = SLACK + (max(b for _, b, _, _ in arrays) + 255) // 256 * 256
    return {what: base + SLACK + i * slot for i, (what, _, _, _) in enumerate(arrays)}, SLACK + len(arrays) * slot


def host_arrays(arrays):
    """Aligned host memory that passes every argument check (the buffer is returned to keep it alive)."""
    buf = (C.c_char * (layout(arrays, 0)[1] + 256))()
    return layout(arrays, (C.addressof(buf) + 255) & ~255)[0], buf


def check_overlaps(L, A, e, p, s, refusals_only=False):
    """An output moved 16 bytes below an input reaches into it; at the input's own address it does so too, unless that is `in place`."""
    for out, inp, in_place in e["overlaps"]:
        want = e["prefix"] + out.encode() + b" overlaps " + inp.encode()
        assert e["call"](L, A, dict(p, **{out: p[inp] - 16}), s) == ERR_INVALID and want in L.gnxr_last_error(), (out, inp, L.gnxr_last_error())
        if in_place and refusals_only:
            continue
        rc = e["call"](L, A, dict(p, **{out: p[inp]}), s)
        if in_place:
            assert rc != ERR_INVALID or b"overlaps" not in L.gnxr_last_error(), (out, inp, L.gnxr_last_error())
        else:
            assert rc == ERR_INVALID and want in L.gnxr_last_error(), (out, inp, L.gnxr_last_error())


# ---------------------------------------------------------------- CPU
@every_entry
def test_misaligned_array_is_refused_by_name(gx, e):
    L, A = gx.lib(), gx._abi
    arrays = e["arrays"](e["small"])
    p, keep = host_arrays(arrays)
    for what, _, align, _ in arrays:
        for off in sorted({align // 2, align - 4} - {0}):   # floats that sit on a float's boundary, not on the array's
            assert e["call"](L, A, dict(p, **{what: p[what] + off}), e["small"]) == ERR_INVALID, (what, off)
            msg = L.gnxr_last_error()
            if e["named"]:
                assert e["prefix"] + what.encode() + b" is not %d-byte aligned" % align in msg, (what, off, msg)
            else:
                assert msg.startswith(e["prefix"]) and what.encode() in msg and b"-byte aligned" in msg, (what, off, msg)
    del keep


@pytest.mark.parametrize("e", [e for e in ENTRIES if e["overlaps"] and not e.get("after_walk")], ids=lambda e: e["name"])
def test_output_that_overlaps_an_input_is_refused(gx, e):
    p, keep = host_arrays(e["arrays"](e["small"]))
    check_overlaps(gx.lib(), gx._abi, e, p, e["small"])
    del keep


@every_entry
def test_empty_call_returns_before_the_device_and_a_full_one_needs_it(gx, e):
    L, A = gx.lib(), gx._abi
    p, keep = host_arrays(e["arrays"](e["small"]))
    if e["empty"] is not None:
        assert e["call"](L, A, p, e["empty"]) == 0
    if not torch.cuda.is_available():   # arguments that pass every check need the runtime: no CPU fallback
        assert e["call"](L, A, p, e["small"]) == ERR_NO_DEVICE
    del keep


# ---------------------------------------------------------------- GPU
def device_arrays(arrays, device=DEV, fill=False):
    """The layout in one device buffer (returned with the addresses), zeros or the contents the table asks for."""
    buf = torch.zeros(layout(arrays, 0)[1], dtype=torch.uint8, device=device)
    p = layout(arrays, buf.data_ptr())[0]
    assert buf.data_ptr() % 256 == 0
    for what, nbytes, _, contents in arrays if fill else ():
        first = p[what] - buf.data_ptr()
        if contents != "0":
            buf[first:first + (nbytes if contents == "f" else nbytes // 2)].view(torch.float32).uniform_(0.1, 1.0)
    return p, buf


def short_allocation():
    """hipMalloc and hipFree of the runtime this process already runs on."""
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    return hip


@pytest.mark.gpu
@every_entry
def test_device_arrays_pass_and_host_arrays_are_refused_by_name(gpu, e):
    L, A = gpu.lib(), gpu._abi
    s = e["small"]
    arrays = e["arrays"](s)
    torch.manual_seed(7)
    p, buf = device_arrays(arrays, fill=True)
    before = buf.clone()
    assert e["call"](L, A, p, s) == 0, L.gnxr_last_error()
    torch.cuda.synchronize()
    done = buf.clone()
    assert not torch.equal(done, before)   # the call wrote its output
    host = torch.zeros(layout(arrays, 0)[1] // 4)   # host memory where device memory belongs, one array at a time
    assert host.data_ptr() % 16 == 0
    for what, _, _, _ in arrays:
        assert e["call"](L, A, dict(p, **{what: host.data_ptr()}), s) == ERR_INVALID, what
        assert e["prefix"] + what.encode() + b" is not device memory" + e["hint"] in L.gnxr_last_error(), (what, L.gnxr_last_error())
    if e.get("after_walk"):
        check_overlaps(L, A, e, p, s, refusals_only=True)
    if torch.cuda.device_count() > 1 and len(arrays) > 1:   # the last array on another device than the first
        last = arrays[-1][0]
        other = torch.zeros(arrays[-1][1], dtype=torch.uint8, device="cuda:1")
        assert e["call"](L, A, dict(p, **{last: other.data_ptr()}), s) == ERR_INVALID
        assert e["prefix"] + arrays[0][0].encode() + b" and " + last.encode() + b" live on different devices" in L.gnxr_last_error(), L.gnxr_last_error()
        assert int(other.count_nonzero()) == 0
        print("two devices: the refusal ran")
    else:
        print("one device or one array: the refusal for arrays on different devices did not run")
    torch.cuda.synchronize()
    assert torch.equal(buf, done)   # the refused calls queued nothing
    if e.get("after_walk"):
        check_overlaps(L, A, e, p, s)   # once more with the output at an input's own address: where that is in place, the call runs
        torch.cuda.synchronize()


@pytest.mark.gpu
@every_entry
def test_array_past_the_end_of_its_allocation_is_refused_by_name(gpu, e):
    L, A = gpu.lib(), gpu._abi
    s = e["big"]
    arrays = e["arrays"](s)
    p, buf = device_arrays(arrays)
    hip, small = short_allocation(), C.c_void_p()
    assert hip.hipMalloc(C.byref(small), 4096) == 0
    try:
        for what in e["past"]:
            assert dict((w, b) for w, b, _, _ in arrays)[what] > 4096
            assert e["call"](L, A, dict(p, **{what: small.value}), s) == ERR_INVALID, what
            msg = L.gnxr_last_error()
            assert msg.startswith(e["prefix"] + what.encode() + b": ") and b"past the end of its allocation" in msg, (what, msg)
    finally:
        assert hip.hipFree(small) == 0
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0   # nothing was queued
