"""What the Python layer refuses before it reaches the library, message by message: one table row per entry point that takes a tensor or
an array -- how to call it on correct arguments at the smallest shapes, its array arguments with dtype, shape and the words its refusal
starts with, its result tensors, and the refusals of its other arguments -- and the same mutations for every row.  A message is compared
whole: the row's words, then what the mutation handed in (type, dtype, shape, device), spelled out here from what the test built.

Part A needs no GPU: on CPU tensors every mutation of a call's first array is refused before the library or torch.cuda is reached, and
so are the layout mutations of the later arrays of the calls that check layouts first, the host-memory side of the scene-editing methods
and every refusal of a plain argument that comes before the first device check.  Part B runs the rest on cuda:0: the later arrays, the
result tensors and the plain arguments that are checked after the arrays.  Scene methods run on a stub (no handle: no refusal reads it)."""
import numpy as np
import pytest
import torch

import gnxraytracer_amd as gx

A = gx._abi
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
OTHER = {F32: torch.float64, I32: torch.int64, U8: torch.int32}
LAYOUT = ("list", "dtype", "trailing", "extra", "strided")
GPU = "cuda:0"
IMG = "must be a contiguous float32 (H, W, 4) or (V, H, W, 4) tensor on a GPU, got "


def stub_scene():
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_triangles, s.n_vertices, s.n_lights = None, 0, 3, 3, 1
    s._env_light, s._textures = None, [gx.Texture()]
    return s


def cam():
    return gx.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0)


def grid_medium():
    m = gx.Medium()
    m.type, m.nx, m.ny, m.nz = A.MEDIUM_GRID, 2, 2, 2
    return m


def box():
    return gx.film_filter("box", 0.5)


def got(kind, dtype, shape, device, tn=True, dev=True):
    """the tail of a refusal, from what the test knows it handed in"""
    return f"{kind + ' ' if tn else ''}{dtype} {tuple(shape)}{' on %s' % device if dev else ''}"


def arr(arg, dtype, shape, head, **k):
    """An array argument: `head` is its refusal up to "got "; layout=: the words of a layout check that runs before every device check
    (its tail has no device); rows=: the whole message for one row too many, None where no count is compared; list= / extra= / ...: the
    whole message of that mutation where it differs; tn / dev: whether the tail names the type and the device; put: how to set it."""
    k = {("on_" + key if key in LAYOUT + ("rows",) else key): v for key, v in k.items()}
    return dict(dict(arg=arg, dtype=dtype, shape=tuple(shape), head=head, layout=None, on_rows=None, tn=True, dev=True, put=None, skip=()), **k)


def mutate(a, m, device):
    """(value, kind, dtype, shape, device) of mutation m of array a, None where it does not apply"""
    d, s = a["dtype"], a["shape"]
    if m == "list":
        return [0], "list", None, (), None
    if m == "dtype":
        return torch.zeros(s, dtype=OTHER[d], device=device), "Tensor", OTHER[d], s, device
    if m == "trailing":
        if len(s) < 2:
            return None
        s = s[:-1] + (s[-1] + 1,)
    elif m == "extra":
        s = s + (1,)
    elif m == "rows":
        s = (s[0] + 1,) + s[1:]
    elif m == "strided":
        return torch.zeros(s[:-1] + (2 * s[-1],), dtype=d, device=device)[..., ::2], "Tensor", d, s, device
    elif m == "cpu":
        device = "cpu"
    return torch.zeros(s, dtype=d, device=device), "Tensor", d, s, device


def expected(a, m, facts):
    if a.get("on_" + m) is not None:
        return a["on_" + m]
    if a["layout"] and m in LAYOUT:
        return a["layout"] + got(*facts, tn=a["tn"], dev=False)
    return a["head"] + got(*facts, tn=a["tn"], dev=a["dev"])


def good(row, device):
    args = dict(row["args"]())
    for a in row["arrays"]:
        if a["put"] is None:
            args[a["arg"]] = torch.zeros(a["shape"], dtype=a["dtype"], device=device)
    for a in row["arrays"]:
        if a["put"] is not None:
            a["put"](args, torch.zeros(a["shape"], dtype=a["dtype"], device=device))
    return args


def refused(row, args, exc, message):
    with pytest.raises(exc) as e:
        row["call"](stub_scene(), **args)
    assert type(e.value) is exc and str(e.value) == message, str(e.value)


def run_array(row, k, m, device):
    a = row["arrays"][k]
    mut = mutate(a, m, device)
    if mut is None or m in a["skip"] or (m == "rows" and a["on_rows"] is None):
        return 0
    args = good(row, device)
    if a["put"] is None:
        args[a["arg"]] = mut[0]
    else:
        a["put"](args, mut[0])
    refused(row, args, ValueError, expected(a, m, mut[1:]))
    return 1


def out_(arg, dtype, shape, head, put=None):
    return arr(arg, dtype, shape, head, put=put)


def into(key, index, size=0):
    """sets entry `index` of the dict or of the tuple of `size` entries that is argument `key`"""
    def put(args, t):
        if isinstance(index, str):
            args[key] = dict(args.get(key) or {}, **{index: t})
        else:
            cur = list(args.get(key) or (None,) * size)
            args[key] = tuple(cur[:index] + [t] + cur[index + 1:])
    return put


def O(what, dtype, shape, device=GPU):
    return f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "


def D(what, dtype, tail, where=GPU):
    return f"{what}: expected a contiguous {dtype} ({tail}) tensor on {where}, got "


def Lq(what, dtype, cols):
    return f"{what}: expected a contiguous {dtype} (n, {cols}) tensor, got "


PI = gx.PathIntegrator(2)
VIEW = dict(width=2, height=2)
# cpu: (changed arguments, exception, message) refused before the first device check, on correct CPU arrays; gpu: the same after it.
ROWS = [
    dict(name="Scene.intersect", call=lambda sc, **a: sc.intersect(**a), args=dict,
         arrays=[arr("rays", F32, (3, 8), D("intersect: rays", F32, "n, 8"))], outs=[out_("out", F32, (3, 8), O("intersect: out", F32, (3, 8)))]),
    dict(name="Scene.occluded", call=lambda sc, **a: sc.occluded(**a), args=dict,
         arrays=[arr("rays", F32, (3, 8), D("occluded: rays", F32, "n, 8"))], outs=[out_("out", U8, (3,), O("occluded: out", U8, (3,)))]),
    dict(name="Scene.bsdf", call=lambda sc, **a: sc.bsdf(**a), args=dict,
         arrays=[arr("rays", F32, (3, 8), D("bsdf: rays", F32, "n, 8"), layout=Lq("bsdf: rays", F32, 8)),
                 arr("wi", F32, (3, 3), D("bsdf: wi", F32, "n, 3"), layout=Lq("bsdf: wi", F32, 3), rows="bsdf: wi has 4 rows for 3 rays"),
                 arr("u", F32, (3, 2), D("bsdf: u", F32, "n, 2"), layout=Lq("bsdf: u", F32, 2), rows="bsdf: u has 4 rows for 3 rays"),
                 arr("differentials", F32, (3, 12), D("bsdf: differentials", F32, "n, 12"), layout=Lq("bsdf: differentials", F32, 12),
                     rows="bsdf: differentials has 4 rows for 3 rays")],
         outs=[out_("out", F32, (3, 16), O("bsdf: out", F32, (3, 16)))],
         cpu=[(dict(flags=32), ValueError, "bsdf: flags must be a BxDFType mask in [0, 31], got 32")]),
    dict(name="Scene.sample_light", call=lambda sc, **a: sc.sample_light(**a), args=lambda: dict(light=0),
         arrays=[arr("p", F32, (3, 3), D("sample_light: p", F32, "n, 3"), layout=Lq("sample_light: p", F32, 3)),
                 arr("n", F32, (3, 3), D("sample_light: n", F32, "n, 3"), layout=Lq("sample_light: n", F32, 3), rows="sample_light: n has 4 rows for 3 p"),
                 arr("u", F32, (3, 2), D("sample_light: u", F32, "n, 2"), layout=Lq("sample_light: u", F32, 2), rows="sample_light: u has 4 rows for 3 p"),
                 arr("wi_query", F32, (3, 3), D("sample_light: wi_query", F32, "n, 3"), layout=Lq("sample_light: wi_query", F32, 3),
                     rows="sample_light: wi_query has 4 rows for 3 p"),
                 # (the index tensor is compared whole and may be strided: that mutation is not a refusal)
                 arr("light", I32, (3,), "sample_light: light must be an int or an int32 (3,) tensor on cuda:0, got ", tn=False, skip=("strided",),
                     list="sample_light: light must be an int or an int32 tensor, got list",
                     rows="sample_light: light must be an int or an int32 (3,) tensor on cuda:0, got torch.int32 (4,) on cuda:0")],
         outs=[out_("out", F32, (3, 12), O("sample_light: out", F32, (3, 12)))], first_only=4,
         cpu=[(dict(strategy="bogus"), ValueError, "sample_light: strategy must be one of ['power', 'spatial', 'uniform'] or LIGHTS_SPATIAL / LIGHTS_UNIFORM / LIGHTS_POWER, got 'bogus'"),
              (dict(strategy=True), ValueError, "sample_light: strategy must be one of ['power', 'spatial', 'uniform'] or LIGHTS_SPATIAL / LIGHTS_UNIFORM / LIGHTS_POWER, got True")],
         gpu=[(dict(light=1.5), ValueError, "sample_light: light must be an int or an int32 tensor, got float"),
              (dict(light=True), ValueError, "sample_light: light must be an int or an int32 tensor, got bool")]),
    dict(name="Scene.light_le", call=lambda sc, **a: sc.light_le(**a), args=lambda: dict(light=0),
         arrays=[arr("rays", F32, (3, 8), D("light_le: rays", F32, "n, 8"), layout=Lq("light_le: rays", F32, 8))],
         outs=[out_("out", F32, (3, 3), O("light_le: out", F32, (3, 3)))]),
    dict(name="Scene.motion", call=lambda sc, **a: sc.motion(**a), args=lambda: dict(VIEW, prev_cameras=cam()),
         arrays=[arr("prev_vertices", F32, (3, 3), D("motion: prev_vertices", F32, "n, 3"), rows="motion: prev_vertices has 4 rows, the scene has 3 vertices", first_rows=True)],
         outs=[out_("motion", F32, (2, 2, 4), O("motion: out['motion']", F32, (2, 2, 4)), into("out", "motion")),
               out_("guide", F32, (2, 2, 4), O("motion: out['guide']", F32, (2, 2, 4)), into("out", "guide")),
               out_("prim", I32, (2, 2), O("motion: out['prim']", I32, (2, 2)), into("out", "prim"))],
         cpu=[(dict(width=0), ValueError, "motion: prev_cameras: invalid image size 0 x 2"), (dict(height=-1), ValueError, "motion: prev_cameras: invalid image size 2 x -1"),
              (dict(prev_cameras=None), ValueError, "motion: prev_cameras is required (the cameras of the previous frame)"),
              (dict(prev_cameras=[1]), ValueError, "motion: prev_cameras: cameras must be gnxr Camera records (camera(...)), got int"),
              (dict(cameras=[1]), ValueError, "motion: cameras must be gnxr Camera records (camera(...)), got int"),
              (dict(prev_cameras=[cam(), cam()]), ValueError, "motion: 2 previous cameras for 1 view"),
              (dict(prev_cameras=[cam()], cameras=[cam(), cam()]), ValueError, "motion: 1 previous cameras for 2 views")],
         gpu=[(dict(out={"depth": None}), ValueError, "motion: out holds ['depth']; the channels are ('motion', 'guide', 'prim')")]),
    dict(name="PathIntegrator.Li", call=lambda sc, **a: PI.Li(sc, **a), args=lambda: dict(VIEW, spp=1),
         arrays=[arr("rays", F32, (3, 8), D("Li: rays", F32, "n, 8"), layout=Lq("Li: rays", F32, 8)),
                 arr("samples", I32, (3, 4), D("Li: samples", I32, "n, 4"), layout=Lq("Li: samples", I32, 4), rows="Li: 4 sample records for 3 rays")],
         outs=[out_("out", F32, (3, 4), O("Li: out", F32, (3, 4)))], cpu_outs=True),
    dict(name="PathIntegrator.RenderViews", call=lambda sc, **a: PI.RenderViews(sc, **a), args=lambda: dict(VIEW, cameras=[cam()], spp=1), arrays=[],
         outs=[out_("out", F32, (1, 2, 2, 4), O("RenderViews: out", F32, (1, 2, 2, 4)))], cpu_outs=True,
         cpu=[(dict(width=0), ValueError, "RenderViews: invalid image size 0 x 2"), (dict(height=0), ValueError, "RenderViews: invalid image size 2 x 0"),
              (dict(cameras=[1]), ValueError, "RenderViews: cameras must be gnxr Camera records (camera(...)), got int"),
              (dict(media=[0, 0]), ValueError, "RenderViews: 2 media for 1 cameras")]),
    dict(name="PathIntegrator.RenderAdaptive", call=lambda sc, **a: PI.RenderAdaptive(sc, **a), args=lambda: dict(VIEW, spp=2, threshold=0.1, min_spp=1), arrays=[],
         outs=[out_("out", F32, (2, 2, 4), O("RenderAdaptive: out", F32, (2, 2, 4))), out_("count_out", I32, (2, 2), O("RenderAdaptive: count_out", I32, (2, 2)))],
         cpu=[(dict(width=0), ValueError, "RenderAdaptive: invalid image size 0 x 2"),
              (dict(min_spp=3), ValueError, "RenderAdaptive: spp >= 1 and min_spp in [1, spp] are required, got spp = 2, min_spp = 3"),
              (dict(step_spp=0), ValueError, "RenderAdaptive: step_spp must be at least 1, got 0"), (dict(guard=9), ValueError, "RenderAdaptive: guard must lie in [0, 8], got 9"),
              (dict(threshold=-1), ValueError, "RenderAdaptive: threshold and floor must be numbers >= 0, got -1.0 and 0.01"),
              (dict(bogus=1), ValueError, "RenderAdaptive: unexpected arguments ['bogus'] (samples_per_pass, passes_in_flight)")]),
    dict(name="PathIntegrator.RenderAOV", call=lambda sc, **a: PI.RenderAOV(sc, **a), args=lambda: dict(VIEW, spp=1), arrays=[],
         outs=[out_("albedo", F32, (2, 2, 4), O("RenderAOV: out['albedo']", F32, (2, 2, 4)), into("out", "albedo")),
               out_("depth", F32, (2, 2), O("RenderAOV: out['depth']", F32, (2, 2)), into("out", "depth")),
               out_("ids", I32, (2, 2, 2), O("RenderAOV: out['ids']", I32, (2, 2, 2)), into("out", "ids"))],
         cpu=[(dict(channels=("bogus",)), ValueError, "RenderAOV: channels must be a non-empty selection of ('albedo', 'normal', 'shading_normal', 'depth', 'ids'), got ('bogus',)"),
              (dict(media=[0]), ValueError, "RenderAOV: media goes with cameras; the scene's own camera sits in the scene's camera medium"),
              (dict(width=0), ValueError, "RenderAOV: invalid image size 0 x 2"),
              (dict(bogus=1), ValueError, "RenderAOV: unexpected arguments ['bogus'] (spp_begin, spp_end, samples_per_pass)"),
              (dict(channels=("depth",), out={"ids": None}), ValueError, "RenderAOV: out holds ['ids'], which channels does not name")]),
    dict(name="PathIntegrator.RenderDenoised", call=lambda sc, **a: PI.RenderDenoised(sc, **a), args=lambda: dict(VIEW, spp=2), arrays=[], outs=[],
         cpu=[(dict(spp=3), ValueError, "RenderDenoised: spp must be even and at least 2 (the two halves are the variance estimate), got 3"),
              (dict(normal="x"), ValueError, "RenderDenoised: normal must be 'shading_normal' or 'normal', got 'x'"),
              (dict(media=[0]), ValueError, "RenderDenoised: media goes with cameras; the scene's own camera sits in the scene's camera medium"),
              (dict(bogus=1), ValueError, "RenderDenoised: unexpected arguments ['bogus'] (iterations, sigma_color, sigma_normal, sigma_depth, out)"),
              (dict(width=0), ValueError, "RenderDenoised: invalid image size 0 x 2")]),
    dict(name="PathIntegrator.RenderFiltered", call=lambda sc, **a: PI.RenderFiltered(sc, **a), args=lambda: dict(VIEW, spp=1, filter=box()), arrays=[],
         outs=[out_("accum", F32, (2, 2, 4), O("RenderFiltered: accum", F32, (2, 2, 4))), out_("out", F32, (2, 2, 4), O("RenderFiltered: out", F32, (2, 2, 4)))],
         cpu=[(dict(filter=1), ValueError, "RenderFiltered: filter must be a film_filter(...) record, got int"),
              (dict(media=[0]), ValueError, "RenderFiltered: media goes with cameras; the scene's own camera sits in the scene's camera medium"),
              (dict(width=0), ValueError, "RenderFiltered: invalid image size 0 x 2"),
              (dict(resume=True), ValueError, "RenderFiltered: resume continues an accumulator: pass the tensor of the earlier call as accum"),
              (dict(bogus=1), ValueError, "RenderFiltered: unexpected arguments ['bogus'] (spp_begin, spp_end, samples_per_pass, passes_in_flight)")]),
    dict(name="PathIntegrator.BakeLightmap", call=lambda sc, **a: PI.BakeLightmap(sc, **a), args=lambda: dict(VIEW, spp=1),
         arrays=[arr("lm_uv", F32, (3, 6), D("BakeLightmap: lm_uv", F32, "n, 6"), rows="BakeLightmap: lm_uv has 4 rows for 3 triangles", first_rows=True)],
         outs=[out_("out", F32, (2, 2, 4), O("BakeLightmap: out", F32, (2, 2, 4)))],
         cpu=[(dict(width=0), ValueError, "BakeLightmap: invalid atlas size 0 x 2"), (dict(dilate=-1), ValueError, "BakeLightmap: dilate must be >= 0, got -1"),
              (dict(bogus=1), ValueError, "BakeLightmap: unexpected arguments ['bogus'] (samples_per_pass, passes_in_flight)")]),
    dict(name="PathIntegrator.BakeLightProbes", call=lambda sc, **a: PI.BakeLightProbes(sc, **a), args=lambda: dict(spp=1),
         arrays=[arr("positions", F32, (3, 3), D("BakeLightProbes: positions", F32, "n, 3"))],
         outs=[out_("out", F32, (3, 9, 4), O("BakeLightProbes: out", F32, (3, 9, 4)))],
         gpu=[(dict(width=1, height=1), ValueError, "BakeLightProbes: the 1 x 1 grid of pixels does not hold 3 probes"),
              (dict(width=0), ValueError, "BakeLightProbes: the 0 x 0 grid of pixels does not hold 3 probes"),
              (dict(bogus=1), ValueError, "BakeLightProbes: unexpected arguments ['bogus'] (samples_per_pass, passes_in_flight)")]),
    dict(name="camera_rays_device", call=lambda sc, **a: gx.camera_rays_device(**a), args=lambda: dict(VIEW, camera=cam()),
         arrays=[arr(w, I32, (3,), f"camera_rays_device: {w} must be a contiguous int32 (n,) tensor on one GPU, got ",
                     rows=None if w == "px" else f"camera_rays_device: {w} has 4 entries for 3 px") for w in ("px", "py", "s")],
         outs=[], gpu=[(dict(camera=1), ValueError, "camera_rays_device: camera must be a gnxr Camera record (camera(...)), got int")]),
    dict(name="denoise", call=lambda sc, **a: gx.denoise(**a), args=dict,
         arrays=[arr("color", F32, (2, 2, 4), "denoise: color " + IMG)] +
                [arr(w, F32, (2, 2, 4), O("denoise: " + w, "float32", (2, 2, 4)), rows=O("denoise: " + w, "float32", (2, 2, 4)) + "Tensor torch.float32 (3, 2, 4) on cuda:0")
                 for w in ("color_b", "albedo", "normal")] +
                [arr("depth", F32, (2, 2), O("denoise: depth", "float32", (2, 2)), rows=O("denoise: depth", "float32", (2, 2)) + "Tensor torch.float32 (3, 2) on cuda:0")],
         outs=[out_("out", F32, (2, 2, 4), O("denoise: out", F32, (2, 2, 4)))],
         gpu=[(dict(color=(0, 2, 4), color_b=(0, 2, 4), albedo=(0, 2, 4), normal=(0, 2, 4), depth=(0, 2)), ValueError, "denoise: invalid image size 2 x 0"), (dict(iterations=0), ValueError, "denoise: iterations must lie in [1, 8], got 0"),
              (dict(sigma_color=-1), ValueError, "denoise: the sigmas must be numbers >= 0, got [-1.0, 0.25, 0.01]")]),
    dict(name="film_add", call=lambda sc, **a: gx.film_add(**a), args=lambda: dict(f=box()),
         arrays=[arr("accum", F32, (2, 2, 4), "film_add: accum " + IMG),
                 arr("L", F32, (3, 2, 2, 4), O("film_add: L", "float32", ()).replace("()", "(n, 2, 2, 4)"),
                     rows=O("film_add: offsets", "float32", (4, 2, 2, 2)) + "Tensor torch.float32 (3, 2, 2, 2) on cuda:0"),
                 arr("offsets", F32, (3, 2, 2, 2), O("film_add: offsets", "float32", (3, 2, 2, 2)),
                     rows=O("film_add: offsets", "float32", (3, 2, 2, 2)) + "Tensor torch.float32 (4, 2, 2, 2) on cuda:0")],
         outs=[], cpu=[(dict(f=1), ValueError, "film_add: expected a film_filter(...) record, got int")],
         gpu=[(dict(accum=(0, 2, 4), L=(3, 0, 2, 4), offsets=(3, 0, 2, 2)), ValueError, "film_add: invalid image size 2 x 0")]),
    dict(name="film_resolve", call=lambda sc, **a: gx.film_resolve(**a), args=dict, arrays=[arr("accum", F32, (2, 2, 4), "film_resolve: accum " + IMG)],
         outs=[out_("out", F32, (2, 2, 4), O("film_resolve: out", F32, (2, 2, 4)))], gpu=[(dict(accum=(2, 0, 4)), ValueError, "film_resolve: invalid image size 0 x 2")]),
    dict(name="bake_texels", call=lambda sc, **a: gx.bake_texels(sc, **a), args=lambda: dict(VIEW),
         arrays=[arr("lm_uv", F32, (3, 6), D("bake_texels: lm_uv", F32, "n, 6"), rows="bake_texels: lm_uv has 4 rows for 3 triangles", first_rows=True)],
         outs=[out_("tri", I32, (2, 2), O("bake_texels: out[0]", I32, (2, 2)), into("out", 0, 2)), out_("bary", F32, (2, 2, 2), O("bake_texels: out[1]", F32, (2, 2, 2)), into("out", 1, 2))],
         cpu=[(dict(height=0), ValueError, "bake_texels: invalid atlas size 2 x 0")]),
    dict(name="surface_rays", call=lambda sc, **a: gx.surface_rays(sc, **a), args=lambda: dict(VIEW),
         arrays=[arr("tri", I32, (3,), D("surface_rays: tri", I32, "n")), arr("bary", F32, (3, 2), D("surface_rays: bary", F32, "n, 2"), rows="surface_rays: bary has 4 rows for 3 triangles")] +
                [arr(w, I32, (3,), D("surface_rays: " + w, I32, "n"), rows=f"surface_rays: {w} has 4 entries for 3 triangles") for w in ("px", "py", "s")],
         outs=[out_("rays", F32, (3, 8), O("surface_rays: out[0]", F32, (3, 8)), into("out", 0, 3)), out_("samples", I32, (3, 4), O("surface_rays: out[1]", I32, (3, 4)), into("out", 1, 3)),
               out_("pn", F32, (3, 8), O("surface_rays: out[2]", F32, (3, 8)), into("out", 2, 3))]),
    dict(name="bake_dilate", call=lambda sc, **a: gx.bake_dilate(**a), args=lambda: dict(iterations=1),
         arrays=[arr("img", F32, (2, 2, 4), "bake_dilate: img must be a contiguous float32 (H, W, 4) tensor on a GPU, got ")],
         outs=[out_("out", F32, (2, 2, 4), O("bake_dilate: out", F32, (2, 2, 4)))],
         gpu=[(dict(img=(0, 2, 4)), ValueError, "bake_dilate: invalid image size 2 x 0"), (dict(iterations=-1), ValueError, "bake_dilate: iterations must be >= 0, got -1")]),
    dict(name="lightprobe_rays", call=lambda sc, **a: gx.lightprobe_rays(sc, **a), args=lambda: dict(VIEW),
         arrays=[arr("pos", F32, (3, 3), D("lightprobe_rays: pos", F32, "n, 3"))] +
                [arr(w, I32, (3,), D("lightprobe_rays: " + w, I32, "n"), rows=f"lightprobe_rays: {w} has 4 entries for 3 positions") for w in ("px", "py", "s")],
         outs=[out_("rays", F32, (3, 8), O("lightprobe_rays: out[0]", F32, (3, 8)), into("out", 0, 2)), out_("samples", I32, (3, 4), O("lightprobe_rays: out[1]", I32, (3, 4)), into("out", 1, 2))],
         gpu=[(dict(width=0), ValueError, "lightprobe_rays: invalid image size 0 x 2")]),
    dict(name="sh_project", call=lambda sc, **a: gx.sh_project(**a), args=lambda: dict(n_probes=1),
         arrays=[arr("rays", F32, (3, 8), D("sh_project: rays", F32, "n, 8", "a GPU")), arr("L", F32, (3, 4), D("sh_project: L", F32, "n, 4"), rows="sh_project: L has 4 rows for 3 rays")],
         outs=[out_("out", F32, (1, 9, 4), O("sh_project: out", F32, (1, 9, 4)))],
         gpu=[(dict(n_probes=2), ValueError, "sh_project: 3 records are no whole number of samples for each of 2 probes"),
              (dict(n_probes=-1), ValueError, "sh_project: 3 records are no whole number of samples for each of -1 probes"),
              (dict(accumulate=True), ValueError, "sh_project: accumulate continues the sums of an earlier call: pass its tensor as out")]),
    dict(name="sh_irradiance", call=lambda sc, **a: gx.sh_irradiance(**a), args=dict,
         arrays=[arr("sh", F32, (1, 9, 4), D("sh_irradiance: sh", F32, "n, 9, 4", "a GPU")),
                 arr("probe", I32, (3,), D("sh_irradiance: probe", I32, "n"), rows="sh_irradiance: normals has 3 rows for 4 probe indices"),
                 arr("normals", F32, (3, 3), D("sh_irradiance: normals", F32, "n, 3"), rows="sh_irradiance: normals has 4 rows for 3 probe indices")],
         outs=[out_("out", F32, (3, 4), O("sh_irradiance: out", F32, (3, 4)))]),
    dict(name="temporal_accumulate", call=lambda sc, **a: gx.temporal_accumulate(**a), args=dict,
         arrays=[arr("color", F32, (2, 2, 4), "temporal_accumulate: color " + IMG)] +
                [arr(w, F32, (2, 2, 4), O("temporal_accumulate: " + w, F32, (2, 2, 4)), rows=O("temporal_accumulate: " + w, F32, (2, 2, 4)) + "Tensor torch.float32 (3, 2, 4) on cuda:0")
                 for w in ("motion", "guide")] +
                [arr("prim", I32, (2, 2), O("temporal_accumulate: prim", I32, (2, 2)), rows=O("temporal_accumulate: prim", I32, (2, 2)) + "Tensor torch.int32 (3, 2) on cuda:0")],
         outs=[out_("color", F32, (2, 2, 4), O("temporal_accumulate: out['color']", F32, (2, 2, 4)), into("out", "color")),
               out_("stat", F32, (2, 2, 4), O("temporal_accumulate: out['stat']", F32, (2, 2, 4)), into("out", "stat")),
               out_("history.stat", F32, (2, 2, 4), O("temporal_accumulate: history['stat']", F32, (2, 2, 4)),
                    lambda args, t: args.update(history={"color": torch.zeros((2, 2, 4), device=GPU), "stat": t, "guide": args["guide"], "prim": args["prim"]}))],
         gpu=[(dict(history={"color": None}), ValueError, "temporal_accumulate: history must be None or a dict with 'color', 'stat', 'guide' and 'prim' (what an earlier call returned)"),
              (dict(color=(0, 2, 4), motion=(0, 2, 4), guide=(0, 2, 4), prim=(0, 2)), ValueError, "temporal_accumulate: invalid image size 2 x 0"),
              (dict(max_history=0), ValueError, "temporal_accumulate: max_history must be at least 1, got 0"),
              (dict(depth_tol=-1), ValueError, "temporal_accumulate: depth_tol must be a number >= 0 and normal_cos a number, got -1.0 and 0.9"),
              (dict(out={"guide": None}), ValueError, "temporal_accumulate: out holds ['guide']; the outputs are 'color' and 'stat'")]),
    dict(name="skin_vertices", call=lambda sc, **a: gx.skin_vertices(**a), args=dict,
         arrays=[arr("rest", F32, (3, 3), D("skin_vertices: rest", F32, "n, 3", "a GPU")),
                 arr("bone_index", I32, (3, 4), D("skin_vertices: bone_index", I32, "n, 4"), rows="skin_vertices: 3 rest positions, 4 index rows, 3 weight rows"),
                 arr("bone_weight", F32, (3, 4), D("skin_vertices: bone_weight", F32, "n, 4"), rows="skin_vertices: 3 rest positions, 3 index rows, 4 weight rows"),
                 arr("bones", F32, (1, 12), D("skin_vertices: bones", F32, "n, 12"), extra=D("skin_vertices: bones", F32, "n, 3, 4") + "Tensor torch.float32 (1, 12, 1) on cuda:0"),
                 arr("morph_delta", F32, (2, 3, 3), D("skin_vertices: morph_delta", F32, "n, 3, 3"), rows="skin_vertices: 3 morph targets, 2 weights"),
                 arr("morph_weight", F32, (2,), D("skin_vertices: morph_weight", F32, "n"), rows="skin_vertices: 2 morph targets, 3 weights")],
         outs=[out_("out", F32, (3, 3), O("skin_vertices: out", F32, (3, 3)))],
         gpu=[(dict(bones=(0, 12)), ValueError, "skin_vertices: at least one bone is required"),
              (dict(morph_weight=None), ValueError, "skin_vertices: morph_delta and morph_weight come together or not at all")]),
    dict(name="luminance_histogram", call=lambda sc, **a: gx.luminance_histogram(**a), args=dict, arrays=[arr("color", F32, (2, 2, 4), "luminance_histogram: color " + IMG)],
         outs=[out_("out", I32, (1, 260), O("luminance_histogram: out", I32, (1, 260)))],
         gpu=[(dict(color=(2, 0, 4)), ValueError, "luminance_histogram: invalid image size 0 x 2"), (dict(min_log2=200), ValueError, "luminance_histogram: min_log2 must lie in [-126, 111], got 200")]),
    dict(name="auto_exposure", call=lambda sc, **a: gx.auto_exposure(**a), args=dict,
         arrays=[arr("hist", I32, (1, 260), "auto_exposure: hist must be a contiguous int32 (V, 260) tensor on a GPU (luminance_histogram), got "),
                 arr("prev", F32, (1, 4), "auto_exposure: prev must be None or a contiguous float32 (1, 4) tensor on cuda:0, got ",
                     rows="auto_exposure: prev must be None or a contiguous float32 (1, 4) tensor on cuda:0, got Tensor torch.float32 (2, 4) on cuda:0")],
         outs=[out_("out", F32, (1, 4), O("auto_exposure: out", F32, (1, 4)))],
         gpu=[(dict(min_log2=-200), ValueError, "auto_exposure: min_log2 must lie in [-126, 111], got -200"),
              (dict(key=float("inf")), ValueError, "auto_exposure: key, low, high, rate, min_exposure and max_exposure must be finite"),
              (dict(low=0.9, high=0.5), ValueError, "auto_exposure: 0 <= low < high <= 1 is required, got 0.9 and 0.5"),
              (dict(rate=0), ValueError, "auto_exposure: key > 0, 0 < rate <= 1 and 0 < min_exposure <= max_exposure are required, got 0.18, 0.0, 0.00390625 and 256.0")]),
    dict(name="tonemap", call=lambda sc, **a: gx.tonemap(**a), args=dict,
         arrays=[arr("color", F32, (2, 2, 4), "tonemap: color " + IMG),
                 arr("exposure", F32, (1, 4), "tonemap: an exposure tensor must be a contiguous float32 (1, 4) tensor on cuda:0 (auto_exposure), got ", tn=False,
                     list="tonemap: exposure must be a number or the tensor of auto_exposure, got list",
                     rows="tonemap: an exposure tensor must be a contiguous float32 (1, 4) tensor on cuda:0 (auto_exposure), got torch.float32 (2, 4) on cuda:0")],
         outs=[out_("out", U8, (2, 2, 4), O("tonemap: out", U8, (2, 2, 4)))],
         gpu=[(dict(curve="x"), ValueError, "tonemap: curve must be one of ['aces', 'linear', 'reference', 'reinhard'], got 'x'"),
              (dict(white=0), ValueError, "tonemap: white must lie in [1e-3, 65504], got 0.0"), (dict(exposure=-1), ValueError, "tonemap: exposure must be finite and >= 0, got -1.0"),
              (dict(exposure="x"), ValueError, "tonemap: exposure must be a number or the tensor of auto_exposure, got str")]),
    dict(name="Display.present", call=lambda sc, **a: gx.Display(2, 2).present(**a), args=dict, arrays=[arr("color", F32, (2, 2, 4), "Display.present: color " + IMG)], outs=[],
         gpu=[(dict(color=(3, 2, 4)), ValueError, "Display.present: color is 1 x 3 x 2, the display 1 x 2 x 2")]),
]
for _r in ROWS:
    _r.setdefault("cpu", []); _r.setdefault("gpu", [])
by_name = dict(ids=lambda r: r["name"])


def run_plain(row, device, cases):
    for change, exc, message in cases:
        args = good(row, device)
        args.update({k: torch.zeros(v, dtype=args[k].dtype, device=device) if isinstance(v, tuple) and isinstance(args.get(k), torch.Tensor) else v for k, v in change.items()})
        refused(row, args, exc, message)


# ---------------------------------------------------------------- Part A: no GPU
@pytest.mark.parametrize("row", [r for r in ROWS if r["arrays"]], **by_name)
def test_first_array_and_layouts_are_refused_on_the_cpu(row):
    """On CPU tensors: every mutation of the first array, the layout mutations of the arrays whose layout is checked before any device,
    and the correct CPU tensor where a GPU is required."""
    first = row["arrays"][0]
    n = sum(run_array(row, 0, m, "cpu") for m in LAYOUT)
    if first["layout"]:
        n += sum(run_array(row, k, m, "cpu") for k in range(1, row.get("first_only", len(row["arrays"]))) if row["arrays"][k]["layout"] for m in LAYOUT)
    refused(row, good(row, "cpu"), ValueError, first["head"] + got("Tensor", first["dtype"], first["shape"], "cpu", tn=first["tn"], dev=first["dev"]))
    print(f"{row['name']}: {n + 1} refusals")


@pytest.mark.parametrize("row", [r for r in ROWS if r["cpu"] or r.get("cpu_outs")], **by_name)
def test_plain_arguments_are_refused_on_the_cpu(row):
    run_plain(row, "cpu", row["cpu"])
    for o in row["outs"] if row.get("cpu_outs") else ():   # a result tensor that is checked before the device of the inputs
        where = "cpu" if row["arrays"] else GPU
        for m in ("dtype", "trailing", "extra", "strided"):
            value, *facts = mutate(o, m, "cpu")
            refused(row, dict(good(row, "cpu"), out=value), ValueError, o["head"].replace(GPU, where) + got(*facts))


# ---------------------------------------------------------------- Part A: the scene-editing methods, host memory and what comes before the device
f4 = lambda *s: np.zeros(s, np.float32)
f8 = lambda *s: np.zeros(s, np.float64)
i4 = lambda *s: np.zeros(s, np.int32)
HOST = " in host memory (all arrays numpy, or all tensors on the scene's device), got "
THERE = " on cuda:0 (all arrays tensors there, or all numpy), got "
GEO = lambda **k: dict(dict(vertices=f4(3, 3), indices=i4(3, 3), tri_material=0), **k)
EDITS = [   # (method, arguments, exception, message)
    ("update_vertices", dict(xyz=f8(3, 3)), ValueError, "update_vertices: expected a float32 array of shape (n, 3), got float64 (3, 3)"),
    ("update_vertices", dict(xyz=f4(3, 4)), ValueError, "update_vertices: expected a float32 array of shape (n, 3), got float32 (3, 4)"),
    ("update_vertices", dict(xyz=f4(3, 3, 1)), ValueError, "update_vertices: expected a float32 array of shape (n, 3), got float32 (3, 3, 1)"),
    ("update_vertices", dict(xyz=[0]), ValueError, "update_vertices: expected a numpy array or a torch tensor, got list"),
    ("update_vertices", dict(xyz=f4(3, 3), stream="x"), TypeError, "update_vertices: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("update_vertices", dict(xyz=f4(3, 3), stream=-1), ValueError, "update_vertices: a hipStream_t is not negative, got -1"),
    ("set_triangle_materials", dict(ids=np.zeros(3, np.int64)), ValueError, "set_triangle_materials: expected an int32 array of shape (n,), got int64 (3,)"),
    ("set_triangle_materials", dict(ids=i4(3, 1)), ValueError, "set_triangle_materials: expected an int32 array of shape (n,), got int32 (3, 1)"),
    ("set_triangle_materials", dict(ids=[0]), ValueError, "set_triangle_materials: expected a numpy array or a torch tensor, got list"),
    ("set_triangle_materials", dict(ids=i4(3), stream=1.5), TypeError, "set_triangle_materials: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got float"),
    ("set_triangle_materials", dict(ids=i4(3), stream=-2), ValueError, "set_triangle_materials: a hipStream_t is not negative, got -2"),
    ("update_attributes", dict(), ValueError, "update_attributes: none of uv, normals, tangents given"),
    ("update_attributes", dict(uv=[0]), ValueError, "update_attributes: uv: expected a numpy array or a torch tensor, got list"),
    ("update_attributes", dict(uv=f8(3, 6)), ValueError, "update_attributes: uv: expected a float32 array of shape (n, 6)" + HOST + "ndarray float64 (3, 6)"),
    ("update_attributes", dict(normals=f4(3, 6)), ValueError, "update_attributes: normals: expected a float32 array of shape (n, 9)" + HOST + "ndarray float32 (3, 6)"),
    ("update_attributes", dict(tangents=f4(3, 9, 1)), ValueError, "update_attributes: tangents: expected a float32 array of shape (n, 9)" + HOST + "ndarray float32 (3, 9, 1)"),
    ("update_attributes", dict(uv=f4(3, 6), normals=[0]), ValueError, "update_attributes: normals: expected a float32 array of shape (n, 9)" + HOST + "list None ()"),
    ("update_attributes", dict(uv=f4(3, 6), normals=torch.zeros(3, 9)), ValueError, "update_attributes: normals: expected a float32 array of shape (n, 9)" + HOST + "Tensor torch.float32 (3, 9)"),
    ("update_attributes", dict(uv=f4(3, 6), normals=f4(4, 9)), ValueError, "update_attributes: normals has 4 rows, uv has 3"),
    ("update_attributes", dict(uv=torch.zeros(3, 6), normals=f4(3, 9)), ValueError, "update_attributes: uv: expected a contiguous float32 (n, 6) tensor" + THERE + "Tensor torch.float32 (3, 6) on cpu"),
    ("update_attributes", dict(uv=f4(3, 6), stream="x"), TypeError, "update_attributes: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("update_attributes", dict(uv=f4(3, 6), stream=-1), ValueError, "update_attributes: a hipStream_t is not negative, got -1"),
    ("set_geometry", GEO(vertices=[0]), ValueError, "set_geometry: vertices: expected a numpy array or a torch tensor, got list"),
    ("set_geometry", GEO(vertices=f8(3, 3)), ValueError, "set_geometry: vertices: expected a float32 array of shape (n, 3)" + HOST + "ndarray float64 (3, 3)"),
    ("set_geometry", GEO(vertices=f4(0, 3)), ValueError, "set_geometry: vertices: expected a float32 array of shape (n, 3)" + HOST + "ndarray float32 (0, 3)"),
    ("set_geometry", GEO(indices=i4(3, 4)), ValueError, "set_geometry: indices: expected a int32 array of shape (n, 3)" + HOST + "ndarray int32 (3, 4)"),
    ("set_geometry", GEO(indices=torch.zeros(3, 3, dtype=I32)), ValueError, "set_geometry: indices: expected a int32 array of shape (n, 3)" + HOST + "Tensor torch.int32 (3, 3)"),
    ("set_geometry", GEO(tri_material=i4(4)), ValueError, "set_geometry: tri_material: expected a int32 array of shape (3)" + HOST + "ndarray int32 (4,)"),
    ("set_geometry", GEO(tri_material=1.5), ValueError, "set_geometry: tri_material: expected a int32 array of shape (3)" + HOST + "float None ()"),
    ("set_geometry", GEO(tri_light=f4(3)), ValueError, "set_geometry: tri_light: expected a int32 array of shape (3)" + HOST + "ndarray float32 (3,)"),
    ("set_geometry", GEO(uv=f4(3, 9)), ValueError, "set_geometry: uv: expected a float32 array of shape (3, 6)" + HOST + "ndarray float32 (3, 9)"),
    ("set_geometry", GEO(normals=f4(2, 9)), ValueError, "set_geometry: normals: expected a float32 array of shape (3, 9)" + HOST + "ndarray float32 (2, 9)"),
    ("set_geometry", GEO(medium_inside=i4(3)), ValueError, "set_geometry: medium_inside and medium_outside come together or not at all"),
    ("set_geometry", GEO(vertices=torch.zeros(3, 3)), ValueError, "set_geometry: vertices: expected a contiguous float32 array of shape (n, 3)" + THERE + "Tensor torch.float32 (3, 3) on cpu"),
    ("set_geometry", GEO(stream="x"), TypeError, "set_geometry: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("set_geometry", GEO(vertices=[0], stream=-1), ValueError, "set_geometry: vertices: expected a numpy array or a torch tensor, got list"),
    ("set_geometry", GEO(vertices=f8(3, 3), stream=-1), ValueError, "set_geometry: a hipStream_t is not negative, got -1"),
    ("update_environment", dict(rgb=f8(2, 2, 3)), ValueError, "update_environment: expected a float32 array of shape (h, w, 3), got float64 (2, 2, 3)"),
    ("update_environment", dict(rgb=f4(2, 2, 4)), ValueError, "update_environment: expected a float32 array of shape (h, w, 3), got float32 (2, 2, 4)"),
    ("update_environment", dict(rgb=f4(2, 3)), ValueError, "update_environment: expected a float32 array of shape (h, w, 3), got float32 (2, 3)"),
    ("update_environment", dict(rgb=[0]), ValueError, "update_environment: expected a numpy array, a torch tensor or None, got list"),
    ("update_environment", dict(stream="x"), TypeError, "update_environment: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("update_environment", dict(rgb=f4(2, 2, 3), stream=-1), ValueError, "update_environment: a hipStream_t is not negative, got -1"),
    ("update_media", dict(media=[1]), ValueError, "update_media: media must be gnxr Medium records, got int"),
    ("update_media", dict(media=grid_medium(), density=1), ValueError, "update_media: expected a numpy array, a torch tensor, a list of them or None, got int"),
    ("update_media", dict(media=grid_medium(), density=[f4(8), f4(8)]), ValueError, "update_media: 2 density arrays for 1 GRID records"),
    ("update_media", dict(media=[grid_medium(), grid_medium()], density=[f4(8), torch.zeros(8)]), ValueError, "update_media: density arrays must be all numpy arrays or all torch tensors"),
    ("update_media", dict(media=grid_medium(), density=f8(2, 2, 2)), ValueError, "update_media: expected a float32 array of shape (2, 2, 2) or (8,), got float64 (2, 2, 2)"),
    ("update_media", dict(media=grid_medium(), density=f4(2, 2, 3)), ValueError, "update_media: expected a float32 array of shape (2, 2, 2) or (8,), got float32 (2, 2, 3)"),
    ("update_media", dict(media=grid_medium(), density=[[0]]), ValueError, "update_media: expected a numpy array or a torch tensor, got list"),
    ("update_media", dict(media=grid_medium(), stream="x"), TypeError, "update_media: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("update_media", dict(media=grid_medium(), density=f4(8), stream=-1), ValueError, "update_media: a hipStream_t is not negative, got -1"),
    ("update_textures", dict(images=1), ValueError, "update_textures: expected a numpy array, a torch tensor, a list of them or None, got int"),
    ("update_textures", dict(params=1), ValueError, "update_textures: params must be a dict, a list of dicts or None, got int"),
    ("update_textures", dict(), ValueError, "update_textures: neither images nor params given"),
    ("update_textures", dict(images=f4(2, 2, 3), params=[{}, {}]), ValueError, "update_textures: 2 parameter dicts for 1 images"),
    ("update_textures", dict(images=[f4(2, 2, 3), f4(2, 2, 3)]), ValueError, "update_textures: textures [0, 2) outside the scene's 1 textures"),
    ("update_textures", dict(params={"x": 1}), ValueError, "update_textures: unknown texture parameter 'x' (expected one of su, sv, du, dv, trilinear, max_aniso, wrap, scale, gamma)"),
    ("update_textures", dict(params={"wrap": "x"}), ValueError, "update_textures: wrap must be 'repeat', 'black' or 'clamp', got 'x'"),
    ("update_textures", dict(images=f8(2, 2, 3)), ValueError, "update_textures: expected a float32 array of shape (h, w, 3), got float64 (2, 2, 3)"),
    ("update_textures", dict(images=f4(0, 2, 3)), ValueError, "update_textures: expected a float32 array of shape (h, w, 3), got float32 (0, 2, 3)"),
    ("update_textures", dict(images=f4(2, 2, 3, 1)), ValueError, "update_textures: expected a float32 array of shape (h, w, 3), got float32 (2, 2, 3, 1)"),
    ("update_textures", dict(images=[[0]]), ValueError, "update_textures: expected a numpy array or a torch tensor, got list"),
    ("update_textures", dict(params={"su": 2.0}, stream="x"), TypeError, "update_textures: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("update_textures", dict(images=f4(2, 2, 3), stream=-1), ValueError, "update_textures: a hipStream_t is not negative, got -1"),
    ("set_lights", dict(lights=[1]), ValueError, "set_lights: lights must be gnxr Light records, got int"),
    ("set_lights", dict(lights=[], stream="x"), TypeError, "set_lights: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got str"),
    ("recompute_normals", dict(stream=-1), ValueError, "recompute_normals: a hipStream_t is not negative, got -1"),
    ("rebuild_bvh", dict(stream=True), TypeError, "rebuild_bvh: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got bool"),
]
# the device-memory side of the same methods: `arg` as a tensor; n: the tail names no type
EDIT_TENSORS = [
    dict(name="update_vertices", args=dict, arrays=[arr("xyz", F32, (3, 3), "update_vertices: expected a contiguous float32 (n, 3) tensor on cuda:0, got ", tn=False)]),
    dict(name="set_triangle_materials", args=dict, arrays=[arr("ids", I32, (3,), "set_triangle_materials: expected a contiguous int32 (n,) tensor on cuda:0, got ", tn=False)]),
    dict(name="update_attributes", args=dict,
         arrays=[arr(w, F32, (3, c), f"update_attributes: {w}: expected a contiguous float32 (n, {c}) tensor" + THERE, rows=None if w == "uv" else f"update_attributes: {w} has 4 rows, uv has 3")
                 for w, c in (("uv", 6), ("normals", 9), ("tangents", 9))]),
    dict(name="set_geometry", args=dict,
         arrays=[arr("vertices", F32, (3, 3), "set_geometry: vertices: expected a contiguous float32 array of shape (n, 3)" + THERE),
                 arr("indices", I32, (3, 3), "set_geometry: indices: expected a contiguous int32 array of shape (n, 3)" + THERE,
                     rows="set_geometry: tri_material: expected a contiguous int32 array of shape (4)" + THERE + "Tensor torch.int32 (3,) on cuda:0")] +
                [arr(w, I32, (3,), f"set_geometry: {w}: expected a contiguous int32 array of shape (3)" + THERE,
                     rows=f"set_geometry: {w}: expected a contiguous int32 array of shape (3)" + THERE + "Tensor torch.int32 (4,) on cuda:0") for w in ("tri_material", "tri_light")] +
                [arr(w, F32, (3, c), f"set_geometry: {w}: expected a contiguous float32 array of shape (3, {c})" + THERE,
                     rows=f"set_geometry: {w}: expected a contiguous float32 array of shape (3, {c})" + THERE + f"Tensor torch.float32 (4, {c}) on cuda:0") for w, c in (("uv", 6), ("normals", 9))]),
    dict(name="update_environment", args=dict, arrays=[arr("rgb", F32, (2, 2, 3), "update_environment: expected a contiguous float32 (h, w, 3) tensor on cuda:0, got ", tn=False)]),
    dict(name="update_media", args=lambda: dict(media=grid_medium()),
         arrays=[arr("density", F32, (2, 2, 2), "update_media: expected a contiguous float32 (2, 2, 2) or (8,) tensor on cuda:0, got ", tn=False)]),
    dict(name="update_textures", args=dict, arrays=[arr("images", F32, (2, 2, 3), "update_textures: expected a contiguous float32 (h, w, 3) tensor on cuda:0, got ", tn=False)]),
]
for _r in EDIT_TENSORS:
    _r["call"] = (lambda name: lambda sc, **a: getattr(sc, name)(**a))(_r["name"])
NOT_AN_ARRAY = {"update_vertices": "update_vertices: expected a numpy array or a torch tensor, got list",
                "set_triangle_materials": "set_triangle_materials: expected a numpy array or a torch tensor, got list",
                "update_attributes": "update_attributes: uv: expected a numpy array or a torch tensor, got list",
                "set_geometry": "set_geometry: vertices: expected a numpy array or a torch tensor, got list",
                "update_environment": "update_environment: expected a numpy array, a torch tensor or None, got list"}


@pytest.mark.parametrize("case", EDITS, ids=lambda c: c[0])
def test_scene_edit_refuses_host_arguments(case):
    method, args, exc, message = case
    with pytest.raises(exc) as e:
        getattr(stub_scene(), method)(**args)
    assert type(e.value) is exc and str(e.value) == message, str(e.value)


@pytest.mark.parametrize("row", EDIT_TENSORS, **by_name)
def test_scene_edit_refuses_tensors_on_the_cpu(row):
    first = row["arrays"][0]
    for m in ("dtype", "trailing", "extra", "strided"):
        run_array(row, 0, m, "cpu")
    refused(row, good(row, "cpu"), ValueError, first["head"] + got("Tensor", first["dtype"], first["shape"], "cpu", tn=first["tn"]))


def test_a_list_is_no_array_of_a_scene_edit():
    """update_media and update_textures take a list as the list of their arrays, the others name it"""
    for row in EDIT_TENSORS:
        args = good(row, "cpu")
        args[row["arrays"][0]["arg"]] = [0]
        if row["name"] in ("update_media", "update_textures"):
            args[row["arrays"][0]["arg"]] = [[0]]
            refused(row, args, ValueError, row["name"] + ": expected a numpy array or a torch tensor, got list")
        else:
            refused(row, args, ValueError, NOT_AN_ARRAY[row["name"]])


CONSTRUCTORS = [
    (lambda: gx.TemporalAccumulator(PI, None, 0, 2, 1), "TemporalAccumulator: invalid image size 0 x 2"),
    (lambda: gx.TemporalAccumulator(PI, None, 2, 2, 0), "TemporalAccumulator: spp and max_history must be at least 1, got 0 and 32"),
    (lambda: gx.TemporalAccumulator(PI, None, 2, 2, 1, bogus=1), "TemporalAccumulator: unexpected arguments ['bogus'] (depth_tol, normal_cos)"),
    (lambda: gx.Display(0, 2), "Display: invalid size 1 x 0 x 2"), (lambda: gx.Display(2, 2, n_views=0), "Display: invalid size 0 x 2 x 2"),
    (lambda: gx.Display(2, 2, bogus=1), "Display: unexpected arguments ['bogus'] (min_log2, key, low, high, rate, min_exposure, max_exposure, curve, white, srgb, round)"),
    (lambda: gx.Display(2, 2, min_log2=200), "Display: min_log2 must lie in [-126, 111], got 200"),
    (lambda: gx.film_filter_table(1), "film_filter_table: expected a film_filter(...) record, got int"),
    (lambda: gx.camera_matrices(1, 2, 2), "camera_matrices: camera must be a gnxr Camera record (camera(...)), got int"),
]


@pytest.mark.parametrize("k", range(len(CONSTRUCTORS)))
def test_constructors_and_host_calls_refuse(k):
    make, message = CONSTRUCTORS[k]
    with pytest.raises(ValueError) as e:
        make()
    assert str(e.value) == message


def test_every_entry_point_has_a_row():
    import inspect
    covered = {r["name"].split(".")[-1] for r in ROWS + EDIT_TENSORS} | {"present"}
    takes_tensors = [n for n, f in inspect.getmembers(gx, inspect.isfunction) if f.__module__ == gx.__name__ and not n.startswith("_") and "stream" in inspect.signature(f).parameters]
    for cls in (gx.Scene, gx.PathIntegrator):
        takes_tensors += [n for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_") and "stream" in inspect.signature(f).parameters and
                          n not in ("RenderDevice", "set_lights", "recompute_normals", "rebuild_bvh")]   # (no array: a pointer, records, nothing)
    assert sorted(set(takes_tensors) - covered) == []


# ---------------------------------------------------------------- Part B: cuda:0
MUTATIONS = LAYOUT + ("cpu", "rows")


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS + EDIT_TENSORS if r["arrays"]], **by_name)
def test_every_array_is_refused_on_the_gpu(gpu, row):
    """Correct arrays on cuda:0 and one of them mutated at a time; `rows` only from the second array on (or against the scene's count)."""
    n = 0
    for k, a in enumerate(row["arrays"]):
        for m in MUTATIONS:
            if m == "list" and row in EDIT_TENSORS and k == 0:
                continue   # (test_a_list_is_no_array_of_a_scene_edit)
            if m == "rows" and k == 0 and not a.get("first_rows"):
                continue
            n += run_array(row, k, m, GPU)
    print(f"{row['name']}: {n} refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS if r["outs"]], **by_name)
def test_every_result_tensor_is_refused_on_the_gpu(gpu, row):
    """`out` of a wrong dtype, shape or layout, and in host memory"""
    n = 0
    for o in row["outs"]:
        for m in ("list", "dtype", "trailing", "extra", "strided", "cpu"):
            mut = mutate(o, m, GPU)
            if mut is None:
                continue
            args = good(row, GPU)
            if o["put"] is None:
                args[o["arg"]] = mut[0]
            else:
                o["put"](args, mut[0])
            refused(row, args, ValueError, o["head"] + got(*mut[1:]))
            n += 1
    print(f"{row['name']}: {n} refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS if r["gpu"] or r["cpu"]], **by_name)
def test_plain_arguments_are_refused_on_the_gpu(gpu, row):
    run_plain(row, GPU, row["cpu"] + row["gpu"])


@pytest.mark.gpu
def test_tensor_on_another_gpu(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: a tensor on another GPU cannot be built")
    for row in ROWS:
        for k, a in enumerate(row["arrays"][1:], 1):
            mut = torch.zeros(a["shape"], dtype=a["dtype"], device="cuda:1")
            args = good(row, GPU)
            args[a["arg"]] = mut
            refused(row, args, ValueError, a["head"] + got("Tensor", a["dtype"], a["shape"], "cuda:1", tn=a["tn"], dev=a["dev"]))
