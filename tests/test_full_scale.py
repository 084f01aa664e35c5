"""The launch plans at the sizes the benchmark and callers really use (run with -m gpu on an MI355X).

The other GPU modules pin the path loop at 48 x 40 or render two of the 1024 samples at 1920 x 1080: one sub-pass, one region, no reuse.
bench.py's call gets another plan (csrc/api_render.hip.h, RenderPlan::size_passes): 32 sub-passes of 32 spp, four alive
at once in regions of one 265 420 800-slot state, every region reused eight times, queues of different sub-passes merged, lagging counter
copies, ~130 k compaction tiles.  This module runs those plans -- and full-size batches through the device-memory entry points -- and
compares them bit for bit (image words and both ray counts; no tolerance anywhere) in two legs:

  oracle leg  the device renders the WHOLE frame with the plan under test; the CPU oracle renders horizontal stripes of it (shard_index = i,
              shard_count = ceil(H / r), shard_rows = r are exactly rows r * i .. r * i + r - 1, all columns, all samples of the call: slots
              are sample-major, so the top, middle and bottom stripes pin early, middle and late slots of every region).  A device render of
              the same stripe gives the ray counts the oracle's are compared with.
  plan leg    the same call through a plan the small tests pin (passes_in_flight = 1, a small samples_per_pass), whole frame and ray counts:
              extends the oracle's verdict from the stripes to every pixel.

Each case prints the plan it ran and asserts it, so a change of the default plan makes the test say so instead of quietly testing something
else.  The default cfg 3 plan needs ~140 GB of free HBM (four regions are granted while 63 GB < 0.45 x free); with less the plan assertion fails
and prints the free memory -- nothing here skips or falls back to a smaller plan.

Order: A (timed plans), B (device-memory entry points; every Scene is destroyed before the multi-GB tensors), C (refusals; the many-regions
cases, up to 150 GB of state, last)."""
import contextlib
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded: torch's HIP runtime must come up first for device tensors in this process)

import oracle_lib as ol
import scenes

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
PIX = W * H
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
SLOT_BYTES = 238            # path state per slot (kSlotBytesEstimate, csrc/api_render.hip.h; the plan rules below are stated in it)
STATE_CAP = 150e9           # kStateCapBytes: size_passes never grants more path state than this
COUNT_KEYS = ("rays_closest", "rays_any", "camera_samples")   # (loop_iterations / kernel_launches depend on when lagging counters arrive)
RAY_KEYS = ("rays_closest", "rays_any")                       # what the oracle counts
# hipMalloc hands out device memory in 2 MiB units on this runtime: a refused call may move free memory by bookkeeping of that size, not by
# path state (>= 63 GB in every refusal below)
ALLOC_GRANULE = 2 << 20
STRIPES_1080 = (0, 528, 1072)   # top rows, rows through the mesh, the (partial at r = 16) bottom stripe that ends with the last row


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def diff_report(a, b):
    """None when a and b hold the same words (NaN equal to NaN), else where they differ"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return f"shapes {a.shape} / {b.shape}"
    bad = ~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))
    if not bad.any():
        return None
    where = np.argwhere(bad)
    return f"{int(bad.sum())} of {bad.size} words differ, first at {where[0].tolist()}, last at {where[-1].tolist()}"


def same(a, b):
    return diff_report(a, b) is None


def plan(st, free=None):
    s = f"passes={st['passes']} passes_in_flight={st['passes_in_flight']} state_bytes={st['state_bytes']}"
    return s if free is None else s + f" (free device memory before the call: {free / 1e9:.1f} GB)"


def counts(st, keys=COUNT_KEYS):
    return tuple(st[k] for k in keys)


def free_bytes():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


@contextlib.contextmanager
def device_scene(gpu, b):
    """a Scene that is destroyed (path state included) when the block ends"""
    scene = gpu.Scene(b)
    try:
        yield scene
    finally:
        scene.close()
        torch.cuda.empty_cache()


def check_stripes(label, osc, integ, img, width, height, spp, r, starts, scene=None, **kw):
    """Oracle leg: rows y0 .. y0 + r - 1 of `img` (the device's whole frame) for every y0 of `starts` against the oracle's render of that
    stripe.  With `scene`, the device renders the stripe too: its image must be the frame's rows and its ray counts the oracle's."""
    n_stripes = -(-height // r)
    secs = 0.0
    for y0 in starts:
        assert y0 % r == 0 and y0 < height
        shard = dict(shard_index=y0 // r, shard_count=n_stripes, shard_rows=r)
        t = time.perf_counter()
        oimg, ost = osc.render(integ, width, height, spp, **shard, **kw)
        secs += time.perf_counter() - t
        y1 = min(y0 + r, height)
        assert oimg[y0:y1, :, :3].any(), f"{label}: rows {y0}..{y1 - 1} are black in the oracle: nothing would be compared"
        assert not oimg[:y0, :, :3].any() and not oimg[y1:, :, :3].any(), f"{label}: the oracle's stripe is not rows {y0}..{y1 - 1}"
        rep = diff_report(img[y0:y1, :, :3], oimg[y0:y1, :, :3])
        assert rep is None, f"{label}: rows {y0}..{y1 - 1} against the oracle: {rep}"
        if scene is not None:
            simg, sst = integ.Render(scene, width, height, spp, **shard, **kw)
            assert same(simg[y0:y1, :, :3], img[y0:y1, :, :3]), f"{label}: device stripe {y0} differs from the frame's rows"
            assert counts(sst, RAY_KEYS) == counts(ost, RAY_KEYS), f"{label}: stripe {y0}: device {counts(sst, RAY_KEYS)}, oracle {counts(ost, RAY_KEYS)}"
    print(f"{label}: rows {[(y, min(y + r, height) - 1) for y in starts]} x {width} columns equal the oracle's; oracle {secs:.1f} s")


def pinned_subset(n, m, seed, period):
    """at least m seeded indices of range(n), with the first 64, the last 64 and 64 either side of every multiple of `period`"""
    edge = [np.arange(0, 64), np.arange(n - 64, n)]
    for k in range(period, n, period):
        edge.append(np.arange(k - 64, min(k + 64, n)))
    rng = np.random.default_rng(seed)
    idx = np.unique(np.concatenate(edge + [rng.integers(0, n, m + m // 8)]))
    assert len(idx) >= m
    return idx


def frame_samples(width, height, spp):
    """px, py, s of every pixel and sample of a frame, sample-major (the order of the render's slots), int32 on the device"""
    i = torch.arange(width * height * spp, device="cuda")
    s = (i // (width * height)).to(torch.int32)
    i -= s.to(torch.int64) * (width * height)
    py = (i // width).to(torch.int32)
    px = (i % width).to(torch.int32)
    return px, py, s


def path_integrator(gpu):
    return gpu.PathIntegrator(8, 1.0, "spatial")


def cfg3_builder():
    return scenes.dragon_cornell(100000, "glass+metal")


@pytest.fixture(scope="module")
def b3(gpu):
    return cfg3_builder()


@pytest.fixture(scope="module")
def b4(gpu):
    return scenes.dragon_cornell(100000, "zoo", env=scenes.synthetic_env_path(1000, 500))


@pytest.fixture(scope="module")
def cfg3(gpu, b3):
    """bench.py's call -- cfg 3, 1920 x 1080, all 1024 samples, default plan -- twice on one scene object"""
    free = free_bytes()
    with device_scene(gpu, b3) as scene:
        first = path_integrator(gpu).Render(scene, W, H, 1024)
        second = path_integrator(gpu).Render(scene, W, H, 1024)
    return dict(free=free, first=first, second=second)


# ---------------------------------------------------------------- A. the timed plans
def test_cfg3_timed_plan(gpu, b3, cfg3):
    """cfg 3 as bench.py times it: 32 sub-passes of 32 spp, four in flight in a 63 GB state.  Two runs on one scene object are identical
    (the loop's schedule depends on when lagging counters reach the host, the result must not); the plan leg (64 passes of 16 spp, one
    region) equals it on every pixel; three 8-row stripes over all 1024 samples equal the oracle."""
    integ = path_integrator(gpu)
    (img, st), (img2, st2) = cfg3["first"], cfg3["second"]
    print(f"cfg 3 default plan: {plan(st, cfg3['free'])}")
    assert (st["passes"], st["passes_in_flight"]) == (32, 4) and st["state_bytes"] > 5e10, \
        f"not the timed plan (32 sub-passes, 4 in flight, > 5e10 bytes of state: needs ~140 GB free): {plan(st, cfg3['free'])}"
    assert st["camera_samples"] == PIX * 1024 and (img[..., 3] == 1).all()
    assert counts(st2) == counts(st) and plan(st2) == plan(st)
    rep = diff_report(img, img2)
    assert rep is None, f"two runs of the default plan on one scene differ: {rep}"
    with device_scene(gpu, b3) as scene:
        ref, rst = integ.Render(scene, W, H, 1024, samples_per_pass=16, passes_in_flight=1)
        print(f"cfg 3 plan leg: {plan(rst)}")
        assert (rst["passes"], rst["passes_in_flight"]) == (64, 1)
        assert counts(st) == counts(rst), (counts(st), counts(rst))
        rep = diff_report(img, ref)
        assert rep is None, f"default plan against 64 x 16 spp in one region: {rep}"
        check_stripes("cfg 3, 1024 spp", ol.OracleScene(b3), integ, img, W, H, 1024, 8, STRIPES_1080, scene=scene)


def test_cfg4_timed_plan(gpu, b4):
    """cfg 4 (environment light, Plastic, Disney: escape queue and forked shade streams): samples 768 .. 1023 at 1920 x 1080, eight sub-passes
    of 32 spp, four in flight, every region reused once."""
    integ = path_integrator(gpu)
    kw = dict(spp_begin=768, spp_end=1024)
    free = free_bytes()
    with device_scene(gpu, b4) as scene:
        img, st = integ.Render(scene, W, H, 1024, **kw)
        print(f"cfg 4 default plan, samples 768..1023: {plan(st, free)}")
        assert (st["passes"], st["passes_in_flight"]) == (256 // 32, 4), f"not the timed plan: {plan(st, free)}"
        assert st["camera_samples"] == PIX * 256
        ref, rst = integ.Render(scene, W, H, 1024, samples_per_pass=16, passes_in_flight=1, **kw)
        print(f"cfg 4 plan leg: {plan(rst)}")
        assert (rst["passes"], rst["passes_in_flight"]) == (16, 1)
        assert counts(st) == counts(rst), (counts(st), counts(rst))
        rep = diff_report(img, ref)
        assert rep is None, f"default plan against 16 x 16 spp in one region: {rep}"
        check_stripes("cfg 4, samples 768..1023", ol.OracleScene(b4), integ, img, W, H, 1024, 16, STRIPES_1080, scene=scene, **kw)


def test_cfg5_timed_plan(gpu):
    """cfg 5 (VolPath, 512 x 512, 256 spp): one pass of 64 Mi paths -- packing, parked tracking loops, 64 Mi-slot compaction -- against 16
    passes of 16 spp and against 8-row oracle stripes (top, through the smoke, bottom)."""
    b = scenes.volume_cornell_cfg5(1.0)
    integ = gpu.VolPathIntegrator(8, 1.0, "spatial")
    free = free_bytes()
    with device_scene(gpu, b) as scene:
        img, st = integ.Render(scene, 512, 512, 256)
        print(f"cfg 5 default plan: {plan(st, free)}")
        assert st["passes"] == 1, f"not the timed plan: {plan(st, free)}"
        assert st["camera_samples"] == 512 * 512 * 256
        ref, rst = integ.Render(scene, 512, 512, 256, samples_per_pass=16)
        print(f"cfg 5 plan leg: {plan(rst)}")
        assert rst["passes"] == 16
        assert counts(st) == counts(rst), (counts(st), counts(rst))
        rep = diff_report(img, ref)
        assert rep is None, f"one pass against 16 x 16 spp: {rep}"
        check_stripes("cfg 5, 256 spp", ol.OracleScene(b), integ, img, 512, 512, 256, 8, (0, 328, 504), scene=scene)


@pytest.mark.parametrize("name", ["whitted", "direct_all"])
def test_whitted_and_direct_at_full_resolution(gpu, b4, name):
    """The depth-first integrators on the cfg 4 scene at 1920 x 1080, 8 samples: the default plan gives them 1 - 2 samples per pass here, i.e.
    several passes over per-record state `record * cap + path` with cap in the millions.  Plan leg: another pass size (another cap)."""
    integ, k = (gpu.WhittedIntegrator(5), 1) if name == "whitted" else (gpu.DirectLightingIntegrator("all", 3), 3)
    free = free_bytes()
    with device_scene(gpu, b4) as scene:
        img, st = integ.Render(scene, W, H, 8)
        print(f"{name} default plan: {plan(st, free)}")
        assert st["passes"] > 1, plan(st, free)
        assert st["camera_samples"] == PIX * 8
        ref, rst = integ.Render(scene, W, H, 8, samples_per_pass=k, passes_in_flight=1)
        print(f"{name} plan leg: {plan(rst)}")
        assert rst["passes"] == -(-8 // k) and rst["passes"] != st["passes"], "the plan leg must be another plan than the default"
        assert counts(st) == counts(rst), (counts(st), counts(rst))
        rep = diff_report(img, ref)
        assert rep is None, f"default plan against samples_per_pass = {k}: {rep}"
        check_stripes(f"{name}, 8 spp", ol.OracleScene(b4), integ, img, W, H, 8, 16, STRIPES_1080, scene=scene)


# ---------------------------------------------------------------- B. full-size batches through the device-memory entry points
def test_ray_queries_full_size_batch(gpu, b3):
    """Scene.intersect / occluded with ONE batch of 2^27 + 5 rays made on the device (4.3 GB of rays, as much of hits): a seeded subset of
    >= 2^20 answers (the ends and both sides of every multiple of 2^26 included) against the oracle, and the whole answer against the same
    rays sent in 2^22-ray batches."""
    n, step = (1 << 27) + 5, 1 << 22
    g = torch.Generator(device="cuda")
    g.manual_seed(20)
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    for a in range(0, n, 1 << 24):   # (in pieces: bounded temporaries)
        m = min(1 << 24, n - a)
        d = torch.randn((m, 3), generator=g, device="cuda")
        t = torch.rand((m,), generator=g, device="cuda") * 5.7 + 0.3   # segments shorter and longer than the box ...
        t[::2] = math.inf                                               # ... and unbounded rays
        rays[a:a + m, 0:3] = torch.rand((m, 3), generator=g, device="cuda") * 4.8 - 2.4
        rays[a:a + m, 3] = t
        rays[a:a + m, 4:7] = d / d.norm(dim=1, keepdim=True)
    del d, t
    idx = pinned_subset(n, 1 << 20, 21, 1 << 26)
    tidx = torch.from_numpy(idx).cuda()
    with device_scene(gpu, b3) as scene:
        t0 = time.perf_counter()
        hits = scene.intersect(rays).hits
        occ = scene.occluded(rays)
        torch.cuda.synchronize()
        print(f"intersect + occluded of {n} rays in one batch each: {time.perf_counter() - t0:.2f} s")
        hits2, occ2 = torch.empty_like(hits), torch.empty_like(occ)
        for a in range(0, n, step):
            scene.intersect(rays[a:a + step], out=hits2[a:a + step])
            scene.occluded(rays[a:a + step], out=occ2[a:a + step])
        torch.cuda.synchronize()
        assert torch.equal(hits.view(torch.int32), hits2.view(torch.int32)), "one batch and 2^22-ray batches give different hit records"
        assert torch.equal(occ, occ2), "one batch and 2^22-ray batches give different occlusion flags"
        sub = rays[tidx].cpu().numpy()
        h = np.ascontiguousarray(hits[tidx].cpu().numpy()).view(gpu.HIT_DTYPE).reshape(-1)
        o = occ[tidx].cpu().numpy()
    del rays, hits, hits2, occ, occ2
    torch.cuda.empty_cache()
    osc = ol.OracleScene(b3)
    oh, oo = osc.Intersect(sub), osc.IntersectP(sub)
    assert (h["prim"] == oh["prim"]).all(), f"{int((h['prim'] != oh['prim']).sum())} primitives differ, first at ray {idx[np.argmax(h['prim'] != oh['prim'])]}"
    m = oh["prim"] >= 0
    assert 0.5 < m.mean() < 1.0 and (h["prim"][:64] == oh["prim"][:64]).all() and (h["prim"][-64:] == oh["prim"][-64:]).all()
    for f in ("t", "b0", "b1", "b2", "n"):
        assert same(h[f][m], oh[f][m]), f
    assert (o == oo).all() and 0.05 < oo.mean() < 0.95


def test_li_full_frame_three_chunks(gpu, b3):
    """integrator.Li on the camera rays of a whole 1920 x 1080 frame x 96 samples (199 065 600 rays = 2.97 x 2^26: three default chunks in
    three regions), summed in sample order and divided by spp: equal to Render of the same samples on every pixel (the identity
    test_li_of_camera_rays_equals_render asserts at 64 x 64) and to the oracle on three stripes."""
    integ, spp = path_integrator(gpu), 96
    n = PIX * spp
    d = b3.desc()
    with device_scene(gpu, b3) as scene:
        px, py, s = frame_samples(W, H, spp)
        rays, samples = gpu.camera_rays_device(d.camera, W, H, px, py, s)
        del px, py, s
        free = free_bytes()
        t0 = time.perf_counter()
        L, st = integ.Li(scene, rays, samples, W, H, spp)
        torch.cuda.synchronize()
        print(f"Li of {n} camera rays: {plan(st, free)}, {time.perf_counter() - t0:.2f} s")
        assert st["passes"] == 3 == -(-n // (1 << 26)), f"not the default chunking: {plan(st, free)}"
        assert st["camera_samples"] == n
        Lv = L.view(spp, H, W, 4)
        assert bool((Lv[..., 3] == 1).all())
        acc = np.zeros((H, W, 3), np.float32)
        for k in range(spp):   # colObj += Li in sample order, then / spp: k_resolve and k_finish
            acc += Lv[k, :, :, :3].cpu().numpy()
        img = acc / np.float32(spp)
        del rays, samples, L, Lv
        torch.cuda.empty_cache()
        ref, rst = integ.Render(scene, W, H, spp)
        for k in ("rays_closest", "rays_any", "rays_closest_nee"):
            assert st[k] == rst[k], (k, st[k], rst[k])
        rep = diff_report(img, ref[..., :3])
        assert rep is None, f"Li of the camera rays against Render: {rep}"
        check_stripes("Li, 96 spp", ol.OracleScene(b3), integ, img, W, H, spp, 16, STRIPES_1080)


def view_arc(V):
    """V cameras on an arc in front of the Cornell box's open side, at changing heights and two fields of view"""
    cams = []
    for v in range(V):
        a = math.radians(-40.0 + 80.0 * v / max(1, V - 1))
        cams.append(dict(eye=(5.0 * math.sin(a), 0.5 * math.cos(3 * a), 5.0 * math.cos(a)), look=(0, 0, 0), up=(0, 1, 0), fov=90.0 if v % 2 == 0 else 60.0))
    return cams


def test_render_views_64_cameras(gpu):
    """integrator.RenderViews with 64 cameras at 512 x 512, 16 spp on the cfg 3 scene (16.8 M pixels per sample: four sub-passes of 4 spp in
    flight): every view equals set_camera + Render whole-frame, the ray counts are their sums, and stripes of the first, a middle and the
    last view equal the oracle's render through that camera."""
    V, S, spp = 64, 512, 16
    b = cfg3_builder()   # (a builder of its own: set_camera below changes it)
    integ = path_integrator(gpu)
    arc = view_arc(V)
    free = free_bytes()
    with device_scene(gpu, b) as scene:
        out, st = integ.RenderViews(scene, [gpu.camera(**c) for c in arc], S, S, spp)
        torch.cuda.synchronize()
        img = out.cpu().numpy()
        del out
        print(f"RenderViews, {V} views of {S} x {S} at {spp} spp: {plan(st, free)}")
        assert (st["passes"], st["passes_in_flight"]) == (4, 4), f"not the default plan of this call: {plan(st, free)}"
        assert st["camera_samples"] == V * S * S * spp
        total = [0, 0]
        for v in range(V):
            scene.set_camera(**arc[v])
            one, s1 = integ.Render(scene, S, S, spp)
            rep = diff_report(img[v], one)
            assert rep is None and one[..., :3].any(), f"view {v} against set_camera + Render: {rep}"
            total[0] += s1["rays_closest"]
            total[1] += s1["rays_any"]
        assert (st["rays_closest"], st["rays_any"]) == tuple(total)
    for v in (0, V // 2, V - 1):
        b.set_camera(**arc[v])
        check_stripes(f"view {v}", ol.OracleScene(b), integ, img[v], S, S, spp, 16, (0, 256, 496))


def test_bsdf_full_size_batch(gpu, b3):
    """Scene.bsdf on ONE batch of 1920 x 1080 x 33 = 68 428 800 >= 2^26 camera rays: a seeded subset of >= 2^20 rows (the ends, both sides of
    2^26 and of every multiple of the call's 2^22-ray rounds included) against OracleScene.bsdf_probe."""
    spp = 33
    n = PIX * spp
    assert n >= 1 << 26
    d = b3.desc()
    g = torch.Generator(device="cuda")
    g.manual_seed(22)
    idx = np.unique(np.concatenate([pinned_subset(n, 1 << 20, 23, 1 << 26), pinned_subset(n, 1, 24, 1 << 22)]))
    tidx = torch.from_numpy(idx).cuda()
    with device_scene(gpu, b3) as scene:
        px, py, s = frame_samples(W, H, spp)
        rays, _ = gpu.camera_rays_device(d.camera, W, H, px, py, s)
        del px, py, s, _
        wi = torch.randn((n, 3), generator=g, device="cuda")
        wi /= wi.norm(dim=1, keepdim=True)
        u = torch.rand((n, 2), generator=g, device="cuda")
        t0 = time.perf_counter()
        out = scene.bsdf(rays, wi, u)
        torch.cuda.synchronize()
        print(f"bsdf of {n} camera rays in one batch: {time.perf_counter() - t0:.2f} s")
        got = out[tidx].cpu().numpy()
        sub, swi, su = rays[tidx].cpu().numpy(), wi[tidx].cpu().numpy(), u[tidx].cpu().numpy()
        del rays, wi, u, out
    want = ol.OracleScene(b3).bsdf_probe(sub, swi, su, 31)
    assert (want[:, 13] == 1).mean() >= 0.25
    rep = diff_report(got, want)
    assert rep is None, f"bsdf rows {idx[0]} .. {idx[-1]} against the oracle: {rep}"


# ---------------------------------------------------------------- C. the refusals at the 32-bit limits
def refused(gpu, call, code, text):
    """`call` raises GnxrError `code` whose message holds `text`, and free device memory is the same afterwards (to the allocator's unit):
    the refusal comes before any path state is allocated"""
    before = free_bytes()
    with pytest.raises(gpu.GnxrError) as e:
        call()
    after = free_bytes()
    print(f"refused ({e.value}); free device memory moved by {before - after} bytes")
    assert f"gnxr error {code}:" in str(e.value) and text in str(e.value), str(e.value)
    assert abs(before - after) <= ALLOC_GRANULE, (before, after)


def still_renders(gpu, scene, b):
    """the handle is usable after a refusal: a small frame equals the oracle's"""
    integ = gpu.PathIntegrator(5, 1.0, "spatial")
    img, st = integ.Render(scene, 48, 40, 4)
    oimg, ost = ol.OracleScene(b).render(integ, 48, 40, 4)
    assert counts(st, RAY_KEYS) == counts(ost, RAY_KEYS) and same(img[..., :3], oimg[..., :3]) and img[..., :3].any()


def halton_need(width, height):
    """HaltonSampler's sample stride (the smallest 2^a >= min(width, 128) times the smallest 3^b >= min(height, 128), HaltonSampler.cpp:33-60)
    and the smallest X with stride * X >= 2^32: a render is refused when spp * max(Light::nSamples used) + 1 >= X"""
    s2 = 1
    while s2 < min(width, 128): s2 *= 2
    s3 = 1
    while s3 < min(height, 128): s3 *= 3
    return s2 * s3, -(-(1 << 32) // (s2 * s3))


def test_refuses_pass_too_large(gpu):
    """samples_per_pass = 1024 at 1920 x 1080 is 2 123 366 400 slots: 1.1 % below 2^31, but the traversal's 32-bit work cursor counts a
    continuation ray and two NEE items per slot, and cap * 3 >= 2^32.  DirectLighting("all") is refused by the same rule much earlier:
    cap * (1 + 2 * records) reaches 2^32 with cap itself (and cap * records) below 2^31."""
    b = scenes.cornell()
    with device_scene(gpu, b) as scene:
        still_renders(gpu, scene, b)   # (light grid and the small frame's state exist before free memory is read)
        assert PIX * 1024 * 3 >= 1 << 32
        refused(gpu, lambda: path_integrator(gpu).Render(scene, W, H, 1024, samples_per_pass=1024), ERR_INVALID, "pass too large")
        still_renders(gpu, scene, b)
        d = b.desc()
        recs = sum(max(1, d.lights[i].n_samples) for i in range(d.n_lights))
        k = -(-(1 << 32) // ((1 + 2 * recs) * PIX))
        cap = k * PIX
        assert recs > 1 and k <= 1024 and cap < 1 << 31 and cap * recs < 1 << 31 and cap * (1 + 2 * recs) >= 1 << 32, (recs, k)
        refused(gpu, lambda: gpu.DirectLightingIntegrator("all", 3).Render(scene, W, H, 1024, samples_per_pass=k), ERR_INVALID, "pass too large")
        still_renders(gpu, scene, b)


@pytest.mark.parametrize("name", ["path", "direct_all"])
def test_refuses_spp_beyond_32_bit_halton_indices(gpu, name):
    """stride * (spp * max_light_samples + 1) >= 2^32 is refused (GNXR_ERR_UNSUPPORTED); one sample less per pixel renders, and its LAST
    sample -- the largest Halton indices a call can draw -- equals the oracle's."""
    b = scenes.cornell()
    d = b.desc()
    integ, m = (gpu.PathIntegrator(5, 1.0, "spatial"), 1) if name == "path" else (gpu.DirectLightingIntegrator("all", 3), max(d.lights[i].n_samples for i in range(d.n_lights)))
    stride, need = halton_need(128, 128)
    spp = -(-(need - 1) // m)   # the smallest refused spp
    assert stride == 128 * 243 and (m == 1 or m == 5)
    assert stride * (spp * m + 1) >= 1 << 32 > stride * ((spp - 1) * m + 1)
    with device_scene(gpu, b) as scene:
        still_renders(gpu, scene, b)
        refused(gpu, lambda: integ.Render(scene, 128, 128, spp, spp_begin=0, spp_end=1), ERR_UNSUPPORTED, "spp too large for 32-bit Halton indices")
        still_renders(gpu, scene, b)
        kw = dict(spp_begin=spp - 2, spp_end=spp - 1)
        img, st = integ.Render(scene, 128, 128, spp - 1, **kw)
        oimg, ost = ol.OracleScene(b).render(integ, 128, 128, spp - 1, **kw)
        assert counts(st, RAY_KEYS) == counts(ost, RAY_KEYS) and st["rays_any"] > 0
        rep = diff_report(img[..., :3], oimg[..., :3])
        assert rep is None and img[..., :3].any(), rep


def test_refuses_views_beyond_32_bit_path_indexing(gpu):
    """RenderViews with n_views * W * H one view above kMaxViewPixels = (2^32 - 1) / 3 (86 views of 4096 x 4096) is refused before the output
    is looked at (the image pointer is a 256-byte tensor); exactly at the limit is not rendered here (memory)."""
    b = scenes.cornell()
    kmax = ((1 << 32) - 1) // 3
    S = 4096
    V = kmax // (S * S) + 1
    assert (V - 1) * S * S <= kmax < V * S * S and V == 86
    integ = path_integrator(gpu)
    with device_scene(gpu, b) as scene:
        still_renders(gpu, scene, b)
        p = integ.params(S, S, 1)
        cams = (gpu.Camera * V)(*[gpu.camera() for _ in range(V)])
        small = torch.zeros(64, dtype=torch.float32, device="cuda")
        st = gpu.Stats()
        before = free_bytes()
        rc = gpu.lib().gnxr_render_views_device(scene._h, C.byref(p), cams, None, V, C.c_void_p(small.data_ptr()), None, C.byref(st))
        after = free_bytes()
        msg = gpu.lib().gnxr_last_error().decode()
        print(f"refused ({rc}: {msg}); free device memory moved by {before - after} bytes")
        assert rc == ERR_INVALID and "overflow the 32-bit path indexing" in msg and str(kmax) in msg
        assert abs(before - after) <= ALLOC_GRANULE and not bool(small.any())
        still_renders(gpu, scene, b)


@pytest.mark.parametrize("k", [32, 64])
def test_more_regions_than_the_default(gpu, b3, cfg3, k):
    """passes_in_flight = 8 at 1920 x 1080: with 32 spp per sub-pass 530 M slots (126 GB: inside the index rules and the 150 GB cap, granted
    while the growth fits 0.45 x free), with 64 spp 253 GB, which the cap must cut down.  Neither may fail; whatever is granted renders the
    image and ray counts of the default plan.  (The granted value depends on the memory other users of the card hold: printed, not pinned.)"""
    free = free_bytes()
    with device_scene(gpu, b3) as scene:
        img, st = path_integrator(gpu).Render(scene, W, H, 1024, samples_per_pass=k, passes_in_flight=8)
    granted = st["passes_in_flight"]
    print(f"asked for 8 regions of {k} spp, granted {granted}: {plan(st, free)}")
    assert 1 <= granted <= 8 and st["passes"] == 1024 // k
    assert granted * k * PIX * SLOT_BYTES <= STATE_CAP, plan(st, free)
    ref, rst = cfg3["first"]
    assert counts(st) == counts(rst), (counts(st), counts(rst))
    rep = diff_report(img, ref)
    assert rep is None, f"{granted} regions of {k} spp against the default plan: {rep}"

