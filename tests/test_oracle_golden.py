"""The CPU oracle against the golden vectors generated from the COMPILED REFERENCE (oracle/make_goldens.py).
Everything here is bit-exact: the oracle runs the reference's arithmetic on the same x86-64 SSE2 target."""
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import scenes
from conftest import GOLDEN, golden
import os


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def test_rng():
    g = golden("rng.npz")["u32"]
    assert (ol.oracle_rng(64) == g[:64]).all() and (ol.oracle_rng(64, 7) == g[64:]).all()


def test_permutations_and_primes():
    g = golden("perms.npz")
    p = ol.oracle_perms()
    assert len(p) == int(g["n"]) == 3682913
    assert zlib.crc32(p.tobytes()) == int(g["crc32"])
    assert (p[:4096] == g["head"]).all()
    gp = golden("primes.npz")
    pr, sm = ol.oracle_primes()
    assert (pr == gp["primes"]).all() and (sm == gp["sums"]).all()


@pytest.mark.parametrize("res", [(256, 256), (1920, 1080), (64, 64)])
def test_halton(res):
    g = golden(f"halton_{res[0]}x{res[1]}.npz")
    q = g["q"]
    v = ol.oracle_halton(res[0], res[1], q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    assert (v.view(np.uint32) == g["bits"]).all()
    assert (v >= 0).all() and (v < 1).all()


@pytest.mark.parametrize("res", [(256, 256), (1920, 1080)])
def test_camera_rays(res):
    g = golden(f"camrays_{res[0]}x{res[1]}.npz")
    b = scenes.cornell()
    o, d = ol.oracle_camera_rays(b.desc().camera, res[0], res[1], g["q"][:, 0], g["q"][:, 1], g["q"][:, 2])
    assert biteq(np.concatenate([o, d], 1), g["od"])


def _scene(name):
    if name == "cornell":
        return scenes.cornell()
    return scenes.dragon_cornell(2000, "glass+metal", mesh_path=os.path.join(GOLDEN, "mesh_2k.3d"))


@pytest.mark.parametrize("name", ["cornell", "mesh2k"])
def test_bvh_and_hits(name):
    b = _scene(name)
    osc = ol.OracleScene(b)
    g = golden(f"bvh_{name}.npz")
    bounds, off, npr, ax, order = osc.bvh(b.desc().n_triangles)
    assert biteq(bounds, g["bounds"])
    assert (off == g["meta"][:, 0]).all() and (npr == g["meta"][:, 1]).all() and (ax == g["meta"][:, 2]).all()
    assert (order == g["order"]).all()
    h = golden(f"hits_{name}.npz")
    oh = osc.Intersect(h["rays"])
    assert (oh["prim"] == h["prim"]).all()
    m = h["prim"] >= 0
    assert m.sum() > 1000
    assert biteq(oh["t"][m], h["t"][m]) and biteq(oh["n"][m], h["n"][m])
    assert (osc.IntersectP(h["srays"]) == h["occluded"]).all()


def test_bsdf_tables():
    g = golden("bsdf_zoo.npz")
    osc = ol.OracleScene(scenes.material_zoo())
    for flags in (31, 15):
        o = osc.bsdf_probe(g["rays"], g["wi"], g["u"], flags)
        assert biteq(o, g[f"out_{flags}"]), flags
    assert (g["out_31"][:, 13] == 1).sum() > 4000


def test_area_lights_and_spatial_distribution():
    g = golden("light_area.npz")
    osc = ol.OracleScene(scenes.cornell())
    for li in (0, 1):
        o = osc.light_probe(li, g["refP"], g["refN"], g["u"], g["wiQ"])
        r = g[f"light{li}"].copy()
        o[:, 8] = 0
        r[:, 8] = 0
        assert biteq(o, r), li
    for li in (0, 1):
        pdf = osc.light_probe(li, g["pts"], g["pts"] * 0, g["pts"][:, :2] * 0 + 0.5, g["pts"], strategy=0)[:, 8]
        assert biteq(pdf, g["spatial_pdf"][:, li])


def test_env_and_skybox_lights():
    g = golden("light_env.npz")
    b = scenes.cornell(sky=True)
    b.AddInfLight(os.path.join(GOLDEN, "env_100x50.hdr"))
    d = b.desc()
    px = np.ctypeslib.as_array(d.env_rgb, shape=(d.env_height, d.env_width, 3))
    assert biteq(px, g["hdr_pixels"])          # RGBE reader == stbi_loadf
    osc = ol.OracleScene(b)
    for li, nm in ((2, "sky"), (3, "env")):
        o = osc.light_probe(li, g["refP"], g["refN"], g["u"], g["wiQ"], strategy=1)
        r = g[nm].copy()
        o[:, 8] = 0
        r[:, 8] = 0
        pdf_pos = r[:, 3] > 0
        assert biteq(o[:, :8], r[:, :8]), nm
        assert biteq(o[pdf_pos, 9:], r[pdf_pos, 9:]), nm
        assert biteq(osc.light_le(li, g[nm + "_rays"]), g[nm + "_le"]), nm


@pytest.mark.parametrize("name", ["cornell", "zoo", "mesh2k", "cornell_env", "cornell_uniform", "cornell_env_power"])
def test_render_images(name, gx):
    g = golden("render.npz")
    W, H, spp, depth = (int(v) for v in g[name + "_cfg"])
    if name in ("cornell", "cornell_uniform"):
        b = scenes.cornell()
    elif name == "zoo":
        b = scenes.material_zoo()
    elif name == "mesh2k":
        b = _scene("mesh2k")
    else:
        b = scenes.cornell(sky=True)
        b.AddInfLight(os.path.join(GOLDEN, "env_100x50.hdr"))
    integ = gx.PathIntegrator(depth, 1.0, {"cornell_uniform": "uniform", "cornell_env_power": "power"}.get(name, "spatial"))
    img, st = ol.OracleScene(b).render(integ, W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])


@pytest.mark.parametrize("name", ["vol_synth", "vol_cfg5"])
def test_volpath_images(name, gx):
    """VolPathIntegrator::Li + GridDensityMedium / HomogeneousMedium / HenyeyGreenstein (cfg 5): the restated loop
    running on the reference's own Medium, BSDF, Light and BVH classes produced these images and ray counts."""
    g = golden("render_vol.npz")
    W, H, spp, depth = (int(v) for v in g[name + "_cfg"])
    b = scenes.volume_cornell(sigma_a=(0.5,) * 3, sigma_s=(3.5,) * 3, g_grid=0.3) if name == "vol_synth" else scenes.volume_cornell_cfg5(0.05)
    ol.olib().gnxo_max_dimension(1)
    img, st = ol.OracleScene(b).render(gx.VolPathIntegrator(depth, 1.0, "spatial"), W, H, spp)
    assert ol.olib().gnxo_max_dimension(1) < 1000       # beyond this the reference indexes PrimeSums out of bounds
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])


@pytest.mark.parametrize("name", ["cornell", "zoo", "cfg1"])
def test_whitted_images(name, gx):
    """WhittedIntegrator::Li + SpecularReflect / SpecularTransmit (cfg 1): the restated recursion running on
    the reference's own classes produced these images, ray counts and the full-size cfg 1 checksum."""
    g = golden("render_whitted.npz")
    if name == "cfg1":
        img, st = ol.OracleScene(scenes.cornell()).render(gx.WhittedIntegrator(5), 256, 256, 16)
        # the complete reference traced 1 048 576 closest-hit / 2 028 213 any-hit rays for cfg 1
        assert (st["rays_closest"], st["rays_any"]) == (1048576, 2028213) == tuple(int(v) for v in g["cfg1_rays"])
        assert abs(float(img[..., :3].astype(np.float64).sum()) - float(g["cfg1_checksum"])) < 1e-6
        assert biteq(img[::4, ::4, :3], g["cfg1_thumb"])
        return
    W, H, spp, depth = (int(v) for v in g[name + "_cfg"])
    b = scenes.cornell() if name == "cornell" else scenes.material_zoo()
    img, st = ol.OracleScene(b).render(gx.WhittedIntegrator(depth), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

@pytest.mark.parametrize("name", ["cornell_all", "cornell_one", "zoo_all", "zoo_one"])
def test_direct_lighting_images(name, gx):
    """DirectLightingIntegrator::Li with UniformSampleAllLights (Sampler::Request2DArray / Get2DArray sample arrays, nSamples = 5
    per area light, Get2D fallback once the arrays are used up) and UniformSampleOneLight: the restated integrator running on the
    reference's own Sampler, BSDF, Light and BVH classes produced these images and ray counts (oracle/ref_driver.cpp refDirectLi)."""
    g = golden("render_direct.npz")
    W, H, spp, depth = (int(v) for v in g[name + "_cfg"])
    scene, strat = name.split("_")
    b = scenes.cornell() if scene == "cornell" else scenes.material_zoo()
    ol.olib().gnxo_max_dimension(1)
    img, st = ol.OracleScene(b).render(gx.DirectLightingIntegrator(strat, depth), W, H, spp)
    assert ol.olib().gnxo_max_dimension(1) < 1000
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

def _textured_integrator(gx, name, depth):
    return {"path": lambda: gx.PathIntegrator(depth, 1.0, "spatial"), "whitted": lambda: gx.WhittedIntegrator(depth),
            "direct_all": lambda: gx.DirectLightingIntegrator("all", depth), "volpath": lambda: gx.VolPathIntegrator(depth, 1.0, "spatial")}[name]()


@pytest.mark.parametrize("name", ["path", "whitted", "direct_all", "volpath"])
def test_textured_images(name, gx):
    """ImageTexture / UVMapping2D / MIPMap (Lanczos resample of the 96x80 image, pyramid, EWA and trilinear filters,
    Repeat / Clamp wrap, gamma, scale) behind Plastic (the reference's getSmileFacePlasticMaterial) and Matte, with the camera ray
    differentials, ComputeDifferentials and -- Whitted / DirectLighting -- their propagation through a mirror and a glass sheet.
    The reference's own ImageTexture, MIPMap, camera and Interaction code produced these images and ray counts; its PathIntegrator
    slices the RayDifferential (`Ray ray(r)`), so Path looks every texture up unfiltered, which the fixture also pins."""
    g = golden("render_textured.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    b = scenes.textured_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr"))
    img, st = ol.OracleScene(b).render(_textured_integrator(gx, name, depth), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

@pytest.mark.parametrize("name", ["path", "whitted", "direct_one", "volpath"])
def test_textured_uv_images(name, gx):
    """TriangleMesh::uv (per-vertex uvs, Triangle::GetUVs / the dpdu-dpdv block of Triangle::Intersect): a poster mapped with the
    whole image, a Disney panel whose uvs run past 1 and a panel with coinciding uvs (the degenerate-uv fallback to
    CoordinateSystem(ng)); the uvs also set the shading frame of every lobe.  Images and ray counts of the reference's classes."""
    g = golden("render_textured_uv.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    b = scenes.textured_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr"), uv_quads=True)
    integ = gx.DirectLightingIntegrator("one", depth) if name == "direct_one" else _textured_integrator(gx, name, depth)
    img, st = ol.OracleScene(b).render(integ, W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

@pytest.mark.parametrize("name", ["path", "whitted", "direct_all", "volpath"])
def test_smooth_normal_images(name, gx):
    """TriangleMesh::n (per-vertex shading normals, the shading-geometry block of Triangle::Intersect, shape/Triangle.cpp:228-297):
    interpolated normal, (ss, ts) frame, dndu / dndv, geometric normal flipped onto the shading side -- on a mirror ball, a glass
    ball, a textured ball with uvs, a non-uniformly scaled Disney ellipsoid and a medium container.  The reference's classes."""
    g = golden("render_smooth.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    b = scenes.smooth_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr"))
    img, st = ol.OracleScene(b).render(_textured_integrator(gx, name, depth), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

def test_texture_filter_sweep():
    """ImageTexture::Evaluate / MIPMap::Lookup of the compiled reference over EWA and trilinear x Repeat / Black / Clamp x images of
    16x16, 64x4, 5x3, 33x17 and 1x1 texels x five footprint sizes (scenes.TEXTURE_FILTER_QUADS, oracle/make_goldens.py
    texture_filter_goldens): the oracle reproduces every record bit for bit, through gnxo_bsdf_probe_diff given the offset rays the
    reference's driver builds from its float diffEps.  tests/test_texture_filter.py counts which branches these probes take."""
    g = golden("texture_filter.npz")
    rays, wi, u, out = g["rays"], g["wi"], g["u"], g["out"]
    assert out.dtype == np.float32 and out.shape == (len(rays), len(g["eps"]), 16) and len(g["eps"]) == 5
    osc = ol.OracleScene(scenes.texture_filter_scene("sweep"))
    for k, eps in enumerate(g["eps"]):
        o = osc.bsdf_probe_diff(rays, wi, u, scenes.synthetic_differentials(rays, eps), 31)
        assert o.shape == out[:, k].shape and biteq(o, out[:, k]), float(eps)
        assert (out[:, k, 13] == 1).mean() >= 0.25
    # the footprints matter: the five eps values give five different answers on most valid probes
    valid = out[:, 0, 13] == 1
    assert (np.array([len(np.unique(out[i, :, 0:3].view(np.uint32), axis=0)) for i in np.nonzero(valid)[0]]) >= 3).mean() > 0.5


DELTA_CASES = ["path_spatial", "path_power", "path_uniform", "whitted", "direct_all", "direct_one", "volpath"]


def _delta_integrator(gx, name, depth):
    return {"path_spatial": lambda: gx.PathIntegrator(depth, 1.0, "spatial"), "path_power": lambda: gx.PathIntegrator(depth, 1.0, "power"),
            "path_uniform": lambda: gx.PathIntegrator(depth, 1.0, "uniform"), "whitted": lambda: gx.WhittedIntegrator(depth),
            "direct_all": lambda: gx.DirectLightingIntegrator("all", depth), "direct_one": lambda: gx.DirectLightingIntegrator("one", depth),
            "volpath": lambda: gx.VolPathIntegrator(depth, 1.0, "spatial")}[name]()


@pytest.mark.parametrize("name", DELTA_CASES)
def test_delta_light_images(name, gx):
    """PointLight / SpotLight / DistantLight (the reference's AddSpotLight / AddDistLight, ui/ModelList.cpp:149-161, plus a point
    light): Sample_Li, Power, DistantLight::Preprocess, the IsDeltaLight branches of EstimateDirect with and without media, the
    spatial / power / uniform light distributions over a mix of delta and area lights.  Images and ray counts of the reference's own
    light classes under the restated integrators."""
    g = golden("render_delta.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    img, st = ol.OracleScene(scenes.delta_cornell()).render(_delta_integrator(gx, name, depth), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

def _ortho_scene():
    b = scenes.textured_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr"))
    b.set_camera(eye=(0.2, 0.1, 5.0), look=(0.0, -0.2, 0.0), orthographic=True)
    return b


@pytest.mark.parametrize("name", ["path", "whitted", "volpath"])
def test_orthographic_camera_images(name, gx):
    """OrthographicCamera::GenerateRayDifferential (camera/Orthographic.cpp:36-92) as CreateOrthographicCamera builds it, on the
    textured scene (the offset rays feed the texture filters under Whitted / VolPath): the reference's camera class."""
    g = golden("render_ortho.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    img, st = ol.OracleScene(_ortho_scene()).render(_textured_integrator(gx, name, depth), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name])

def _hlbvh_scene(name):
    b = scenes.smooth_cornell(os.path.join(GOLDEN, "tex_smile_96x80.hdr")) if name == "smooth" else \
        scenes.dragon_cornell(2000, "glass+metal", mesh_path=os.path.join(GOLDEN, "mesh_2k.3d"))
    b.set_bvh_split_method({"middle": "middle", "equal": "equal_counts"}.get(name, "hlbvh"))   # the other BVHAccel::SplitMethod values ride along
    return b


@pytest.mark.parametrize("name", ["mesh2k", "smooth", "middle", "equal"])
def test_oracle_traverses_the_reference_hlbvh_tree(name, gx):
    """BVHAccel(prims, 1, SplitMethod::HLBVH) of the compiled reference, dumped as LinearBVHNode[] + primitive order: the oracle
    traverses that tree (it does not restate the HLBVH builder) and reproduces the image and ray counts the reference rendered
    through it.  The product's own HLBVH build is compared with the same dump in tests/test_gpu_parity.py."""
    g = golden("bvh_hlbvh.npz")
    W, H, spp, depth = (int(v) for v in g["cfg"])
    osc = ol.OracleScene(_hlbvh_scene(name))
    osc.set_bvh(g[name + "_bounds"], g[name + "_meta"], g[name + "_order"])
    img, st = osc.render(gx.PathIntegrator(depth, 1.0, "spatial"), W, H, spp)
    assert (st["rays_closest"], st["rays_any"]) == tuple(int(v) for v in g[name + "_rays"])
    assert biteq(img, g[name + "_img"])


def test_cfg2_reproduces_the_recorded_reference_run(gx):
    """the complete reference traced 16 058 662 closest-hit and 12 329 468 any-hit rays
    for cfg 2 and its image summed to 78538.576918.  This pins the restated Render / Li / EstimateDirect /
    SpatialLightDistribution loop, the one part of the path that cannot be compiled here (it needs Qt)."""
    g = golden("cfg2_recorded.npz")
    img, st = ol.OracleScene(scenes.cornell()).render(gx.PathIntegrator(8, 1.0, "spatial"), 256, 256, 64)
    assert (st["rays_closest"], st["rays_any"]) == (16058662, 12329468) == tuple(int(v) for v in g["rays"])
    assert abs(float(img[..., :3].astype(np.float64).sum()) - 78538.576918) < 1e-5
    assert biteq(img[::4, ::4, :3], g["thumb"])
