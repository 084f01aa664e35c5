"""Checks on the reference's own Resources/ inputs, against what the compiled reference returned for them.  They pin BASELINE
config 4's inputs at their own size: the reference's Resources/MonValley1000.hdr (1000 x 500, run-length encoded) through the
builder's RGBE reader, the 1000x500 -> 1024x512 Lanczos resample + Distribution2D of InfiniteAreaLight, and Plastic / Disney /
Glass / Metal lit by it -- oracle against the reference's own classes, bit for bit.  The inputs are data fixtures under
tests/golden/ (xz / bz2 copies of the Resources/ files; TropicalRuins1000.hdr as two valid files of 250 scanlines each, scanline
bytes untouched), the reference's answers are recorded in tests/golden/reference_assets.npz (stbi_loadf's floats and the larger
images as SHA-256 of their bits); oracle/make_goldens.py section 18 made both."""
import bz2
import hashlib
import lzma
import os

import numpy as np
import pytest

import oracle_lib as ol
import scenes
from conftest import GOLDEN


def _rec():
    return np.load(os.path.join(GOLDEN, "reference_assets.npz"))


def _fixture(name, tmp_path):
    """tests/golden/<name>.xz / .bz2 unpacked into tmp_path: the path of the file as the reference had it."""
    src = os.path.join(GOLDEN, name)
    dst = str(tmp_path / os.path.basename(name).rsplit(".", 1)[0])
    with (lzma.open if name.endswith(".xz") else bz2.open)(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    return dst


def _sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def _builder_pixels(gx, path):
    b = gx.SceneBuilder()
    b.AddInfLight(path)
    d = b.desc()
    return np.ctypeslib.as_array(d.env_rgb, shape=(d.env_height, d.env_width, 3)).copy()


@pytest.mark.parametrize("name", ["MonValley1000.hdr", "TropicalRuins1000.hdr"])
def test_rgbe_reader_equals_stbi_on_the_reference_hdr(gx, name, tmp_path):
    """The reference's own environment maps are new-style RLE Radiance files: the RLE branch of read_rgbe
    (csrc/scene_builder.cpp) must return stbi_loadf's floats (3rd/stb_image.h, as lights/InfiniteAreaLight.cpp:27 calls it)
    bit for bit."""
    rec = _rec()
    if os.path.exists(os.path.join(GOLDEN, name + ".xz")):
        mine = _builder_pixels(gx, _fixture(name + ".xz", tmp_path))
    else:   # stored as two files of 250 scanlines each: the rows of the whole file, in order
        mine = np.concatenate([_builder_pixels(gx, _fixture(f"{name[:-4]}_part{i}.hdr.xz", tmp_path)) for i in (0, 1)])
    assert mine.shape == tuple(rec["stbi_shape_" + name]) == (500, 1000, 3)
    assert _sha256(mine) == str(rec["stbi_sha256_" + name])


def test_rgbe_reader_equals_stbi_on_the_synthetic_stand_in(gx, tmp_path):
    """bench.py --workload cfg4 and the 1080p GPU test use a synthetic 1000 x 500 map written RLE-encoded by tests/scenes.py
    (the file as scenes.write_rgbe wrote it is the fixture)."""
    mine = _builder_pixels(gx, _fixture("synthetic_env_1000x500.hdr.xz", tmp_path))
    assert mine.shape == (500, 1000, 3)
    assert _sha256(mine) == str(_rec()["stbi_sha256_synthetic"])


@pytest.mark.parametrize("strategy", ["spatial", "power"])
def test_oracle_equals_reference_classes_under_the_reference_hdr(gx, strategy, tmp_path):
    """cfg 4 at a size the CPU finishes in seconds: 2 k-triangle mesh in Glass / Metal / Plastic / Disney quarters inside the
    Cornell box, InfiniteAreaLight(MonValley1000.hdr) with the transform of ui/ModelList.cpp:172-179 -- the oracle against the
    restated Render / Li loop on the reference's own InfiniteAreaLight, MIPMap, Distribution2D, BSDF and BVH classes."""
    env = _fixture("MonValley1000.hdr.xz", tmp_path)
    b = scenes.dragon_cornell(2000, "zoo", env=env, mesh_path=os.path.join(GOLDEN, "mesh_2k.3d"))
    W, H, spp, depth = 96, 54, 4, 8
    integ = gx.PathIntegrator(depth, 1.0, strategy)
    oimg, ost = ol.OracleScene(b).render(integ, W, H, spp)
    rec = _rec()
    rimg, cnt = rec[f"env_{strategy}_img"], rec[f"env_{strategy}_rays"]
    assert rimg.shape == (H, W, 3)
    assert (int(cnt[0]), int(cnt[1])) == (ost["rays_closest"], ost["rays_any"])
    assert (oimg[..., :3].view(np.uint32) == rimg.view(np.uint32)).all()
    assert oimg[..., :3].max() > 0.5   # the environment actually lights the scene


def test_volume_reader_on_the_reference_density_file(gx, tmp_path):
    """Resources/density_render.70.volume (100 x 100 x 40, CRLF) through gnxr_builder_add_volume_file: header and all 400 000
    densities equal the committed data fixture tests/golden/density_70.npz (which cfg 5's goldens were rendered from)."""
    g = np.load(os.path.join(GOLDEN, "density_70.npz"))
    b = gx.SceneBuilder()
    m = b.add_volume_file(_fixture("density_render.70.volume.bz2", tmp_path))
    d = b.desc()
    md = d.media[m]
    assert (md.nx, md.ny, md.nz) == (int(g["nx"]), int(g["ny"]), int(g["nz"])) == (100, 100, 40)
    assert list(md.sigma_a) == [10.0] * 3 and list(md.sigma_s) == [90.0] * 3
    got = np.ctypeslib.as_array(d.grid_density, shape=(100 * 100 * 40,))
    assert (got.view(np.uint32) == g["density"].reshape(-1).astype(np.float32).view(np.uint32)).all()


def _ref_render(key):
    """The reference's render of a test below, as recorded: SHA-256 of its image bits (rgb, float32) and its two ray counts."""
    rec = _rec()
    cnt = rec[key + "_rays"]
    return str(rec[key + "_sha256"]), (int(cnt[0]), int(cnt[1]))


def test_volpath_at_config_size_oracle_equals_reference_classes(gx):
    """cfg 5's geometry at cfg 5's image size (512 x 512; 2 spp of HaltonSampler(2), sigma scaled by 0.05 so that no sample passes
    Halton dimension 1000, where the reference is undefined): the two restatements of VolPathIntegrator::Li
    (integrators/VolPathIntegrator.cpp:24-159) -- the oracle's and ref_driver.cpp's on the reference's own GridDensityMedium /
    HomogeneousMedium / HenyeyGreenstein / BVH / light classes -- agree bit for bit, ray counts included.  The 64 x 64 fixture
    (render_vol.npz) pins the same pair at fixture size; this closes the gap up to the configuration's own size."""
    b = scenes.volume_cornell_cfg5(0.05, golden_dir=GOLDEN)
    W, H, spp, depth = 512, 512, 2, 8
    ol.olib().gnxo_max_dimension(1)
    oimg, ost = ol.OracleScene(b).render(gx.VolPathIntegrator(depth, 1.0, "spatial"), W, H, spp, threads=8)
    assert ol.olib().gnxo_max_dimension(1) < 1000
    rsha, rrays = _ref_render("vol512")   # ref_driver render args [W, H, spp, depth, 1.0, 0, 8, 1]
    assert rrays == (ost["rays_closest"], ost["rays_any"])
    assert _sha256(oimg[..., :3]) == rsha
    assert rrays[0] > 2 * W * H   # media segments make several closest-hit rays per camera sample


def test_direct_lighting_all_at_256_oracle_equals_reference_classes(gx):
    """DirectLightingIntegrator, UniformSampleAll, on the one-of-each-material scene at 256 x 256 (integrators/
    DirectLightingIntegrator.cpp:30-64 + the sample arrays of core/Sampler.cpp:52-72): oracle == the restatement on the reference's
    Sampler / BSDF / light / BVH classes, bit for bit -- four times the linear size of the render_direct.npz fixture."""
    b = scenes.material_zoo()
    W, H, spp, depth = 256, 256, 4, 5
    oimg, ost = ol.OracleScene(b).render(gx.DirectLightingIntegrator("all", depth), W, H, spp, threads=8)
    rsha, rrays = _ref_render("direct256")   # ref_driver render args [W, H, spp, depth, 1.0, 0, 8, 3, 0]
    assert rrays == (ost["rays_closest"], ost["rays_any"])
    assert _sha256(oimg[..., :3]) == rsha
