"""Scene set-ups of BASELINE.json's configs, authored through the product's SceneBuilder
(the mirror of ui/ModelList.cpp / ui/MaterialList.cpp / ui/RenderThread.cpp:46-187)."""
import os
import tempfile

import numpy as np

import gnxraytracer_amd as gx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# seeded synthetic inputs (stand-in mesh, environment map) are written once and reused from here; build/ is not versioned
CACHE_DIR = os.path.join(ROOT, "build", "synthetic_inputs")


def synthetic_cache_dir():
    """CACHE_DIR when this user may write there; otherwise (a tree built by another user, or read-only) a directory of this user's
    own under the system temporary directory.  The files are seeded, so either place holds the same bytes."""
    own = os.path.join(tempfile.gettempdir(), f"gnxr_synthetic_inputs_{os.getuid()}")
    for d in (CACHE_DIR, own):
        try:
            os.makedirs(d, exist_ok=True)
        except OSError:
            continue
        if os.access(d, os.W_OK | os.X_OK) and (d == CACHE_DIR or os.stat(d).st_uid == os.getuid()):
            return d
    raise RuntimeError(f"no writable directory for the synthetic scene inputs ({CACHE_DIR}, {own})")


WHITE = (0.91, 0.91, 0.91)
RED = (0.9, 0.1, 0.17)
BLUE = (0.14, 0.21, 0.87)
DRAGON_GREEN = (0.2, 0.8, 0.2)


def cornell(light_material="white", sky=False):
    """cfg 1/2: Cornell box, 10 wall triangles + 2 light triangles, Matte sigma=60 (RenderThread.cpp:79-133)."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    red = b.MatteMaterial(RED, 60.0)
    blue = b.MatteMaterial(BLUE, 60.0)
    b.AddCornell(red, blue, white)
    lm = white if light_material == "white" else b.MatteMaterial(DRAGON_GREEN, 60.0)
    b.AddAreaLight(lm)
    if sky:
        b.AddSkyLight()
    return b


def material_zoo():
    """Cornell box whose walls carry one of each material (function-level BSDF parity)."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    lambert = b.MatteMaterial(RED, 0.0)
    mirror = b.MirrorMaterial(DRAGON_GREEN)
    glass = b.getWhiteGlassMaterial()
    metal = b.getYelloMetalMaterial()
    plastic = b.getPurplePlasticMaterial()
    sglass = b.add_material(type=gx._abi.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0)
    disney = disney_preset(b)
    first = b.AddCornell(lambert, mirror, white)
    # floor: glass / smooth glass, ceiling: metal / plastic, back wall (tris 4,5): disney
    d = b.desc()
    mats = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
    mats[first + 0] = glass
    mats[first + 1] = sglass
    mats[first + 2] = metal
    mats[first + 3] = plastic
    mats[first + 4] = disney
    mats[first + 5] = disney_thin_preset(b)
    b.AddAreaLight(white)
    return b


def disney_preset(b):
    """Build-defined Disney preset for cfg 4 (the reference never instantiates DisneyMaterial)."""
    return b.DisneyMaterial(color=(0.8, 0.45, 0.2), metallic=0.3, eta=1.5, roughness=0.4, specularTint=0.2, anisotropic=0.3,
                            sheen=0.5, sheenTint=0.5, clearcoat=0.6, clearcoatGloss=0.8, specTrans=0.25, thin=False,
                            flatness=0.0, diffTrans=0.0)


def disney_thin_preset(b):
    return b.DisneyMaterial(color=(0.3, 0.6, 0.8), metallic=0.0, eta=1.4, roughness=0.5, specularTint=0.0, anisotropic=0.0,
                            sheen=0.0, sheenTint=0.5, clearcoat=0.0, clearcoatGloss=1.0, specTrans=0.4, thin=True,
                            flatness=0.3, diffTrans=0.8)


def synthetic_mesh_path(n_tris, seed=1, cache_dir=None):
    cache_dir = cache_dir or synthetic_cache_dir()
    os.makedirs(cache_dir, exist_ok=True)
    p = os.path.join(cache_dir, f"synthetic_dragon_{n_tris}_{seed}.3d")
    if not os.path.exists(p):
        tmp = p + f".{os.getpid()}.tmp"
        gx.write_synthetic_3d(tmp, n_tris, seed)
        os.replace(tmp, p)
    return p


def write_rgbe(path, rgb, rle=True):
    """Radiance .hdr writer (32-bit_rle_rgbe).  rle=True writes the new-style run-length-encoded scanlines every Radiance tool
    (and the reference's Resources/*.hdr) uses -- the branch of the builder's reader that stbi's hdr loader calls
    `stbi__hdr_load` RLE -- rle=False the flat layout.  Data only: no reference file is copied."""
    rgb = np.asarray(rgb, np.float64)
    h, w, _ = rgb.shape
    m = rgb.max(axis=2)
    ok = m > 1e-32
    mant, ex = np.frexp(np.where(ok, m, 1.0))           # m = mant * 2^ex, mant in [0.5, 1)
    scale = np.where(ok, mant * 256.0 / np.where(ok, m, 1.0), 0)
    px = np.zeros((h, w, 4), np.uint8)
    px[..., :3] = np.clip(rgb * scale[..., None], 0, 255).astype(np.uint8)
    px[..., 3] = np.where(ok, ex + 128, 0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        if not rle or w < 8 or w >= 32768:
            f.write(px.tobytes())
            return
        for j in range(h):
            out = bytearray([2, 2, (w >> 8) & 0xff, w & 0xff])
            for c in range(4):
                line = px[j, :, c]
                # run boundaries, then greedy: runs of >= 4 equal bytes become (128 + n, value), the rest literal blocks of <= 128
                edges = np.flatnonzero(np.diff(line)) + 1
                starts = np.concatenate([[0], edges]); ends = np.concatenate([edges, [w]])
                lit_start = 0
                def flush_lit(a, b):
                    while a < b:
                        n = min(128, b - a)
                        out.append(n); out.extend(line[a:a + n].tobytes()); a += n
                for a, b in zip(starts.tolist(), ends.tolist()):
                    if b - a >= 4:
                        flush_lit(lit_start, a)
                        v = int(line[a])
                        while a < b:
                            n = min(127, b - a)
                            out.append(128 + n); out.append(v); a += n
                        lit_start = b
                flush_lit(lit_start, w)
            f.write(bytes(out))


def synthetic_env(w=1000, h=500, seed=4):
    """Deterministic outdoor-style lat-long radiance map at the size of the reference's Resources/MonValley1000.hdr (1000 x 500:
    not a power of two, so MIPMap's Lanczos resample to 1024 x 512 runs): graded sky, a small bright sun (the importance table must
    find it; peak 200, MonValley's is 69), ground, a few soft clouds.  Stand-in for the HDR, which cannot travel to the GPU box."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (xx + 0.5) / w, (yy + 0.5) / h
    sky = np.stack([0.25 + 0.5 * v, 0.45 + 0.45 * v, 1.05 - 0.25 * v], 2) * (1.3 - 0.6 * v[..., None])
    ground = np.stack([0.22 + 0.05 * np.sin(40 * u), 0.19 + 0.04 * np.cos(31 * u), 0.12 + 0.0 * u], 2) * (0.6 + 0.8 * (v[..., None] - 0.5))
    img = np.where((v > 0.52)[..., None], ground, sky)
    rng = np.random.default_rng(seed)
    for _ in range(7):   # clouds
        cu, cv, r = rng.random(), 0.1 + 0.3 * rng.random(), 0.03 + 0.06 * rng.random()
        du = np.minimum(np.abs(u - cu), 1 - np.abs(u - cu))
        img += 0.9 * np.exp(-((du / (2 * r)) ** 2 + ((v - cv) / r) ** 2))[..., None] * (v < 0.5)[..., None]
    su, sv = 0.31, 0.22   # the sun: ~3 texels wide, two orders of magnitude above the sky
    img += (2.0e2 * np.exp(-(((u - su) * w) ** 2 + ((v - sv) * h) ** 2) / 4.0))[..., None] * np.array([1.0, 0.93, 0.82])
    img[h - 6:, :, :] = 0.0   # a black band (RGBE exponent 0: the `e == 0` branch of the decoder) with long runs
    return img.astype(np.float32)


def synthetic_env_path(w=1000, h=500, cache_dir=None):
    cache_dir = cache_dir or synthetic_cache_dir()
    os.makedirs(cache_dir, exist_ok=True)
    p = os.path.join(cache_dir, f"synthetic_env_{w}x{h}.hdr")
    if not os.path.exists(p):
        tmp = p + f".{os.getpid()}.tmp"
        write_rgbe(tmp, synthetic_env(w, h), rle=True)
        os.replace(tmp, p)
    return p


def dragon_cornell(n_tris=100000, material="glass", env=None, extra_materials=False, mesh_path=None):
    """cfg 3 (Glass + Metal halves) / cfg 4 (+ InfiniteAreaLight, Plastic, Disney).  The mesh is the seeded
    synthetic stand-in for the absent dragon.3d; AddModel comes first, as in RenderThread.cpp:119-133."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    red = b.MatteMaterial(RED, 60.0)
    blue = b.MatteMaterial(BLUE, 60.0)
    glass = b.getWhiteGlassMaterial()
    metal = b.getYelloMetalMaterial()
    path = mesh_path or synthetic_mesh_path(n_tris)
    first = b.AddModel(path, glass)
    d = b.desc()
    nt = d.n_triangles
    mats = np.ctypeslib.as_array(d.tri_material, shape=(nt,))
    if material == "glass+metal":
        mats[first + nt // 2:first + nt] = metal          # build-defined split: second half of the faces
    elif material == "metal":
        mats[first:first + nt] = metal
    elif material == "zoo":
        plastic = b.getPurplePlasticMaterial()
        dis = disney_preset(b)
        q = nt // 4
        mats[first + q:first + 2 * q] = metal
        mats[first + 2 * q:first + 3 * q] = plastic
        mats[first + 3 * q:first + nt] = dis
    b.AddCornell(red, blue, white)
    b.AddAreaLight(white)
    if env:
        b.AddInfLight(env)
    return b


def random_rays(n, seed=0, inside=2.4, tmax=np.inf):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-inside, inside, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return gx.make_rays(o, d.astype(np.float32), tmax)


def box_mesh(lo, hi):
    """12 triangles with outward geometric normals (n = Cross(p0-p2, p1-p2), shape/Triangle.cpp:223)."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], np.float32)
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]   # -z +z -y +y +x -x, CCW from outside
    idx = []
    for a, b, c, d in quads:
        idx += [[a, b, c], [a, c, d]]
    return v, np.array(idx, np.int32)


def synthetic_density(nx=24, ny=24, nz=12, seed=3):
    """Smooth seeded smoke-like density in [0, 1] (stand-in for Resources/density_render.70.volume in tests)."""
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float32)
    x, y, z = (x + 0.5) / nx, (y + 0.5) / ny, (z + 0.5) / nz
    rng = np.random.default_rng(seed)
    d = np.zeros_like(x)
    for _ in range(5):
        c = rng.random(3)
        r = 0.15 + 0.2 * rng.random()
        d += np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (r * r))
    d = (d / d.max()).astype(np.float32)
    return np.ascontiguousarray(d)   # [nz, ny, nx]: density[(z*ny + y)*nx + x], GridDensityMedium.h:34-38


def read_volume_file(path):
    """Resources/density_render.70.volume: `nx N ny N nz N / p0 / p1 / sigma_a / sigma_s` then nx*ny*nz floats (CRLF)."""
    toks = open(path).read().split()
    nx, ny, nz = int(toks[1]), int(toks[3]), int(toks[5])
    p0 = [float(t) for t in toks[7:10]]
    p1 = [float(t) for t in toks[11:14]]
    sa = [float(t) for t in toks[15:18]]
    ss = [float(t) for t in toks[19:22]]
    d = np.array(toks[22:22 + nx * ny * nz], np.float32)
    return dict(nx=nx, ny=ny, nz=nz, p0=p0, p1=p1, sigma_a=sa, sigma_s=ss, density=d)


def volume_cornell(density=None, sigma_a=(10, 10, 10), sigma_s=(90, 90, 90), g_grid=0.0, grid_lo=(-1.6, -2.4, -1.2), grid_hi=(0.2, -0.6, 0.4)):
    """cfg 5: Cornell + a null-material box filled with a GridDensityMedium + a second null-material box with the
    HomogeneousMedium(2.4, 1.4, 0.5) of ui/RenderThread.cpp:107.  mediumToWorld = Translate(lo) * Scale(hi - lo)."""
    b = cornell()
    if density is None:
        density = synthetic_density()
    nz, ny, nx = density.shape
    lo, hi = np.array(grid_lo, np.float32), np.array(grid_hi, np.float32)
    m2w = np.eye(4, dtype=np.float32)
    m2w[0, 0], m2w[1, 1], m2w[2, 2] = hi - lo
    m2w[0:3, 3] = lo
    grid = gx.Medium()
    grid.type = gx._abi.MEDIUM_GRID
    grid.nx, grid.ny, grid.nz = nx, ny, nz
    grid.sigma_a[:] = sigma_a
    grid.sigma_s[:] = sigma_s
    grid.g = g_grid
    grid.medium_to_world[:] = m2w.reshape(16)
    mg = b.add_medium(grid, density)
    hom = gx.Medium()
    hom.type = gx._abi.MEDIUM_HOMOGENEOUS
    hom.sigma_a[:] = (2.4, 2.4, 2.4)
    hom.sigma_s[:] = (1.4, 1.4, 1.4)
    hom.g = 0.5
    mh = b.add_medium(hom)
    v, i = box_mesh(grid_lo, grid_hi)
    b.add_mesh(v, i, -1, medium_inside=mg, medium_outside=-1)
    v, i = box_mesh((0.6, -2.4, -0.8), (1.9, -0.9, 0.6))
    b.add_mesh(v, i, -1, medium_inside=mh, medium_outside=-1)
    return b


def reference_density(golden_dir=None):
    """The reference's own density grid (Resources/density_render.70.volume, 100x100x40), kept as a data fixture."""
    g = np.load(os.path.join(golden_dir or os.path.join(ROOT, "tests", "golden"), "density_70.npz"))
    return np.ascontiguousarray(g["density"].reshape(int(g["nz"]), int(g["ny"]), int(g["nx"])))


def volume_cornell_cfg5(sigma_scale=1.0, golden_dir=None):
    """cfg 5 with the reference's density grid (sigma_a 10, sigma_s 90 from the file header) in a 2 x 2 x 0.8 box.
    sigma_scale < 1 keeps the delta-tracking loops below Halton dimension 1000, past which the reference reads
    PrimeSums out of bounds (undefined there; this build wraps, device_sampler.h)."""
    return volume_cornell(reference_density(golden_dir), sigma_a=(10 * sigma_scale,) * 3, sigma_s=(90 * sigma_scale,) * 3,
                          grid_lo=(-1.9, -2.4, -0.4), grid_hi=(0.1, -0.4, 0.4))


def cornell_sphere(kind="matte", center=(0.6, -1.5, 0.2), radius=1.0):
    """cfg 1 as BASELINE.json words it ("6 quads + 1 Sphere"): the Cornell box plus one pbrt-v3 sphere (the reference's own
    Sphere is an unfinished stub -- parity unpinned, see include/gnxr.h).  kind: matte | mirror | glass | medium."""
    b = cornell()
    if kind == "matte":
        m = b.MatteMaterial(DRAGON_GREEN, 60.0)
    elif kind == "mirror":
        m = b.MirrorMaterial((0.9, 0.9, 0.9))
    elif kind == "glass":
        m = b.add_material(type=gx._abi.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0)
    else:
        m = -1
    mi = -1
    if kind == "medium":
        hom = gx.Medium()
        hom.type = gx._abi.MEDIUM_HOMOGENEOUS
        hom.sigma_a[:] = (0.4, 0.8, 1.2)
        hom.sigma_s[:] = (2.0, 1.6, 1.2)
        hom.g = 0.3
        mi = b.add_medium(hom)
    b.AddSphere(center, radius, m, medium_inside=mi, medium_outside=-1)
    return b


def cornell_no_lights():
    """walls only: scene.lights is empty (UniformSampleOneLight returns 0, Integrator.cpp:63; Whitted's light loop is empty)."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    b.AddCornell(b.MatteMaterial(RED, 60.0), b.MatteMaterial(BLUE, 60.0), white)
    return b


def cornell_in_fog():
    """the camera sits inside a thin HomogeneousMedium bounded by a large null-material box (Camera::medium != nullptr)."""
    b = cornell()
    hom = gx.Medium()
    hom.type = gx._abi.MEDIUM_HOMOGENEOUS
    hom.sigma_a[:] = (0.02, 0.03, 0.04)
    hom.sigma_s[:] = (0.10, 0.08, 0.06)
    hom.g = -0.2
    m = b.add_medium(hom)
    v, i = box_mesh((-6.0, -6.0, -6.0), (6.0, 6.0, 8.0))
    b.add_mesh(v, i, -1, medium_inside=m, medium_outside=-1)
    b.set_camera_medium(m)
    return b


def textured_cornell(tex_path, glass_sheet=True, uv_quads=False):
    """image-textured materials.  Back wall = the reference's getSmileFacePlasticMaterial (ui/MaterialList.cpp:31-46:
    Kd = Ks = one ImageTexture, EWA, Repeat) on `tex_path`; floor = Matte whose Kd is the same image tiled 3 x 3 through the
    trilinear filter with Clamp wrap, gamma and scale; left wall = mirror and a free-standing smooth-glass sheet so that Whitted /
    DirectLighting carry ray differentials through specular reflection and transmission onto the textures.  Triangles have no
    per-vertex uv in the reference, so every triangle shows the lower-right half of the image (Triangle::GetUVs defaults)."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    blue = b.MatteMaterial(BLUE, 60.0)
    mirror = b.MirrorMaterial((0.9, 0.9, 0.9))
    smile = b.getSmileFacePlasticMaterial(tex_path)
    floor_tex = b.add_image_texture(tex_path, su=3.0, sv=3.0, du=0.25, dv=0.1, trilinear=True, wrap="clamp", scale=0.8, gamma=True)
    floor = b.MatteMaterial(WHITE, 0.0)
    b.set_material_texture(floor, "kd", floor_tex)
    first = b.AddCornell(mirror, blue, white)
    d = b.desc()
    mats = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
    mats[first + 0] = floor
    mats[first + 1] = floor
    mats[first + 4] = smile
    mats[first + 5] = smile
    if glass_sheet:
        sglass = b.add_material(type=gx._abi.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0)
        v = np.array([[0.3, -2.5, 0.4], [1.9, -2.5, -0.6], [1.9, 0.4, -0.6], [0.3, 0.4, 0.4]], np.float32)
        b.add_mesh(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), sglass)
    if uv_quads:
        # meshes WITH per-vertex uv (TriangleMesh::uv): a poster showing the whole image once, a Disney-coated panel whose uvs
        # run to 2.5 (Repeat) -- uv also sets dpdu / dpdv and with them the shading frame of every lobe --, and a panel whose
        # three uvs coincide (degenerate: Triangle::Intersect falls back to CoordinateSystem(ng))
        quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        poster = np.array([[-2.0, -1.0, -2.2], [-0.2, -1.0, -2.3], [-0.2, 0.9, -2.3], [-2.0, 0.9, -2.2]], np.float32)
        b.add_mesh(poster, quad, smile, uv=[[0, 0], [1, 0], [1, 1], [0, 1]])
        panel = np.array([[0.9, -2.45, 1.2], [2.3, -2.45, 0.2], [2.3, -1.2, 0.0], [0.9, -1.2, 1.0]], np.float32)
        b.add_mesh(panel, quad, disney_preset(b), uv=[[0.25, 0.5], [2.5, 0.5], [2.5, 1.75], [0.25, 1.75]])
        flat = np.array([[-2.4, -2.4, 0.5], [-1.2, -2.4, 1.2], [-1.2, -1.5, 1.2], [-2.4, -1.5, 0.5]], np.float32)
        b.add_mesh(flat, quad, floor, uv=[[0.4, 0.6]] * 4)
    b.AddAreaLight(white)
    return b


def uv_sphere_mesh(center, radius, n_lat=8, n_lon=12):
    """Lat-long tessellated sphere with per-vertex uvs (phi / 2pi, theta / pi) and object-space normals (p - center) / r."""
    c = np.asarray(center, np.float64)
    verts, uvs, normals = [], [], []
    for i in range(n_lat + 1):
        th = np.pi * i / n_lat
        for j in range(n_lon + 1):
            ph = 2 * np.pi * j / n_lon
            n = np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
            verts.append(c + radius * n); normals.append(n); uvs.append([j / n_lon, i / n_lat])
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * (n_lon + 1) + j, (i + 1) * (n_lon + 1) + j
            if i > 0: tris.append([a, b, a + 1])
            if i < n_lat - 1: tris.append([a + 1, b, b + 1])
    return np.array(verts, np.float32), np.array(tris, np.int32), np.array(uvs, np.float32), np.array(normals, np.float32)


def smooth_cornell(tex_path, medium_ball=True):
    """Per-vertex shading normals (TriangleMesh::n): coarse lat-long spheres that are smooth-shaded -- a mirror ball and a glass ball
    (the interpolated normal drives the specular directions, dndu / dndv the ray differentials of Whitted / DirectLighting, and the
    geometric normal is flipped onto the shading side, which the glass's etaScale and the medium interface read), a ball with normals
    AND uvs carrying the image-textured plastic, a scaled (non-uniform object-to-world) Disney ellipsoid, and -- for VolPath -- a
    null-material ball with normals around a HomogeneousMedium."""
    b = gx.SceneBuilder()
    white = b.MatteMaterial(WHITE, 60.0)
    red = b.MatteMaterial(RED, 60.0)
    blue = b.MatteMaterial(BLUE, 60.0)
    mirror = b.MirrorMaterial((0.9, 0.9, 0.9))
    sglass = b.add_material(type=gx._abi.MAT_GLASS, kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0), urough=0.0, vrough=0.0)
    smile = b.getSmileFacePlasticMaterial(tex_path)
    b.AddCornell(red, blue, white)
    v, t, uv, n = uv_sphere_mesh((-1.3, -1.6, -0.6), 0.85)
    b.add_mesh(v, t, mirror, normals=n)
    v, t, uv, n = uv_sphere_mesh((1.2, -1.5, 0.6), 0.9, 6, 9)
    b.add_mesh(v, t, sglass, normals=n)
    v, t, uv, n = uv_sphere_mesh((0.0, 0.3, -1.3), 0.8, 7, 10)
    b.add_mesh(v, t, smile, uv=uv, normals=n)
    v, t, uv, n = uv_sphere_mesh((0.0, 0.0, 0.0), 1.0, 6, 8)
    m = np.array([[0.7, 0, 0, 1.4], [0, 0.35, 0, 0.9], [0, 0, 0.5, -0.8], [0, 0, 0, 1]], np.float32)
    # per-vertex tangents (TriangleMesh::s) along the parallels; they vanish at the poles (the `ss.LengthSquared() > 0` fallback)
    tang = np.stack([-n[:, 2], np.zeros(len(n), np.float32), n[:, 0]], 1).astype(np.float32)
    b.add_mesh(v, t, disney_preset(b), object_to_world=m, uv=uv, normals=n, tangents=tang)
    # tangents WITHOUT normals (`mesh->n || mesh->s`): a flat-shaded metal panel whose anisotropic frame follows the given tangents
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    panel = np.array([[-2.3, -2.45, 1.9], [-1.1, -2.45, 1.9], [-1.1, -2.1, 0.9], [-2.3, -2.1, 0.9]], np.float32)
    aniso = b.add_material(type=gx._abi.MAT_METAL, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), urough=0.05, vrough=0.3, remap_roughness=1)
    b.add_mesh(panel, quad, aniso, tangents=[[1, 0, 0.4], [0.8, 0, 0.6], [0.6, 0.1, 0.8], [0.9, 0, 0.3]])
    if medium_ball:
        hom = gx.Medium()
        hom.type = gx._abi.MEDIUM_HOMOGENEOUS
        hom.sigma_a[:] = (0.4, 0.5, 0.9)
        hom.sigma_s[:] = (1.6, 1.4, 0.8)
        hom.g = 0.3
        med = b.add_medium(hom)
        v, t, uv, n = uv_sphere_mesh((-0.3, -1.9, 1.4), 0.55, 6, 8)
        b.add_mesh(v, t, -1, medium_inside=med, medium_outside=-1, normals=n)
    b.AddAreaLight(white)
    return b


def delta_cornell(medium_ball=True):
    """Delta lights (EstimateDirect's IsDeltaLight branch, core/Integrator.cpp:157-158, 168): the reference's AddSpotLight and
    AddDistLight (ui/ModelList.cpp:149-161; their calls are commented out in RenderThread.cpp:138-141) plus a PointLight, next to the
    area light, in the material zoo -- and a HomogeneousMedium ball so that VolPath's handleMedia = true variant takes the branch too."""
    b = material_zoo()
    b.AddSpotLight()
    b.AddDistLight()
    b.add_delta_light("point", (6.0, 4.0, 2.5), light_to_world=[[1, 0, 0, -1.2], [0, 1, 0, -0.4], [0, 0, 1, 1.1], [0, 0, 0, 1]])
    b.add_delta_light("spot", (30.0, 30.0, 40.0), total_width=35.0, falloff_start=10.0,
                      light_to_world=[[0.8, 0, 0.6, 1.9], [0, 1, 0, 1.7], [-0.6, 0, 0.8, 2.0], [0, 0, 0, 1]])
    if medium_ball:
        hom = gx.Medium()
        hom.type = gx._abi.MEDIUM_HOMOGENEOUS
        hom.sigma_a[:] = (0.3, 0.4, 0.6)
        hom.sigma_s[:] = (1.2, 1.0, 0.7)
        hom.g = 0.2
        med = b.add_medium(hom)
        v, t, uv, n = uv_sphere_mesh((0.2, -1.4, 0.9), 0.7, 6, 8)
        b.add_mesh(v, t, -1, medium_inside=med, medium_outside=-1)
    return b


# ---------------------------------------------------------------- the texture-filter sweep (tests/test_texture_filter.py)
# images of the sweep, tests/golden/tex_filter_<name>.hdr (written by oracle/make_goldens.py texture_filter_goldens): (w, h)
TEXTURE_FILTER_IMAGES = {"16x16": (16, 16), "64x4": (64, 4), "5x3": (5, 3), "33x17": (33, 17), "1x1": (1, 1)}
UV_UNIT, UV_WIDE = (0.0, 1.0), (-1.5, 2.5)
# one flat quad per row, each with a material of its own: Matte (sigma 0: f = Kd / pi shows the texture value) whose Kd is the image
# texture `kd`; `ks` makes it a Plastic with a second texture.  uv: the range both coordinates run over across the quad.  half: half the
# edge length; "tiny" is so small under so many uv repeats that dpdu / dpdv give SolveLinearSystem2x2 a determinant below 1e-10.
TEXTURE_FILTER_QUADS = [
    dict(name="ewa_repeat", uv=UV_WIDE, kd=dict(image="16x16", wrap="repeat", max_aniso=8.0)),
    dict(name="ewa_black", uv=UV_WIDE, kd=dict(image="16x16", wrap="black", max_aniso=8.0)),
    dict(name="ewa_clamp", uv=UV_WIDE, kd=dict(image="33x17", wrap="clamp", max_aniso=8.0)),
    dict(name="ewa_repeat_aniso1", uv=UV_WIDE, kd=dict(image="64x4", wrap="repeat", max_aniso=1.0)),
    dict(name="ewa_repeat_aniso16", uv=UV_UNIT, kd=dict(image="33x17", wrap="repeat", max_aniso=16.0)),
    dict(name="tri_repeat", uv=UV_WIDE, kd=dict(image="64x4", wrap="repeat", trilinear=True)),
    dict(name="tri_black", uv=UV_WIDE, kd=dict(image="33x17", wrap="black", trilinear=True)),
    dict(name="tri_clamp", uv=UV_WIDE, kd=dict(image="16x16", wrap="clamp", trilinear=True)),
    dict(name="ewa_mapped", uv=UV_UNIT, kd=dict(image="16x16", wrap="repeat", max_aniso=8.0, su=7.0, sv=0.5, du=-3.25, dv=-0.75)),
    dict(name="tri_gamma_scale", uv=UV_WIDE, kd=dict(image="5x3", wrap="clamp", trilinear=True, gamma=True, scale=0.8)),
    dict(name="ewa_black_5x3", uv=UV_UNIT, kd=dict(image="5x3", wrap="black", max_aniso=8.0)),
    dict(name="ewa_1x1", uv=UV_UNIT, kd=dict(image="1x1", wrap="repeat", max_aniso=8.0)),
    dict(name="tri_black_1x1", uv=UV_WIDE, kd=dict(image="1x1", wrap="black", trilinear=True)),
    dict(name="plastic", uv=UV_WIDE, kd=dict(image="64x4", wrap="clamp", max_aniso=8.0), ks=dict(image="5x3", wrap="repeat", trilinear=True)),
    dict(name="tiny", uv=(0.0, 1000.0), half=0.002, kd=dict(image="16x16", wrap="repeat", max_aniso=8.0)),
]
# (e1, e2) of the quads, taken in turn: the normal e1 x e2 runs along z, x and y (the three axis pairs of ComputeDifferentials) and
# along two tilted directions
_TF_FRAMES = [((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0)), ((0.8, 0.0, -0.6), (0.36, 0.8, 0.48)), ((0.0, 0.6, 0.8), (1.0, 0.0, 0.0))]
TEXTURE_FILTER_UPDATED_QUAD = 0   # case "updated": this quad's texture is the 33x17 image under Clamp instead of 16x16 under Repeat
TEXTURE_FILTER_UPDATED = dict(image="33x17", wrap="clamp", max_aniso=8.0)


def texture_filter_image_path(name, golden_dir=None):
    return os.path.join(golden_dir or os.path.join(ROOT, "tests", "golden"), f"tex_filter_{name}.hdr")


def texture_filter_quad(i):
    """(centre, e1, e2, half, (uv_lo, uv_hi)) of quad i: the quads lie 12 units apart along x, far enough that a probe ray, which
    starts within 1.5 units of its target, meets no other quad first"""
    q = TEXTURE_FILTER_QUADS[i]
    e1, e2 = (np.array(v, np.float64) for v in _TF_FRAMES[i % len(_TF_FRAMES)])
    return np.array([12.0 * i, 0.0, 0.0]), e1, e2, float(q.get("half", 1.0)), q["uv"]


def texture_filter_scene(case="sweep", golden_dir=None):
    """The scene of the texture-filter sweep: TEXTURE_FILTER_QUADS, no lights (the probes evaluate BSDFs only).  case "sweep" is what
    the reference fixture was recorded on; "updated" is the same scene with the texture of quad TEXTURE_FILTER_UPDATED_QUAD replaced,
    what Scene.update_textures must turn a "sweep" scene into.  Texture i of quad j is texture_filter_texture_index(j)."""
    assert case in ("sweep", "updated"), case
    b = gx.SceneBuilder()
    for i, q in enumerate(TEXTURE_FILTER_QUADS):
        c, e1, e2, half, (lo, hi) = texture_filter_quad(i)
        kd = dict(TEXTURE_FILTER_UPDATED if case == "updated" and i == TEXTURE_FILTER_UPDATED_QUAD else q["kd"])
        t = b.add_image_texture(texture_filter_image_path(kd.pop("image"), golden_dir), **kd)
        if "ks" in q:
            ks = dict(q["ks"])
            m = b.add_material(type=gx._abi.MAT_PLASTIC, kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), urough=0.1, remap_roughness=1)
            b.set_material_texture(m, "ks", b.add_image_texture(texture_filter_image_path(ks.pop("image"), golden_dir), **ks))
        else:
            m = b.MatteMaterial(WHITE, 0.0)
        b.set_material_texture(m, "kd", t)
        v = np.array([c - half * e1 - half * e2, c + half * e1 - half * e2, c + half * e1 + half * e2, c - half * e1 + half * e2], np.float32)
        b.add_mesh(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), m, uv=[[lo, lo], [hi, lo], [hi, hi], [lo, hi]])
    return b


def texture_filter_texture_index(quad):
    """index of quad `quad`'s Kd texture in the scene's texture list (a Plastic quad adds two)"""
    return quad + sum(1 for q in TEXTURE_FILTER_QUADS[:quad] if "ks" in q)


TEXTURE_FILTER_COSINES = (1.0, 0.5, 0.1, 0.02)


def texture_filter_probes(quad, n, seed, n_miss=0):
    """n + n_miss BSDF probes built for quad `quad`: (rays, wi, u).  Each of the first n rays is aimed at a seeded uv target -- half of
    them uniform over the quad, half within one texel of an image border (st = 0 or 1 in u, in v or in both, where the quad's uv range
    reaches it) -- from 1 to 1.5 units away, under an incidence cosine from TEXTURE_FILTER_COSINES (the grazing ones stretch the
    footprint) at a seeded azimuth; a quarter arrives from behind the quad.  wi lies on the side of wo, so that the Lambert lobe
    shows Kd, and takes one of four directions, u one of four samples: the sampling columns of the results then repeat.  The last
    n_miss rays point away from the quad and hit nothing."""
    rng = np.random.default_rng([20261019, seed, quad])
    q = TEXTURE_FILTER_QUADS[quad]
    c, e1, e2, half, (lo, hi) = texture_filter_quad(quad)
    nrm = np.cross(e1, e2)
    kd = q["kd"]
    w, h = TEXTURE_FILTER_IMAGES[kd["image"]]
    su, sv, du, dv = kd.get("su", 1.0), kd.get("sv", 1.0), kd.get("du", 0.0), kd.get("dv", 0.0)
    m = n + n_miss
    uv = rng.uniform(lo, hi, (m, 2))
    mode = rng.integers(0, 6, m)          # 0-2: uniform; 3: a border in u; 4: in v; 5: in both
    for axis, (s_, d_, res) in enumerate(((su, du, w), (sv, dv, h))):
        near = (mode == 3 + axis) | (mode == 5)
        st = np.floor(s_ * uv[:, axis] + d_) + rng.integers(0, 2, m) + rng.uniform(-1.0, 1.0, m) / res   # a border of the tile the target lay in
        cand = (st - d_) / s_
        ok = near & (cand > lo) & (cand < hi)
        uv[ok, axis] = cand[ok]
    pad = 1e-3 * (hi - lo)
    uv = np.clip(uv, lo + pad, hi - pad)
    a = (uv - lo) / (hi - lo) * 2.0 - 1.0
    p = c + half * (a[:, 0:1] * e1 + a[:, 1:2] * e2)
    cos = np.array(TEXTURE_FILTER_COSINES)[rng.integers(0, 4, m)]
    phi = rng.uniform(0, 2 * np.pi, m)
    side = np.where(rng.integers(0, 4, m) == 0, -1.0, 1.0)
    sin = np.sqrt(1.0 - cos * cos)
    wo = side[:, None] * cos[:, None] * nrm + sin[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    dist = rng.uniform(1.0, 1.5, m)
    o = p + wo * dist[:, None]
    d = -wo
    d[n:] = wo[n:]                        # the misses leave the quad behind them
    rays = gx.make_rays(o.astype(np.float32), d.astype(np.float32), np.inf)
    k = rng.integers(0, 4, m)
    ct, ph = np.array([0.9, 0.6, 0.3, 0.75])[k], np.array([0.3, 2.0, 4.1, 5.5])[k]
    stt = np.sqrt(1.0 - ct * ct)
    wi = side[:, None] * ct[:, None] * nrm + stt[:, None] * (np.cos(ph)[:, None] * e1 + np.sin(ph)[:, None] * e2)
    u = np.array([[0.12, 0.7], [0.55, 0.31], [0.83, 0.9], [0.4, 0.05]], np.float32)[rng.integers(0, 4, m)]
    return rays, np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(u, np.float32)


def synthetic_differentials(rays, eps):
    """the offset rays oracle/ref_driver.cpp's `bsdf` command builds for diffEps = eps: rx / ryOrigin = o, rxDirection = d + (eps, 0, 0),
    ryDirection = d + (0, eps, 0), in float32: (n, 12) rows for Scene.bsdf(differentials=) and OracleScene.bsdf_probe_diff"""
    eps = np.float32(eps)
    o, d = rays[:, 0:3], rays[:, 4:7]
    rxd, ryd = d.copy(), d.copy()
    rxd[:, 0] = d[:, 0] + eps
    ryd[:, 1] = d[:, 1] + eps
    return np.ascontiguousarray(np.concatenate([o, rxd, o, ryd], 1), np.float32)


# ---------------------------------------------------------------- the material grid (tests/test_material_grid.py, test_shading_queries.py)
# One record per branch of the material compiler (compile_material, csrc/scene_compile.cpp): which lobes a material has, its shade class
# and which narrow kernel shades it all depend on its parameters.  `rec` holds the fields of gnxr_material that differ from a blank
# record; every Disney entry after "disney_preset" is written as its differences from that preset.
def _grid(name, family, **rec):
    return dict(name=name, family=family, rec=rec)


_GRID_KD = (0.5, 0.4, 0.3)
_GRID_BLACK = (0.0, 0.0, 0.0)
_GRID_METAL = dict(eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2))
_GRID_GLASS = dict(kr=(0.98,) * 3, kt=(0.98,) * 3, eta=(1.5, 0, 0))
_PURPLE = tuple(float(np.float32(v)) for v in (0.35, 0.12, 0.48))
_GRID_PLASTIC = dict(kd=_PURPLE, ks=tuple(float(np.float32(1) - np.float32(v)) for v in _PURPLE), urough=0.1, vrough=0.1, remap_roughness=1)
DISNEY_PRESET = dict(kd=(0.8, 0.45, 0.2), eta=(1.5, 0, 0), disney_metallic=0.3, disney_roughness=0.4, disney_spec_tint=0.2, disney_anisotropic=0.3,
                     disney_sheen=0.5, disney_sheen_tint=0.5, disney_clearcoat=0.6, disney_clearcoat_gloss=0.8, disney_spec_trans=0.25,
                     disney_thin=0, disney_flatness=0.0, disney_diff_trans=0.0)


def _matte(name, kd, sigma):
    return _grid(name, "matte", kd=kd, sigma=sigma)


def _glass(name, urough=0.0, vrough=0.0, remap=0, **kw):
    return _grid(name, "glass", **{**_GRID_GLASS, **kw, "urough": urough, "vrough": vrough, "remap_roughness": remap})


def _metal(name, urough, vrough, remap, **kw):
    return _grid(name, "metal", **{**_GRID_METAL, **kw, "urough": urough, "vrough": vrough, "remap_roughness": remap})


def _plastic(name, **kw):
    return _grid(name, "plastic", **{**_GRID_PLASTIC, **kw})


def _disney(name, **diff):
    return _grid(name, "disney", **{**DISNEY_PRESET, **diff})


MATERIAL_GRID = [
    # Matte: sigma == 0 is Lambert, anything else Oren-Nayar; sigma is clamped to [0, 90]; a black Kd drops the lobe; Kd is clamped at 0 only
    _matte("matte_sigma0", _GRID_KD, 0.0), _matte("matte_sigma1", _GRID_KD, 1.0), _matte("matte_sigma90", _GRID_KD, 90.0),
    _matte("matte_sigma200", _GRID_KD, 200.0), _matte("matte_sigma_neg", _GRID_KD, -5.0), _matte("matte_black", _GRID_BLACK, 20.0),
    _matte("matte_kd_clamped", (-1.0, 0.4, 2.0), 0.0),
    _grid("mirror_black", "mirror", kr=_GRID_BLACK), _grid("mirror_bright", "mirror", kr=(0.9, 0.5, 1.5)),
    # Glass: urough == vrough == 0 is specular, anything else microfacet; black Kr / Kt drop lobes; RoughnessToAlpha(0) under remap
    _glass("glass_smooth"), _glass("glass_smooth_t", kr=_GRID_BLACK), _glass("glass_smooth_r", kt=_GRID_BLACK),
    _glass("glass_black_rough", 0.1, 0.1, kr=_GRID_BLACK, kt=_GRID_BLACK), _glass("glass_smooth_eta1", eta=(1.0, 0, 0)),
    _glass("glass_rough_eta1", 0.2, 0.2, 1, eta=(1.0, 0, 0)), _glass("glass_rough_eta07", 0.2, 0.05, 1, eta=(0.7, 0, 0)),
    _glass("glass_u0_remap", 0.0, 0.3, 1), _glass("glass_u0", 0.0, 0.3, 0), _glass("glass_rough1_remap", 1.0, 1.0, 1),
    _glass("glass_rough_t_eta24", 0.01, 0.5, 0, kr=_GRID_BLACK, eta=(2.4, 0, 0)), _glass("glass_rough_r", 0.1, 0.1, 0, kt=_GRID_BLACK),
    # Metal: one conductor microfacet lobe whatever the parameters; the alpha clamp at 0.001, anisotropy, k == 0, eta == 1
    _metal("metal_001_remap", 0.01, 0.01, 1), _metal("metal_0_remap", 0.0, 0.0, 1), _metal("metal_0", 0.0, 0.0, 0),
    _metal("metal_aniso", 1.0, 0.001, 0), _metal("metal_k0", 0.15, 0.15, 0, k=_GRID_BLACK),
    _metal("metal_eta1_k0", 0.15, 0.15, 0, eta=(1.0, 1.0, 1.0), k=_GRID_BLACK), _metal("metal_2_05_remap", 2.0, 0.5, 1),
    # Plastic: a Lambert lobe (Kd) and a dielectric microfacet lobe (Ks, Fresnel etaI 1.5 / etaT 1), each dropped when black
    _plastic("plastic_purple"), _plastic("plastic_black_kd", kd=_GRID_BLACK, remap_roughness=0), _plastic("plastic_black_ks", ks=_GRID_BLACK),
    _plastic("plastic_black", kd=_GRID_BLACK, ks=_GRID_BLACK), _plastic("plastic_u0_remap", urough=0.0, vrough=0.0),
    _plastic("plastic_u0", urough=0.0, vrough=0.0, remap_roughness=0), _plastic("plastic_u1_remap", urough=1.0, vrough=1.0),
    _disney("disney_preset"), _disney("disney_metallic1", disney_metallic=1.0), _disney("disney_opaque", disney_metallic=0.0, disney_spec_trans=0.0),
    _disney("disney_spectrans1", disney_spec_trans=1.0), _disney("disney_metallic1_spectrans1", disney_metallic=1.0, disney_spec_trans=1.0),
    _disney("disney_clearcoat0", disney_clearcoat=0.0), _disney("disney_sheen0", disney_sheen=0.0),
    _disney("disney_clearcoat1_gloss0", disney_clearcoat=1.0, disney_clearcoat_gloss=0.0), _disney("disney_gloss1", disney_clearcoat_gloss=1.0),
    _disney("disney_rough0", disney_roughness=0.0), _disney("disney_rough1", disney_roughness=1.0),
    _disney("disney_rough001_aniso1", disney_roughness=0.01, disney_anisotropic=1.0), _disney("disney_aniso1", disney_anisotropic=1.0),
    _disney("disney_aniso0", disney_anisotropic=0.0), _disney("disney_black", kd=_GRID_BLACK),
    _disney("disney_black_tints1", kd=_GRID_BLACK, disney_spec_tint=1.0, disney_sheen=1.0, disney_sheen_tint=1.0),
    _disney("disney_eta1", eta=(1.0, 0, 0)), _disney("disney_eta1_spectrans08", eta=(1.0, 0, 0), disney_spec_trans=0.8),
    _disney("disney_spectint1_sheentint0", disney_spec_tint=1.0, disney_sheen_tint=0.0),
    _disney("disney_thin", disney_thin=1, disney_flatness=0.3, disney_diff_trans=0.8, disney_spec_trans=0.4),
    _disney("disney_thin_flat1_difftrans2", disney_thin=1, disney_flatness=1.0, disney_diff_trans=2.0),
    _disney("disney_thin_plain", disney_thin=1, disney_spec_trans=0.0, disney_diff_trans=0.0, disney_flatness=0.0),
    _disney("disney_thin_trans1", disney_thin=1, disney_spec_trans=1.0, disney_diff_trans=1.0),
    _disney("disney_thin_metallic1", disney_thin=1, disney_metallic=1.0, disney_diff_trans=1.0),
    _disney("disney_thin_eta1", disney_thin=1, eta=(1.0, 0, 0), disney_spec_trans=0.5, disney_roughness=0.3),
    _disney("disney_thin_eta05", disney_thin=1, eta=(0.5, 0, 0), disney_spec_trans=0.5, disney_roughness=0.3),
    _disney("disney_sheen2_clearcoat2", disney_sheen=2.0, disney_clearcoat=2.0),
]
MATERIAL_GRID_NAMES = [g["name"] for g in MATERIAL_GRID]
_GRID_TYPES = {"matte": "MAT_MATTE", "mirror": "MAT_MIRROR", "glass": "MAT_GLASS", "metal": "MAT_METAL", "plastic": "MAT_PLASTIC", "disney": "MAT_DISNEY"}


def grid_material(name):
    """the gnxr_material record of the grid entry `name` (for Scene.update_materials and descriptions with edited records)"""
    g = MATERIAL_GRID[MATERIAL_GRID_NAMES.index(name)]
    return gx.material(type=getattr(gx._abi, _GRID_TYPES[g["family"]]), has_bump=1, **g["rec"])   # has_bump = 1: as add_material sets it


def add_grid_material(b, name):
    g = MATERIAL_GRID[MATERIAL_GRID_NAMES.index(name)]
    return b.add_material(type=getattr(gx._abi, _GRID_TYPES[g["family"]]), **g["rec"])


def material_grid_quad(i):
    """(centre, e1, e2) of quad i: the layout of the texture-filter sweep (12 units apart along x, the frames of _TF_FRAMES in turn), edge 2"""
    e1, e2 = (np.array(v, np.float64) for v in _TF_FRAMES[i % len(_TF_FRAMES)])
    return np.array([12.0 * i, 0.0, 0.0]), e1, e2


def material_grid(names=None):
    """One flat 2 x 2 quad per entry of MATERIAL_GRID (or of `names`), material i on quad i, no lights: the probes evaluate BSDFs only."""
    b = gx.SceneBuilder()
    for i, name in enumerate(names or MATERIAL_GRID_NAMES):
        c, e1, e2 = material_grid_quad(i)
        v = np.array([c - e1 - e2, c + e1 - e2, c + e1 + e2, c - e1 + e2], np.float32)
        b.add_mesh(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), add_grid_material(b, name))
    return b


MATERIAL_GRID_COSINES = (1.0, 0.7, 0.3, 0.05, 0.002)
MATERIAL_GRID_JITTER = (0.0, 1e-3, 3e-2)
MATERIAL_GRID_U_EDGES = (0.0, 0.5, 1.0 - 2.0 ** -24)


def material_grid_probes(quad, n, seed):
    """n BSDF probes aimed at quad `quad`: (rays, wi, u).  Each ray is aimed at a seeded point of the quad from 1 to 1.5 units away under
    an incidence cosine from MATERIAL_GRID_COSINES (down to grazing) at a seeded azimuth; about 30 % arrive from behind.  A quarter of
    the wi are the mirror direction of wo and a quarter the straight-through direction -wo, each moved by a jitter from
    MATERIAL_GRID_JITTER (0: exactly there, where a low-roughness lobe has its peak), the rest random unit vectors.  u is random, with a
    tenth of the rows drawn from MATERIAL_GRID_U_EDGES squared (the edges of the sampling routines).  Built in float64, rounded once."""
    rng = np.random.default_rng([20261020, seed, quad])
    c, e1, e2 = material_grid_quad(quad)
    nrm = np.cross(e1, e2)
    a = rng.uniform(-0.9, 0.9, (n, 2))
    p = c + a[:, 0:1] * e1 + a[:, 1:2] * e2
    cos = np.array(MATERIAL_GRID_COSINES)[rng.integers(0, len(MATERIAL_GRID_COSINES), n)]
    phi = rng.uniform(0, 2 * np.pi, n)
    side = np.where(rng.random(n) < 0.3, -1.0, 1.0)
    sin = np.sqrt(1.0 - cos * cos)
    wo = side[:, None] * cos[:, None] * nrm + sin[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    o = p + wo * rng.uniform(1.0, 1.5, n)[:, None]
    rays = gx.make_rays(o.astype(np.float32), (-wo).astype(np.float32), np.inf)
    wi = rng.normal(size=(n, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    kind = rng.integers(0, 4, n)          # 0: mirror, 1: straight through, 2-3: random
    mirror = 2.0 * (wo @ nrm)[:, None] * nrm - wo
    jit = np.array(MATERIAL_GRID_JITTER)[rng.integers(0, len(MATERIAL_GRID_JITTER), n)][:, None] * rng.normal(size=(n, 3))
    aimed = np.where((kind == 0)[:, None], mirror, -wo) + jit
    aimed /= np.linalg.norm(aimed, axis=1, keepdims=True)
    wi = np.where((kind < 2)[:, None], aimed, wi)
    u = rng.random((n, 2))
    edge = rng.random(n) < 0.1
    u[edge] = np.array(MATERIAL_GRID_U_EDGES)[rng.integers(0, len(MATERIAL_GRID_U_EDGES), (int(edge.sum()), 2))]
    return rays, np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(u, np.float32)


# ---------------------------------------------------------------- the delta-light grid (light_delta.npz)
_DELTA_SPOT_XF = [[0.8, 0, 0.6, 1.9], [0, 1, 0, 1.7], [-0.6, 0, 0.8, 2.0], [0, 0, 0, 1]]          # a rotation about y, then a translation
_DELTA_POINT_XF = [[2.0, 0, 0, -1.2], [0, 2.0, 0, -0.4], [0, 0, 2.0, 1.1], [0, 0, 0, 1]]            # uniform scale
_DELTA_DIST_XF = [[0, -1.5, 0, 0.5], [1.5, 0, 0, -0.3], [0, 0, 1.5, 0.2], [0, 0, 0, 1]]             # scale, rotation about z, translation
DELTA_SPOT_CONES = [(35.0, 10.0), (35.0, 35.0), (35.0, 50.0), (90.0, 45.0), (120.0, 90.0), (180.0, 0.0), (0.5, 0.25), (45.0, 0.0), (0.0, 0.0)]
DELTA_SPOT_I = (30.0, 30.0, 40.0)
DELTA_GRID = ([dict(name="spot_%g_%g" % c, kind="spot", I=DELTA_SPOT_I, xf=_DELTA_SPOT_XF, total_width=c[0], falloff_start=c[1]) for c in DELTA_SPOT_CONES]
              + [dict(name="point_scaled", kind="point", I=(6.0, 4.0, 2.5), xf=_DELTA_POINT_XF),
                 dict(name="distant_unit", kind="distant", I=(3.0, 2.5, 2.0), xf=np.eye(4).tolist(), w_light=(0.0, 0.6, 0.8)),
                 dict(name="distant_scaled", kind="distant", I=(1.0, 2.0, 3.0), xf=_DELTA_DIST_XF, w_light=(1.0, -2.0, 0.5))])
DELTA_GRID_ANGLE_OFFSETS = (0.0, 1e-7, -1e-7, 1e-4, -1e-4, 1e-2, -1e-2)
DELTA_GRID_DISTANCES = (1e-3, 0.1, 1.0, 2.5, 100.0)


def delta_grid():
    """The Cornell box (its two area-light triangles are lights 0 and 1) plus the lights of DELTA_GRID: (builder, first light index)"""
    b = cornell()
    first = b.desc().n_lights
    for l in DELTA_GRID:
        b.add_delta_light(l["kind"], l["I"], light_to_world=l["xf"], total_width=l.get("total_width", 45.0), falloff_start=l.get("falloff_start", 30.0),
                          w_light=l.get("w_light", (0, 0, 1)))
    return b, first


def delta_grid_probes(k, n, seed):
    """n light probes for light k of DELTA_GRID: (refP, refN, u, wiQ).  The reference points lie at light_to_world(dist * dir): dir makes,
    with the light's axis +z, an angle of total_width, falloff_start, their mean, 0 or 1.5 x total_width, moved by an offset from
    DELTA_GRID_ANGLE_OFFSETS (so that records fall on both sides of every cone edge, at one ulp and further off); a fifth of the
    directions are random; dist is from DELTA_GRID_DISTANCES; about 1 % of the points are the light's position itself (light space 0).
    Built in float64, rounded once."""
    l = DELTA_GRID[k]
    rng = np.random.default_rng([20261021, seed, k])
    tw, fs = np.radians(l.get("total_width", 45.0)), np.radians(l.get("falloff_start", 30.0))
    theta = np.array([tw, fs, 0.5 * (tw + fs), 0.0, 1.5 * tw])[rng.integers(0, 5, n)] + np.array(DELTA_GRID_ANGLE_OFFSETS)[rng.integers(0, 7, n)]
    phi = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], 1)
    rnd = rng.normal(size=(n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    d = np.where((rng.random(n) < 0.2)[:, None], rnd, d)
    dist = np.array(DELTA_GRID_DISTANCES)[rng.integers(0, len(DELTA_GRID_DISTANCES), n)]
    local = d * dist[:, None]
    local[rng.random(n) < 0.01] = 0.0
    xf = np.array(l["xf"], np.float64)
    scale = np.linalg.norm(xf[:3, 0])            # the scaled transforms are uniform: a distance in light space grows by it
    p = (local / scale) @ xf[:3, :3].T + np.array(l["xf"], np.float32).astype(np.float64)[:3, 3]
    shared = np.random.default_rng([20261021, seed])     # a delta light reads none of these three: one set serves every light
    nn, wq = shared.normal(size=(2, n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    wq /= np.linalg.norm(wq, axis=1, keepdims=True)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    return f32(p), f32(nn), f32(shared.random((n, 2))), f32(wq)


MATERIAL_GRID_FILES = {"bsdf_grid_basic.npz": ("matte", "mirror", "glass", "metal", "plastic"), "bsdf_grid_disney.npz": ("disney",)}
MATERIAL_GRID_FLAGS = (31, 15, 29)      # all lobes, no specular lobes, BSDF_REFLECTION only
MATERIAL_GRID_PROBES = 128              # per material
# Seed of the fixture's probes.  Two materials sit close to the floors tests/test_material_grid.py sets for an informative fixture: the
# eta = 1, k = 0 Metal reflects rounding residue only (f > 0 on 0.08 to 0.125 of 128 probes, depending on the seed; 0.094 of 4096) and the
# eta = 1 rough Glass returns NaN whenever it samples transmission (pdf > 0 on 0.41 to 0.55).  2 is the first seed at which the reference's
# numbers pass both floors.
MATERIAL_GRID_SEED = 2
DELTA_GRID_PROBES = 1024                # per light


def material_grid_golden(golden_dir=None):
    """The material-grid fixtures joined in the order of MATERIAL_GRID: rays, wi, u, material (the grid index of every probe) and
    out_<flags>, the compiled reference's 16 columns per probe."""
    parts = [np.load(os.path.join(golden_dir or os.path.join(ROOT, "tests", "golden"), f)) for f in MATERIAL_GRID_FILES]
    g = {k: np.concatenate([p[k] for p in parts]) for k in parts[0].files}
    order = np.argsort(g["material"], kind="stable")
    return {k: np.ascontiguousarray(v[order]) for k, v in g.items()}
