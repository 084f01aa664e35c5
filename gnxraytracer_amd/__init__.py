"""gnxraytracer_amd -- MI355X-native wavefront path-tracing core (host-side Python mirror).

This package is a thin ctypes layer over ``libgnxr.so`` (HIP kernels + C ABI, ``include/gnxr.h``).
Names follow the reference's authoring layer so that tests read like the reference's own scene
set-up (ui/ModelList.cpp, ui/MaterialList.cpp, ui/RenderThread.cpp:46-187):

    b = SceneBuilder()
    white = b.MatteMaterial((0.91, 0.91, 0.91), sigma=60)
    ...
    b.AddCornell(red, blue, white); b.AddAreaLight(white)
    scene = Scene(b)                                   # Scene(make_shared<BVHAccel>(prims, 1), lights)
    img, stats = PathIntegrator(8, rrThreshold=1.0).Render(scene, 256, 256, spp=64)

There is NO CPU fallback: every compute call goes through the HIP library and raises
``GnxrError`` if it (or a GPU) is missing.  The CPU restatement under ``oracle/`` is test
infrastructure and is never imported from here.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (Camera, Hit, Light, LiSample, Material, Medium, Ray, RenderParams, SceneDesc, Stats, Texture)  # noqa: F401
from ._tensors import (ANY_GPU, SOME, _addr, _arrays_on_device, _edit_stream, _expect, _got, _host_or_device, _image, _image_size, _is_tensor, _is_torch, _only_kw,  # noqa: F401
                       _out_tensor, _outputs, _ptr, _refuse, _same_count, _stream_handle, _stream_pair)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNXR_LIB", os.path.join(_HERE, "libgnxr.so"))   # GNXR_LIB: A/B builds during tuning


class GnxrError(RuntimeError):
    pass


_lib = None
_device = 0   # the device gnxr_init / the first device of gnxr_init_devices bound: scenes created afterwards live there


def lib():
    """Load libgnxr.so (built by ``__graft_entry__.build()``); fail loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GnxrError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = _abi.bind(C.CDLL(LIB_PATH))
        if _lib.gnxr_abi_version() != _abi.GNXR_ABI_VERSION:
            raise GnxrError("libgnxr.so ABI version mismatch")
    return _lib


def _check(rc):
    if rc < 0:
        raise GnxrError(f"gnxr error {rc}: {lib().gnxr_last_error().decode(errors='replace')}")
    return rc


def _walk_call(name, plain, counted, args, counts, n_counts, device, st):
    """The tail of the per-lane walk queries (closest_point, all_hits, within / nearest, sphere_cast): `plain(*args, stream)`, or, with
    `counts=` given -- it must be an int64 (n_counts,) tensor on `device` --, `counted(*args, counts, stream)`."""
    import torch
    if counts is None:
        return _check(plain(*args, _addr(st)))
    if not _is_tensor(counts, torch.int64, (n_counts,), device):
        _refuse(counts, f"{name}: counts must be a contiguous torch.int64 ({n_counts},) tensor on {device}")
    return _check(counted(*args, _ptr(counts), _addr(st)))


def _list_length(name, what, k, lowest, highest):
    """K of a query that keeps a list per record (`what`: its name in the messages): an integer in [lowest, highest]"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{name}: {what} must be an integer, got {type(k).__name__}")
    k = int(k)
    if not lowest <= k <= highest:
        raise ValueError(f"{name}: {what} must be in [{lowest}, {highest}], got {k}")
    return k


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


LIGHT_STRATEGIES = {"spatial": _abi.LIGHTS_SPATIAL, "uniform": _abi.LIGHTS_UNIFORM, "power": _abi.LIGHTS_POWER}   # lightSampleStrategy by name


def init(device_id=0):
    global _device
    _check(lib().gnxr_init(int(device_id)))
    _device = int(device_id)


def init_devices(device_ids):
    """One process, several devices: scenes created afterwards are replicated on all of them and Render() shards the image rows
    over them (gnxr_init_devices)."""
    global _device
    ids = (C.c_int32 * len(device_ids))(*[int(d) for d in device_ids])
    _check(lib().gnxr_init_devices(len(device_ids), ids))
    _device = int(device_ids[0])


class SceneBuilder:
    """Mirror of the scene-authoring free functions in ui/ModelList.cpp / ui/MaterialList.cpp."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().gnxr_builder_create(C.byref(self._h)))
        self.hdr_path = None

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.gnxr_builder_destroy(self._h)
            self._h = None

    # ---- materials (return a material index) ----
    def MatteMaterial(self, kd, sigma=60.0):          # ui/RenderThread.cpp:79-99
        return _check(lib().gnxr_builder_matte(self._h, _f3(kd), float(sigma)))

    def MirrorMaterial(self, kr):                     # ui/RenderThread.cpp:102
        return _check(lib().gnxr_builder_mirror(self._h, _f3(kr)))

    def getPurplePlasticMaterial(self):               # ui/MaterialList.cpp:48-56
        return _check(lib().gnxr_builder_purple_plastic(self._h))

    def getYelloMetalMaterial(self):                  # ui/MaterialList.cpp:58-69
        return _check(lib().gnxr_builder_yellow_metal(self._h))

    def getWhiteGlassMaterial(self):                  # ui/MaterialList.cpp:71-83
        return _check(lib().gnxr_builder_white_glass(self._h))

    def add_material(self, **kw):
        m = Material()
        m.has_bump = 1
        for k, v in kw.items():
            if isinstance(v, (tuple, list, np.ndarray)):
                setattr(m, k, (C.c_float * len(v))(*[float(x) for x in v]))
            else:
                setattr(m, k, v)
        return _check(lib().gnxr_builder_add_material(self._h, C.byref(m)))

    def DisneyMaterial(self, color, metallic=0.0, eta=1.5, roughness=0.5, specularTint=0.0, anisotropic=0.0, sheen=0.0,
                       sheenTint=0.5, clearcoat=0.0, clearcoatGloss=1.0, specTrans=0.0, thin=False, flatness=0.0,
                       diffTrans=1.0):                 # materials/DisneyMaterial.h:21-36
        return self.add_material(type=_abi.MAT_DISNEY, kd=color, eta=(eta, 0, 0), disney_metallic=metallic,
                                 disney_roughness=roughness, disney_spec_tint=specularTint,
                                 disney_anisotropic=anisotropic, disney_sheen=sheen, disney_sheen_tint=sheenTint,
                                 disney_clearcoat=clearcoat, disney_clearcoat_gloss=clearcoatGloss,
                                 disney_spec_trans=specTrans, disney_thin=int(thin), disney_flatness=flatness,
                                 disney_diff_trans=diffTrans)

    # ---- geometry / lights ----
    def AddModel(self, path, material):               # ui/ModelList.cpp:47-69
        return _check(lib().gnxr_builder_add_model_3d(self._h, os.fsencode(path), int(material)))

    def AddCornell(self, material1, material2, material3):   # ui/ModelList.cpp:71-118
        return _check(lib().gnxr_builder_add_cornell(self._h, int(material1), int(material2), int(material3)))

    def AddFloor(self, material):                     # ui/ModelList.cpp:20-45
        return _check(lib().gnxr_builder_add_floor(self._h, int(material)))

    def AddAreaLight(self, material):                 # ui/ModelList.cpp:120-147
        return _check(lib().gnxr_builder_add_area_light(self._h, int(material)))

    def AddSkyLight(self):                            # ui/ModelList.cpp:163-170
        return _check(lib().gnxr_builder_add_sky_light(self._h))

    def add_emissive_mesh(self, vertices, indices, material, lemit, n_samples=5, object_to_world=None):
        """AddAreaLight's pattern (ui/ModelList.cpp:137-146) for any mesh: one DiffuseAreaLight per triangle."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        m = None
        if object_to_world is not None:
            m = np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        return _check(lib().gnxr_builder_add_emissive_mesh(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), len(v), i.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           len(i), m, int(material), _f3(lemit), int(n_samples)))

    def AddSpotLight(self):                           # ui/ModelList.cpp:149-154 (the call is commented out in RenderThread.cpp:138)
        return _check(lib().gnxr_builder_add_spot_light(self._h))

    def AddDistLight(self):                           # ui/ModelList.cpp:156-161
        return _check(lib().gnxr_builder_add_dist_light(self._h))

    def add_delta_light(self, kind, I, light_to_world=None, total_width=45.0, falloff_start=30.0, w_light=(0, 0, 1)):
        """PointLight(LightToWorld, I) / SpotLight(LightToWorld, I, totalWidth, falloffStart) / DistantLight(LightToWorld, L, wLight)."""
        l = Light()
        l.type = {"point": _abi.LIGHT_POINT, "spot": _abi.LIGHT_SPOT, "distant": _abi.LIGHT_DISTANT}[kind]
        l.tri = -1
        l.n_samples = 1
        l.le[:] = [float(v) for v in I]
        l.radius = float(total_width)
        l.falloff_start = float(falloff_start)
        l.center[:] = [float(v) for v in w_light]
        m = np.eye(4, dtype=np.float32) if light_to_world is None else np.asarray(light_to_world, dtype=np.float32).reshape(4, 4)
        l.light_to_world[:] = [float(v) for v in m.reshape(16)]
        return _check(lib().gnxr_builder_add_light(self._h, C.byref(l)))

    def AddInfLight(self, hdr_path):                  # ui/ModelList.cpp:172-179
        self.hdr_path = str(hdr_path)
        return _check(lib().gnxr_builder_add_inf_light(self._h, os.fsencode(hdr_path)))

    def AddInfLightData(self, rgb, light_to_world=None, power=(1.0, 1.0, 1.0)):
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w = rgb.shape[:2]
        m = None
        if light_to_world is not None:
            m = np.ascontiguousarray(light_to_world, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        return _check(lib().gnxr_builder_add_inf_light_data(self._h, rgb.ctypes.data_as(C.POINTER(C.c_float)), w, h, m,
                                                            _f3(power)))

    def add_mesh(self, vertices, indices, material, object_to_world=None, medium_inside=-1, medium_outside=-1, uv=None, normals=None, tangents=None):
        """TriangleMesh(ObjectToWorld, nTriangles, vertexIndices, nVertices, P, S = nullptr, N = normals, UV = uv, ...): uv is the
        per-vertex (u, v) array of the mesh or None (Triangle::GetUVs defaults, what every mesh of the reference gets); normals the
        per-vertex object-space shading normals or None (flat shading)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        m = None
        if object_to_world is not None:
            m = np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        first = _check(lib().gnxr_builder_add_mesh(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), len(v),
                                                   i.ctypes.data_as(C.POINTER(C.c_int32)), len(i), m, int(material),
                                                   int(medium_inside), int(medium_outside)))
        if uv is not None:
            corner = np.ascontiguousarray(np.asarray(uv, dtype=np.float32).reshape(-1, 2)[i].reshape(-1, 6))
            _check(lib().gnxr_builder_set_triangle_uv(self._h, first, len(i), corner.ctypes.data_as(C.POINTER(C.c_float))))
        if normals is not None:
            n = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
            if object_to_world is not None:   # Transform::operator()(Normal3f): n' = (M^-1)^T n, evaluated in float like Transform.h:308-315
                minv = np.linalg.inv(np.asarray(object_to_world, dtype=np.float64).reshape(4, 4)).astype(np.float32)
                x, y, z = n[:, 0].copy(), n[:, 1].copy(), n[:, 2].copy()
                n = np.stack([minv[0, 0] * x + minv[1, 0] * y + minv[2, 0] * z, minv[0, 1] * x + minv[1, 1] * y + minv[2, 1] * z,
                              minv[0, 2] * x + minv[1, 2] * y + minv[2, 2] * z], 1).astype(np.float32)
            corner = np.ascontiguousarray(n[i].reshape(-1, 9))
            _check(lib().gnxr_builder_set_triangle_normals(self._h, first, len(i), corner.ctypes.data_as(C.POINTER(C.c_float))))
        if tangents is not None:   # TriangleMesh::s: s[i] = ObjectToWorld(S[i]), a plain vector transform (Triangle.cpp:49-52)
            t = np.asarray(tangents, dtype=np.float32).reshape(-1, 3)
            if object_to_world is not None:
                mm = np.asarray(object_to_world, dtype=np.float32).reshape(4, 4)
                x, y, z = t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()
                t = np.stack([mm[0, 0] * x + mm[0, 1] * y + mm[0, 2] * z, mm[1, 0] * x + mm[1, 1] * y + mm[1, 2] * z,
                              mm[2, 0] * x + mm[2, 1] * y + mm[2, 2] * z], 1).astype(np.float32)
            corner = np.ascontiguousarray(t[i].reshape(-1, 9))
            _check(lib().gnxr_builder_set_triangle_tangents(self._h, first, len(i), corner.ctypes.data_as(C.POINTER(C.c_float))))
        return first

    def add_medium(self, medium, density=None):
        d = None
        if density is not None:
            density = np.ascontiguousarray(density, dtype=np.float32)
            d = density.ctypes.data_as(C.POINTER(C.c_float))
        return _check(lib().gnxr_builder_add_medium(self._h, C.byref(medium), d))

    def add_volume_file(self, path, g=0.0, sigma_scale=1.0, medium_to_world=None):
        """GridDensityMedium from a `.volume` file (Resources/density_render.70.volume's format); returns the medium index."""
        m = None
        if medium_to_world is not None:
            m = np.ascontiguousarray(medium_to_world, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        return _check(lib().gnxr_builder_add_volume_file(self._h, os.fsencode(path), float(g), float(sigma_scale), m))

    def add_image_texture(self, image, su=1.0, sv=1.0, du=0.0, dv=0.0, trilinear=False, max_aniso=8.0, wrap="repeat", scale=1.0, gamma=False):
        """ImageTexture<RGBSpectrum, Spectrum>(UVMapping2D(su, sv, du, dv), file, doTrilinear, maxAniso, wrap, scale, gamma)
        (textures/ImageTexture.h; the defaults are those of getSmileFacePlasticMaterial, ui/MaterialList.cpp:31-46).  `image` is
        the path of a Radiance .hdr or an array [H, W, 3] of decoded texels (row 0 = top row, as stbi_loadf returns them)."""
        t = Texture(0, 0, 0, su, sv, du, dv, max_aniso, scale, int(bool(trilinear)), {"repeat": 0, "black": 1, "clamp": 2}[wrap], int(bool(gamma)), 0)
        if isinstance(image, (str, bytes, os.PathLike)):
            self.texture_paths = getattr(self, "texture_paths", []) + [str(image)]
            return _check(lib().gnxr_builder_add_texture_file(self._h, C.byref(t), os.fsencode(image)))
        rgb = np.ascontiguousarray(image, dtype=np.float32)
        self.texture_paths = getattr(self, "texture_paths", []) + [""]
        return _check(lib().gnxr_builder_add_texture_data(self._h, C.byref(t), rgb.ctypes.data_as(C.POINTER(C.c_float)), rgb.shape[1], rgb.shape[0]))

    def set_material_texture(self, material, slot, texture):
        """slot "kd" / "ks": replace the material's constant Kd / Ks texture by image texture `texture`."""
        return _check(lib().gnxr_builder_set_material_texture(self._h, int(material), {"kd": 0, "ks": 1}[slot], int(texture)))

    def getSmileFacePlasticMaterial(self, image):     # ui/MaterialList.cpp:31-46 (Kd = Ks = the same ImageTexture, roughness 0.1, remap)
        t = self.add_image_texture(image)
        m = self.add_material(type=_abi.MAT_PLASTIC, kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), urough=0.1, remap_roughness=1)
        self.set_material_texture(m, "kd", t)
        self.set_material_texture(m, "ks", t)
        return m

    def material_albedo(self, material):
        """gnxr_material_albedo of material `material` of this builder (see material_albedo): float32 (3,)."""
        d = self.desc()
        material = int(material)
        if not 0 <= material < d.n_materials:
            raise ValueError(f"material_albedo: material {material} is outside [0, {d.n_materials})")
        return _material_albedo(d.materials[material])

    def AddSphere(self, center, radius, material, medium_inside=-1, medium_outside=-1):
        """pbrt-v3 quadratic sphere (the reference's shape/Sphere.h is an unfinished stub; see include/gnxr.h)."""
        c = (C.c_float * 3)(*[float(v) for v in center])
        return _check(lib().gnxr_builder_add_sphere(self._h, c, float(radius), int(material), int(medium_inside), int(medium_outside)))

    def set_camera(self, eye=(0, 0, 5), look=(0, 0, 0), up=(0, 1, 0), fov=90.0, lens_radius=0.0, focal_distance=3.0, orthographic=False):
        """CreatePerspectiveCamera (camera/Perspective.cpp:114-135) or, orthographic=True, CreateOrthographicCamera
        (camera/Orthographic.cpp:94-121) on LookAt(eye, look, up)."""
        cam = Camera(_f3(eye), _f3(look), _f3(up), fov, lens_radius, focal_distance, int(bool(orthographic)))
        _check(lib().gnxr_builder_set_camera(self._h, C.byref(cam)))

    def set_bvh_split_method(self, method):
        """BVHAccel(prims, 1, SplitMethod::SAH | HLBVH | Middle | EqualCounts) (accelerator/BVHAccel.h:24-29); the reference uses SAH."""
        _check(lib().gnxr_builder_set_bvh_split_method(self._h, {"sah": 0, "hlbvh": 1, "middle": 2, "equal_counts": 3}[method]))

    def set_camera_medium(self, medium):
        _check(lib().gnxr_builder_set_camera_medium(self._h, int(medium)))

    def desc(self):
        """gnxr_scene_desc pointing into builder-owned memory (valid until the next builder call)."""
        d = SceneDesc()
        _check(lib().gnxr_builder_desc(self._h, C.byref(d)))
        return d


def camera(eye=(0, 0, 5), look=(0, 0, 0), up=(0, 1, 0), fov=90.0, lens_radius=0.0, focal_distance=3.0, orthographic=False):
    """The gnxr_camera record (ctypes `Camera`) of SceneBuilder.set_camera / Scene.set_camera's arguments: what RenderViews and
    camera_rays_device take."""
    return Camera(_f3(eye), _f3(look), _f3(up), fov, lens_radius, focal_distance, int(bool(orthographic)))


def _material_albedo(m):
    rgb = (C.c_float * 3)()
    _check(lib().gnxr_material_albedo(C.byref(m), rgb))
    return np.array(rgb[:], dtype=np.float32)


def material_albedo(**material_fields):
    """gnxr_material_albedo (host, needs no GPU): the colour the albedo channel of RenderAOV reports for a material with these gnxr_material
    fields (the keywords of SceneBuilder.add_material) -- kd clamped to [0, inf) for MATTE / PLASTIC / DISNEY, kr for MIRROR, 1 for GLASS,
    the normal-incidence conductor reflectance for METAL, 0 for NONE -- as a float32 (3,) array.  A kd_texture does not change it."""
    return _material_albedo(material(**material_fields))


def material(**material_fields):
    """One gnxr_material record (ctypes `Material`) from the keywords of SceneBuilder.add_material: what Scene.update_materials takes."""
    m = Material()
    for k, v in material_fields.items():
        if isinstance(v, (tuple, list, np.ndarray)):
            setattr(m, k, (C.c_float * len(v))(*[float(x) for x in v]))
        else:
            setattr(m, k, v)
    return m


def write_synthetic_3d(path, target_triangles=100000, seed=1):
    """Deterministic stand-in for the absent Resources/dragon.3d (`.MISSING_LARGE_BLOBS`)."""
    _check(lib().gnxr_write_synthetic_3d(os.fsencode(path), int(target_triangles), int(seed)))


class Scene:
    """Device-resident scene: replaces `Scene(make_shared<BVHAccel>(prims, 1), lights)` (RenderThread.cpp:155)."""

    def __init__(self, builder_or_desc):
        self._h = C.c_void_p()
        self._keep = builder_or_desc
        d = builder_or_desc.desc() if isinstance(builder_or_desc, SceneBuilder) else builder_or_desc
        self.n_triangles = int(d.n_triangles)
        self.n_vertices = int(d.n_vertices)
        self.n_lights = int(d.n_lights)   # (set_lights keeps it current)
        self.device = _device
        self.camera = Camera()   # a copy of the scene's own camera record (set_camera keeps it current)
        C.memmove(C.byref(self.camera), C.byref(d.camera), C.sizeof(Camera))
        self._env_light = None   # a copy of the INFINITE light's record (update_environment keeps it current)
        for i in range(int(d.n_lights)):
            if d.lights[i].type == _abi.LIGHT_INFINITE:
                self._env_light = Light()
                C.memmove(C.byref(self._env_light), C.byref(d.lights[i]), C.sizeof(Light))
                break
        self._textures = []      # copies of the Texture records, texel_offset zeroed (update_textures keeps them current)
        for i in range(int(d.n_textures)):
            t = Texture()
            C.memmove(C.byref(t), C.byref(d.textures[i]), C.sizeof(Texture))
            t.texel_offset = 0
            self._textures.append(t)
        _check(lib().gnxr_scene_create(C.byref(d), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.gnxr_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def info(self):
        n, dmax, nv = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().gnxr_scene_info(self._h, C.byref(n), C.byref(dmax), C.byref(nv)))
        return {"bvh_nodes": n.value, "bvh_max_depth": dmax.value, "light_voxels": nv.value}

    def nee_apply_counts(self):
        """gnxr_scene_nee_apply_counts: (light estimates the last PathIntegrator render added inside its traversal launches, by the pass after them)."""
        t, w = C.c_uint64(), C.c_uint64()
        _check(lib().gnxr_scene_nee_apply_counts(self._h, C.byref(t), C.byref(w)))
        return int(t.value), int(w.value)

    def hot_leaf_counts(self):
        """gnxr_scene_hot_leaf_counts: (triangles the last render's counting traversal took from LDS, triangles it loaded)."""
        h, t = C.c_uint64(), C.c_uint64()
        _check(lib().gnxr_scene_hot_leaf_counts(self._h, C.byref(h), C.byref(t)))
        return int(h.value), int(t.value)

    def trace_plan(self, total=1 << 24):
        """gnxr_scene_trace_plan: the shape of a traversal launch of `total` work items on this scene, as a dict."""
        t = _abi.TracePlan()
        _check(lib().gnxr_scene_trace_plan(self._h, int(total), C.byref(t)))
        return {k: int(getattr(t, k)) for k, _ in _abi.TracePlan._fields_ if k != "_pad"}

    # editing between frames (gnxr_scene_update_vertices / gnxr_scene_set_camera)
    def update_vertices(self, xyz, first_vertex=0, stream=None, move_lights=False):
        """Move vertices [first_vertex, first_vertex + len(xyz)) of the description's vertex array to xyz (world space, (n, 3) float32):
        a numpy array (host memory) or a contiguous torch tensor on the scene's device (read on `stream`, by default the current torch
        stream).  The BVH is refitted on the device with its topology kept.  Vertices of emissive triangles cannot move unless
        move_lights=True (gnxr_scene_update_vertices_ex with GNXR_UPDATE_MOVE_LIGHTS): then the area lights' records follow their
        triangles on the device."""
        ptr, xyz, _ = _host_or_device("update_vertices", xyz, np.float32, [(None, 3)], "(n, 3)", self.device)
        stream = _stream_handle("update_vertices", _edit_stream(stream, xyz))
        if move_lights:
            _check(lib().gnxr_scene_update_vertices_ex(self._h, int(first_vertex), int(xyz.shape[0]), _addr(ptr), _abi.UPDATE_MOVE_LIGHTS, _addr(stream)))
        else:
            _check(lib().gnxr_scene_update_vertices(self._h, int(first_vertex), int(xyz.shape[0]), _addr(ptr), _addr(stream)))

    def update_lights(self, lights, first_light=0):
        """Replace lights [first_light, first_light + len(lights)) of the scene's light list by `lights` (gnxr Light records, e.g. copies
        of SceneBuilder.desc().lights[i] with fields changed): le / two_sided / n_samples of an area light, anything of a point, spot or
        distant light, centre and radius of the sky box (gnxr_scene_update_lights).  A changed type, a changed triangle or a changed
        INFINITE record raises GnxrError and leaves the scene as it was."""
        lights = list(lights)
        for l in lights:
            if not isinstance(l, Light):
                raise ValueError(f"update_lights: lights must be gnxr Light records, got {type(l).__name__}")
        arr = (Light * max(len(lights), 1))(*lights)
        _check(lib().gnxr_scene_update_lights(self._h, int(first_light), len(lights), arr))

    def set_lights(self, lights, stream=None):
        """Replace the scene's light list by `lights` (a list of gnxr Light records, possibly empty): lights may be added, removed and
        retyped, and other triangles may become emissive (gnxr_scene_set_lights).  An AREA_TRI record names its triangle in authoring
        order (`tri`), no two the same one; its corners, area and normal come from the vertices the scene holds now.  The INFINITE
        record, if the scene has one, must be in the list unchanged (update_environment changes it).  Afterwards every result is that of
        a scene created with this list; tree, materials, textures, media, environment tables and the reserved path state are kept.
        `stream`: None (the null stream), a torch.cuda.Stream or a hipStream_t as a non-negative integer.  Anything that is not a Light
        raises ValueError before the library is called; a refusal raises GnxrError and leaves the scene as it was."""
        lights = list(lights)
        for l in lights:
            if not isinstance(l, Light):
                raise ValueError(f"set_lights: lights must be gnxr Light records, got {type(l).__name__}")
        handle = _stream_handle("set_lights", stream)
        arr = (Light * max(len(lights), 1))()
        for k, l in enumerate(lights):
            C.memmove(C.byref(arr[k]), C.byref(l), C.sizeof(Light))
        _check(lib().gnxr_scene_set_lights(self._h, arr if lights else None, len(lights), _addr(handle)))
        self.n_lights = len(lights)
        self._env_light = None
        for l in lights:
            if l.type == _abi.LIGHT_INFINITE:
                self._env_light = Light()
                C.memmove(C.byref(self._env_light), C.byref(l), C.sizeof(Light))
                break

    def light_tables(self):
        """Test hook: the light tables of the first device (gnxr_scene_light_tables): (the device's light records as uint32 words,
        (n_lights, 28); per triangle in authoring order the light it is, int32 (n_triangles,), -1 == none)."""
        out = []
        for which, dtype, cols in ((0, np.uint32, _abi.DLIGHT_BYTES // 4), (1, np.int32, 0)):
            n = C.c_int64(0)
            _check(lib().gnxr_scene_light_tables(self._h, which, None, 0, C.byref(n)))
            a = np.zeros(n.value // 4, dtype)
            if n.value:
                _check(lib().gnxr_scene_light_tables(self._h, which, C.c_void_p(a.ctypes.data), n.value, C.byref(n)))
            out.append(a.reshape(-1, cols) if cols else a)
        return tuple(out)

    def update_materials(self, materials, first_material=0):
        """Replace materials [first_material, first_material + len(materials)) of the scene's material list by `materials` (gnxr Material
        records: material(type=..., kd=...), or copies of SceneBuilder.desc().materials[i] with fields changed).  Every field may change,
        the type included (gnxr_scene_update_materials); afterwards the scene renders as one created with those records.  An unknown
        type or a texture the scene does not have raises GnxrError and leaves the scene as it was."""
        materials = list(materials)
        for m in materials:
            if not isinstance(m, Material):
                raise ValueError(f"update_materials: materials must be gnxr Material records, got {type(m).__name__}")
        arr = (Material * max(len(materials), 1))(*materials)
        _check(lib().gnxr_scene_update_materials(self._h, int(first_material), len(materials), arr))

    def set_triangle_materials(self, ids, first_triangle=0, stream=None):
        """Give triangles [first_triangle, first_triangle + len(ids)) (authoring order) the materials `ids`: an int32 (n,) numpy array
        (host memory) or a contiguous int32 (n,) torch tensor on the scene's device (read on `stream`, by default the current torch
        stream), values in [-1, n_materials), -1 == no material (gnxr_scene_set_triangle_materials)."""
        ptr, ids, _ = _host_or_device("set_triangle_materials", ids, np.int32, [(None,)], "(n,)", self.device)
        stream = _stream_handle("set_triangle_materials", _edit_stream(stream, ids))
        _check(lib().gnxr_scene_set_triangle_materials(self._h, int(first_triangle), int(ids.shape[0]), _addr(ptr), _addr(stream)))

    def triangle_materials(self):
        """Test hook: per triangle in authoring order, read from the device, (authored material index it shows or -1, shade class):
        (int32 (n,), uint8 (n,))."""
        mat = np.zeros(self.n_triangles, np.int32); cls = np.zeros(self.n_triangles, np.uint8)
        rc = lib().gnxr_scene_triangle_materials(self._h, mat.ctypes.data_as(C.POINTER(C.c_int32)), cls.ctypes.data_as(C.POINTER(C.c_uint8)), self.n_triangles)
        if rc < 0:
            _check(rc)
        return mat, cls

    def update_attributes(self, uv=None, normals=None, tangents=None, first_triangle=0, stream=None):
        """Replace per-corner attributes of triangles [first_triangle, first_triangle + n) (authoring order) of a live scene
        (gnxr_scene_update_attributes): float32 (n, 6) uv, (n, 9) normals and (n, 9) tangents in the description's layout, None = leave that
        table as it is.  The arrays are ALL numpy arrays (host memory) or ALL contiguous torch tensors on the scene's device, read where
        they lie on `stream` (by default torch's current stream).  Afterwards every result is that of a scene created with these
        attributes.  Malformed arguments raise ValueError before the library is called; a refusal -- a table the scene was created
        without, a triangle that would gain or lose attributes of its own, normals or tangents on an emissive triangle -- raises
        GnxrError and leaves the scene as it was."""
        name = "update_attributes"
        given = [(what, x, cols) for what, x, cols in (("uv", uv, 6), ("normals", normals, 9), ("tangents", tangents, 9)) if x is not None]
        if not given:
            raise ValueError(f"{name}: none of uv, normals, tangents given")
        on_device = _arrays_on_device(name, given[0][0], given[0][1])
        handle = _stream_handle(name, _edit_stream(stream, given[0][1]))
        ptrs, keep, n = {}, [], None
        for what, x, cols in given:
            ptrs[what], x, _ = _host_or_device(f"{name}: {what}", x, np.float32, [(None, cols)], f"(n, {cols})", self.device, on_device)
            keep.append(x)
            if n is not None and x.shape[0] != n:
                raise ValueError(f"{name}: {what} has {x.shape[0]} rows, {given[0][0]} has {n}")
            n = int(x.shape[0])
        _check(lib().gnxr_scene_update_attributes(self._h, int(first_triangle), n, _addr(ptrs.get("uv")), _addr(ptrs.get("normals")), _addr(ptrs.get("tangents")), _addr(handle)))

    def triangle_attributes(self):
        """Test hook: the per-corner attributes the first device holds, in authoring order (gnxr_scene_triangle_attributes):
        (uv (n, 6), normals (n, 9), tangents (n, 9)) float32, None for a table the scene does not have."""
        out = []
        for which, cols in ((0, 6), (1, 9), (2, 9)):
            n = C.c_int64(0)
            _check(lib().gnxr_scene_triangle_attributes(self._h, which, None, 0, C.byref(n)))
            if n.value == 0:
                out.append(None)
                continue
            a = np.zeros(n.value, np.float32)
            _check(lib().gnxr_scene_triangle_attributes(self._h, which, a.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
            out.append(a.reshape(-1, cols))
        return tuple(out)

    def recompute_normals(self, flip=False, stream=None):
        """Shading normals of the smooth triangles (those whose normal row is not all zero) from the vertices the scene holds now
        (gnxr_scene_recompute_normals; the definition, operation by operation: include/gnxr.h): area-weighted sums of face normals over
        the triangles that share a vertex index, normalised; flat triangles, uvs and tangents are untouched.  flip=True negates every
        face normal.  A scene without per-corner normals is left as it is.  `stream`: None (the null stream), a torch.cuda.Stream or a
        hipStream_t as a non-negative integer."""
        handle = _stream_handle("recompute_normals", stream)
        _check(lib().gnxr_scene_recompute_normals(self._h, _abi.NORMALS_FLIP if flip else 0, _addr(handle)))

    def rebuild_bvh(self, stream=None):
        """Rebuild the BVH on the device over the vertices the scene holds now (after update_vertices): the HLBVH tree a new Scene over
        those vertices would get, with materials, textures, tables and the reserved path state kept.  `stream`: None (the null stream),
        a torch.cuda.Stream or a hipStream_t as a non-negative integer (TypeError / ValueError otherwise); the work is ordered after what it
        holds."""
        handle = _stream_handle("rebuild_bvh", stream)
        _check(lib().gnxr_scene_rebuild_bvh(self._h, _addr(handle)))

    def set_geometry(self, vertices, indices, tri_material, tri_light=None, medium_inside=None, medium_outside=None, uv=None, normals=None,
                     tangents=None, stream=None):
        """Replace the scene's triangle mesh (gnxr_scene_set_geometry): float32 (nv, 3) vertices in world space, int32 (nt, 3) indices,
        int32 (nt,) tri_material (or one integer for all triangles; -1 == no material), and optionally int32 (nt,) tri_light (required
        when the scene has area lights: each must be named by exactly one triangle), int32 (nt,) medium_inside and medium_outside (both
        or neither), float32 (nt, 6) uv, (nt, 9) normals and (nt, 9) tangents in the description's layout.  The arrays are ALL numpy
        arrays or ALL contiguous torch tensors on the scene's device; tensors are read where they lie, on `stream` (default: torch's
        current stream).  Afterwards the scene gives the results of a new Scene with this mesh and an HLBVH tree; materials, lights'
        parameters, textures, media, environment, camera and the reserved path state are kept.  Malformed arguments raise ValueError
        before the library is called; a refusal raises GnxrError and leaves the scene as it was."""
        import numbers
        name = "set_geometry"
        on_device = _arrays_on_device(name, "vertices", vertices)
        stream = _edit_stream(stream, vertices)
        handle = _stream_handle(name, stream)

        def arr(what, x, dtype, cols, rows):
            """a checked array and its address: at least one row, `rows` of them where that is given"""
            text = f"({'n' if rows is None else rows}{', %d' % cols if cols else ''})"
            address, x, _ = _host_or_device(f"{name}: {what}", x, dtype, [(rows or SOME,) + ((cols,) if cols else ())], text, self.device, on_device, tensor_text=f"array of shape {text}")
            return x, address

        keep = []
        g = _abi.Geometry()
        g.struct_size = C.sizeof(_abi.Geometry)
        v, g.vertices = arr("vertices", vertices, np.float32, 3, None)
        idx, g.indices = arr("indices", indices, np.int32, 3, None)
        nt = int(idx.shape[0])
        if isinstance(tri_material, numbers.Integral) and not isinstance(tri_material, bool):
            if on_device:   # filled on the stream the call reads on
                import torch
                ts = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(handle, device=v.device)
                with torch.cuda.stream(ts):
                    tri_material = torch.full((nt,), int(tri_material), dtype=torch.int32, device=v.device)
            else:
                tri_material = np.full(nt, int(tri_material), np.int32)
        keep += [v, idx]
        for field, what, x, dtype, cols, required in (("tri_material", "tri_material", tri_material, np.int32, 0, True), ("tri_light", "tri_light", tri_light, np.int32, 0, False),
                                                      ("tri_medium_inside", "medium_inside", medium_inside, np.int32, 0, False),
                                                      ("tri_medium_outside", "medium_outside", medium_outside, np.int32, 0, False), ("tri_uv", "uv", uv, np.float32, 6, False),
                                                      ("tri_n", "normals", normals, np.float32, 9, False), ("tri_s", "tangents", tangents, np.float32, 9, False)):
            if x is None and not required:
                continue
            a, ptr = arr(what, x, dtype, cols, nt)
            keep.append(a)
            setattr(g, field, ptr)
        if (medium_inside is None) != (medium_outside is None):
            raise ValueError(f"{name}: medium_inside and medium_outside come together or not at all")
        g.n_vertices, g.n_triangles = int(v.shape[0]), nt
        _check(lib().gnxr_scene_set_geometry(self._h, C.byref(g), _addr(handle)))
        self.n_triangles, self.n_vertices = nt, int(v.shape[0])

    def update_environment(self, rgb=None, le=None, light_to_world=None, n_samples=None, stream=None):
        """Replace or rotate the environment map of the scene's INFINITE light (gnxr_scene_update_environment).  rgb: the new map, an
        (h, w, 3) float32 numpy array (host memory) or a contiguous float32 (h, w, 3) torch tensor on the scene's device (read on `stream`,
        by default the current torch stream); its size may differ from the old map's.  le, light_to_world (16 floats, row-major) and
        n_samples replace those fields of the light's record; omitted ones keep their current values.  The tables are rebuilt on the
        device and every later result is that of a scene created with this map and record.  rgb=None only rotates (or changes
        n_samples): le must then stay as it is (GnxrError otherwise: the raw map is not retained, send it again)."""
        rec = Light()
        if self._env_light is not None:
            C.memmove(C.byref(rec), C.byref(self._env_light), C.sizeof(Light))
        else:   # (the library refuses a scene without an INFINITE light)
            rec.type, rec.tri, rec.n_samples = _abi.LIGHT_INFINITE, -1, 1
            rec.le[:] = [1.0, 1.0, 1.0]
            rec.light_to_world[:] = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
        if le is not None:
            rec.le[:] = [float(x) for x in le]
        if light_to_world is not None:
            rec.light_to_world[:] = [float(x) for x in np.asarray(light_to_world, dtype=np.float32).reshape(16)]
        if n_samples is not None:
            rec.n_samples = int(n_samples)
        ptr, w, h = None, 0, 0
        if rgb is not None:
            ptr, rgb, _ = _host_or_device("update_environment", rgb, np.float32, [(None, None, 3)], "(h, w, 3)", self.device, or_none=True)
            h, w = rgb.shape[0], rgb.shape[1]
        stream = _stream_handle("update_environment", _edit_stream(stream, rgb))
        _check(lib().gnxr_scene_update_environment(self._h, C.byref(rec), _addr(ptr), int(w), int(h), _addr(stream)))
        self._env_light = rec

    ENV_TABLES = (("env_texels4", np.float32), ("env_cond_func", np.float32), ("env_cond_cdf", np.float32), ("env_cond_int", np.float32),
                  ("env_marg_func", np.float32), ("env_marg_cdf", np.float32), ("env_marg_guide", np.uint16), ("env_cond_guide", np.uint16),
                  ("env", np.uint32), ("env_power_lookup", np.float32))

    def env_tables(self):
        """Test hook: the environment tables of the first device (gnxr_scene_env_tables) as a dict of flat arrays: the eight tables, the
        DEnv record renders are given ("env", as uint32 words) and the Power lookup; empty arrays for a scene without an INFINITE light."""
        out = {}
        for which, (name, dtype) in enumerate(self.ENV_TABLES):
            n = C.c_int64(0)
            _check(lib().gnxr_scene_env_tables(self._h, which, None, 0, C.byref(n)))
            a = np.zeros(n.value // np.dtype(dtype).itemsize, dtype)
            if n.value:
                _check(lib().gnxr_scene_env_tables(self._h, which, C.c_void_p(a.ctypes.data), n.value, C.byref(n)))
            out[name] = a
        return out

    def update_media(self, media, density=None, first_medium=0, stream=None):
        """Replace media [first_medium, first_medium + len(media)) of the scene's medium list by `media` (gnxr Medium records, or one
        record): coefficients, g, medium_to_world, the grid resolution and the type may all change (gnxr_scene_update_media).  density:
        one array per GRID record of the call, in record order (a list, or the array itself when there is one such record); each a
        float32 numpy array (host memory) or a contiguous float32 torch tensor on the scene's device, of shape (nz, ny, nx) or flat with
        nx * ny * nz entries.  The records' density_offset is set here.  Host arrays are packed and sent in ONE call, which takes all
        records or none.  Torch tensors are read where they lie, on `stream` (by default the current torch stream): no tensor is
        concatenated or copied, so the records go one call each, in order (a GRID record with its tensor, a HOMOGENEOUS one alone) --
        a record the library refuses leaves the earlier ones applied.  (The C call itself takes several device grids at once, as one
        packed allocation with the offsets in the records; this method does not offer that form: a caller who needs several device grids
        to change together calls gnxr_scene_update_media through lib().)  density=None changes coefficients only: every GRID record must then
        name a medium that is GRID now, with the same resolution, whose grid stays.  Afterwards the scene renders as one created with
        these media and grids; a refused call raises GnxrError and leaves the scene as it was."""
        media = [media] if isinstance(media, Medium) else list(media)
        for m in media:
            if not isinstance(m, Medium):
                raise ValueError(f"update_media: media must be gnxr Medium records, got {type(m).__name__}")
        recs = (Medium * max(len(media), 1))()
        for k, m in enumerate(media):
            C.memmove(C.byref(recs[k]), C.byref(m), C.sizeof(Medium))
        if density is None:
            handle = _stream_handle("update_media", stream)
            _check(lib().gnxr_scene_update_media(self._h, int(first_medium), len(media), recs, None, _addr(handle)))
            return
        grids = [density] if isinstance(density, np.ndarray) or _is_torch(density) else density
        if not isinstance(grids, (list, tuple)):
            raise ValueError(f"update_media: expected a numpy array, a torch tensor, a list of them or None, got {type(density).__name__}")
        grids = list(grids)
        grid_recs = [k for k, m in enumerate(media) if m.type == _abi.MEDIUM_GRID]
        if len(grids) != len(grid_recs):
            raise ValueError(f"update_media: {len(grids)} density arrays for {len(grid_recs)} GRID records")
        on_device = [_is_torch(g) for g in grids]
        if any(on_device) and not all(on_device):
            raise ValueError("update_media: density arrays must be all numpy arrays or all torch tensors")
        for i, k in enumerate(grid_recs):
            nx, ny, nz = recs[k].nx, recs[k].ny, recs[k].nz
            shapes = ((nz, ny, nx), (nx * ny * nz,))
            _, grids[i], _ = _host_or_device("update_media", grids[i], np.float32, shapes, f"{shapes[0]} or {shapes[1]}", self.device)
        if not any(on_device):   # host memory: one packed array, one call
            offsets = np.cumsum([0] + [g.size for g in grids])
            packed = np.concatenate([g.reshape(-1) for g in grids]) if grids else np.zeros(1, np.float32)
            for k, off in zip(grid_recs, offsets):
                recs[k].density_offset = int(off)
            handle = _stream_handle("update_media", stream)
            _check(lib().gnxr_scene_update_media(self._h, int(first_medium), len(media), recs, _addr(packed.ctypes.data), _addr(handle)))
            return
        handle = _stream_handle("update_media", _edit_stream(stream, grids[0]))
        tensor_of = dict(zip(grid_recs, grids))
        for k in range(len(media)):
            one = (Medium * 1)()
            C.memmove(C.byref(one[0]), C.byref(recs[k]), C.sizeof(Medium))
            one[0].density_offset = 0
            _check(lib().gnxr_scene_update_media(self._h, int(first_medium) + k, 1, one, _ptr(tensor_of.get(k)), _addr(handle)))

    def media_tables(self):
        """Test hook: the medium tables of the first device (gnxr_scene_media_tables): {"records": the device's medium records as uint32
        words, (n_media, 32), density_offset written as 0; "grids": one flat float32 array per medium, empty for a HOMOGENEOUS one}."""
        n = C.c_int64(0)
        _check(lib().gnxr_scene_media_tables(self._h, 0, 0, None, 0, C.byref(n)))
        records = np.zeros((n.value // _abi.DMEDIUM_BYTES, _abi.DMEDIUM_BYTES // 4), np.uint32)
        if n.value:
            _check(lib().gnxr_scene_media_tables(self._h, 0, 0, C.c_void_p(records.ctypes.data), n.value, C.byref(n)))
        grids = []
        for i in range(len(records)):
            _check(lib().gnxr_scene_media_tables(self._h, 1, i, None, 0, C.byref(n)))
            g = np.zeros(n.value // 4, np.float32)
            if n.value:
                _check(lib().gnxr_scene_media_tables(self._h, 1, i, C.c_void_p(g.ctypes.data), n.value, C.byref(n)))
            grids.append(g)
        return {"records": records, "grids": grids}

    TEXTURE_PARAMS = ("su", "sv", "du", "dv", "trilinear", "max_aniso", "wrap", "scale", "gamma")

    def update_textures(self, images=None, first_texture=0, params=None, stream=None):
        """Replace image textures [first_texture, first_texture + n) of the scene's texture list (gnxr_scene_update_textures).  images:
        one array per replaced texture (a list, or the array itself when there is one): each an (h, w, 3) float32 numpy array (host
        memory) or a contiguous float32 (h, w, 3) torch tensor on the scene's device, decoded texels with row 0 the top row; the size may
        differ from the old texture's.  params: per texture a dict of the keywords of SceneBuilder.add_image_texture (su, sv, du, dv,
        trilinear, max_aniso, wrap, scale, gamma), or one dict when there is one texture; omitted keys keep the texture's current
        value.  The Scene keeps a copy of every record, as created and as edited.  Host arrays are packed and sent in ONE call, which
        takes all textures or none.  Torch tensors are read where they lie, on `stream` (by default the current torch stream): no tensor
        is concatenated or copied, so the textures go one call each, in order -- a texture the library refuses leaves the earlier ones
        applied.  (The C call itself takes several device textures at once, as one packed allocation with the offsets in the records;
        this method does not offer that form: a caller who needs several device textures to change together calls
        gnxr_scene_update_textures through lib().)  images=None changes parameters only: su, sv, du, dv, max_aniso and trilinear; wrap,
        gamma and scale are baked into the texels and must then stay as they are (GnxrError otherwise: send the image).  The pyramids are
        built on the device and every later result is that of a scene created with these textures; a refused call raises GnxrError and
        leaves the scene as it was."""
        if images is None:
            imgs = None
        elif isinstance(images, np.ndarray) or _is_torch(images):
            imgs = [images]
        elif isinstance(images, (list, tuple)):
            imgs = list(images)
        else:
            raise ValueError(f"update_textures: expected a numpy array, a torch tensor, a list of them or None, got {type(images).__name__}")
        if params is None:
            plist = None
        elif isinstance(params, dict):
            plist = [params]
        elif isinstance(params, (list, tuple)):
            plist = list(params)
        else:
            raise ValueError(f"update_textures: params must be a dict, a list of dicts or None, got {type(params).__name__}")
        if imgs is None and plist is None:
            raise ValueError("update_textures: neither images nor params given")
        n = len(imgs) if imgs is not None else len(plist)
        if plist is not None and len(plist) != n:
            raise ValueError(f"update_textures: {len(plist)} parameter dicts for {n} images")
        first_texture = int(first_texture)
        if first_texture < 0 or first_texture + n > len(self._textures):
            raise ValueError(f"update_textures: textures [{first_texture}, {first_texture + n}) outside the scene's {len(self._textures)} textures")
        recs = (Texture * max(n, 1))()
        for k in range(n):
            C.memmove(C.byref(recs[k]), C.byref(self._textures[first_texture + k]), C.sizeof(Texture))
            for key, v in ((plist[k] or {}) if plist is not None else {}).items():
                if key not in self.TEXTURE_PARAMS:
                    raise ValueError(f"update_textures: unknown texture parameter {key!r} (expected one of {', '.join(self.TEXTURE_PARAMS)})")
                if key == "wrap":
                    if v not in ("repeat", "black", "clamp"):
                        raise ValueError(f"update_textures: wrap must be 'repeat', 'black' or 'clamp', got {v!r}")
                    recs[k].wrap = {"repeat": 0, "black": 1, "clamp": 2}[v]
                elif key in ("trilinear", "gamma"):
                    setattr(recs[k], key, int(bool(v)))
                else:
                    setattr(recs[k], key, float(v))
        on_device = [_is_torch(g) for g in imgs] if imgs is not None else []
        if any(on_device) and not all(on_device):
            raise ValueError("update_textures: images must be all numpy arrays or all torch tensors")
        for k in range(len(imgs or [])):
            _, imgs[k], _ = _host_or_device("update_textures", imgs[k], np.float32, [(SOME, SOME, 3)], "(h, w, 3)", self.device)
            recs[k].height, recs[k].width = int(imgs[k].shape[0]), int(imgs[k].shape[1])

        def keep(k):
            C.memmove(C.byref(self._textures[first_texture + k]), C.byref(recs[k]), C.sizeof(Texture))
            self._textures[first_texture + k].texel_offset = 0

        if imgs is None or not any(on_device):   # parameters only, or host memory: one packed array, one call
            packed = None
            if imgs:
                offsets = np.cumsum([0] + [g.size for g in imgs])
                packed = np.concatenate([g.reshape(-1) for g in imgs])
                for k in range(n):
                    recs[k].texel_offset = int(offsets[k])
            handle = _stream_handle("update_textures", stream)
            _check(lib().gnxr_scene_update_textures(self._h, first_texture, n, recs, _addr(packed.ctypes.data) if packed is not None else None, _addr(handle)))
            for k in range(n):
                keep(k)
            return
        handle = _stream_handle("update_textures", _edit_stream(stream, imgs[0]))
        for k in range(n):
            one = (Texture * 1)()
            C.memmove(C.byref(one[0]), C.byref(recs[k]), C.sizeof(Texture))
            one[0].texel_offset = 0
            _check(lib().gnxr_scene_update_textures(self._h, first_texture + k, 1, one, _ptr(imgs[k]), _addr(handle)))
            keep(k)

    def texture_tables(self):
        """Test hook: the texture tables of the first device (gnxr_scene_texture_tables): {"records": the device's texture records as
        uint32 words, (n_textures, 28); "texels": one flat float32 array per texture, the float4 (rgb_) texels of all its levels}."""
        n = C.c_int64(0)
        _check(lib().gnxr_scene_texture_tables(self._h, 0, 0, None, 0, C.byref(n)))
        records = np.zeros((n.value // _abi.DTEXTURE_BYTES, _abi.DTEXTURE_BYTES // 4), np.uint32)
        if n.value:
            _check(lib().gnxr_scene_texture_tables(self._h, 0, 0, C.c_void_p(records.ctypes.data), n.value, C.byref(n)))
        texels = []
        for i in range(len(records)):
            _check(lib().gnxr_scene_texture_tables(self._h, 1, i, None, 0, C.byref(n)))
            t = np.zeros(n.value // 4, np.float32)
            if n.value:
                _check(lib().gnxr_scene_texture_tables(self._h, 1, i, C.c_void_p(t.ctypes.data), n.value, C.byref(n)))
            texels.append(t)
        return {"records": records, "texels": texels}

    def set_camera(self, eye=(0, 0, 5), look=(0, 0, 0), up=(0, 1, 0), fov=90.0, lens_radius=0.0, focal_distance=3.0, orthographic=False, medium=-1):
        """The camera of SceneBuilder.set_camera (and the medium it sits in, -1 == none) for later renders."""
        cam = camera(eye, look, up, fov, lens_radius, focal_distance, orthographic)
        _check(lib().gnxr_scene_set_camera(self._h, C.byref(cam), int(medium)))
        self.camera = cam

    # Aggregate seam: Scene::Intersect / IntersectP, batched
    def bvh(self):
        """Test hook: (bounds [n, 6], meta [n, 3] = offset / nPrimitives / axis, primitive order) of the flattened binary BVH."""
        n = C.c_int64(0)
        _check(lib().gnxr_scene_bvh(self._h, None, None, None, 0, C.byref(n)))
        bounds = np.zeros((n.value, 6), np.float32); meta = np.zeros((n.value, 3), np.int32); order = np.zeros(self.n_triangles, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        _check(lib().gnxr_scene_bvh(self._h, bounds.ctypes.data_as(C.POINTER(C.c_float)), ip(meta), ip(order), n.value, C.byref(n)))
        return bounds, meta, order

    def bvh4(self):
        """Test hook: (nodes [n, 32] uint32 = the 128-byte DNode4 records of the first device, root reference, worst-case stack entries)
        of the 4-wide tree."""
        n, root4, need = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _check(lib().gnxr_scene_bvh4(self._h, None, 0, C.byref(n), C.byref(root4), C.byref(need)))
        nodes = np.zeros((n.value, 32), np.uint32)
        _check(lib().gnxr_scene_bvh4(self._h, C.c_void_p(nodes.ctypes.data), n.value, C.byref(n), C.byref(root4), C.byref(need)))
        return nodes, root4.value, need.value

    def light_grid_table(self, strategy="spatial", on_host=False):
        """Test hook: the light-selection table (device-built or host-built)."""
        code = {"spatial": _abi.LIGHTS_SPATIAL, "uniform": _abi.LIGHTS_UNIFORM, "power": _abi.LIGHTS_POWER}[strategy]
        n = C.c_int64(0)
        _check(lib().gnxr_light_grid_table(self._h, code, int(on_host), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float32)
        _check(lib().gnxr_light_grid_table(self._h, code, int(on_host), out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return out

    def Intersect(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        _check(lib().gnxr_trace_closest(self._h, rays.ctypes.data_as(C.POINTER(Ray)), len(rays),
                                        hits.ctypes.data_as(C.POINTER(Hit))))
        return hits

    def IntersectP(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        occ = np.zeros(len(rays), dtype=np.uint8)
        _check(lib().gnxr_trace_any(self._h, rays.ctypes.data_as(C.POINTER(Ray)), len(rays),
                                    occ.ctypes.data_as(C.POINTER(C.c_uint8))))
        return occ

    # batched queries on device memory (gnxr_trace_closest_device / gnxr_trace_any_device)
    def _query(self, name, rays, out, dtype, cols, stream):
        import torch
        _expect(f"{name}: rays", rays, torch.float32, (8,), self.device)
        n = rays.shape[0]
        out = _out_tensor(f"{name}: out", out, (n, cols) if cols else (n,), dtype, rays.device)
        st, _ = _stream_pair(stream, rays.device)
        fn = lib().gnxr_trace_closest_device if cols else lib().gnxr_trace_any_device
        _check(fn(self._h, _ptr(rays), n, _ptr(out), _addr(st)))
        return out

    def intersect(self, rays, out=None, stream=None):
        """Scene::Intersect for rays already on the GPU: `rays` is a contiguous float32 (n, 8) tensor in the gnxr_ray layout (rays_tensor)
        on the scene's device.  Returns RayHits: the (n, 8) float32 gnxr_hit records (`out` when given) and named views of them.  The
        work is queued on `stream` (by default torch's current stream) and nothing waits for it; the results equal Intersect's bit for bit."""
        import torch
        hits = self._query("intersect", rays, out, torch.float32, 8, stream)
        return RayHits(hits, hits.view(torch.int32)[:, 0], hits[:, 1], hits[:, 2:5], hits[:, 5:8])

    def occluded(self, rays, out=None, stream=None):
        """Scene::IntersectP for rays already on the GPU (see intersect): a uint8 (n,) tensor, 1 where something is hit in (0, tmax)."""
        import torch
        return self._query("occluded", rays, out, torch.uint8, 0, stream)

    # shading queries on device memory (gnxr_bsdf_device / gnxr_light_sample_device / gnxr_light_le_device)
    def _query_args(self, name, args, out, out_cols, stream):
        """`args`: (what, tensor, dtype, cols) each -- contiguous (n, cols) tensors on the scene's device with one n.  Returns
        (n, out, hipStream_t, torch stream of that handle)."""
        import torch
        n = None
        for what, x, dtype, cols in args:
            _expect(f"{name}: {what}", x, dtype, (cols,))
        for what, x, dtype, cols in args:
            _expect(f"{name}: {what}", x, dtype, (cols,), self.device)
            n = x.shape[0] if n is None else n
            _same_count(name, what, x.shape[0], n, args[0][0])
        out = _out_tensor(f"{name}: out", out, (n, out_cols), torch.float32, args[0][1].device)
        return (n, out) + _stream_pair(stream, args[0][1].device)

    def bsdf(self, rays, wi, u, flags=31, differentials=None, out=None, stream=None):
        """BSDF::f / Pdf / Sample_f at the hits of rays already on the GPU (gnxr_bsdf_device): Scene::Intersect along `rays` (float32
        (n, 8), the gnxr_ray layout of rays_tensor), ComputeScatteringFunctions(Radiance, allowMultipleLobes = true) there and, with
        wo = Normalize(-d): f and Pdf towards the world-space `wi` (n, 3), Sample_f with `u` (n, 2), under the BxDFType mask `flags`
        (31 = BSDF_ALL).  `differentials`: None, or (n, 12) rxOrigin, rxDirection, ryOrigin, ryDirection (they filter image textures).
        Returns a float32 (n, 16) tensor (`out` when given) whose columns are f[0:3], pdf[3], sample_f[4:7], sample_pdf[7],
        sample_wi[8:11], sampled_type[11], n_components[12], valid[13], dudx[14], dvdy[15]; valid is 1 where the ray hit a surface
        with a BSDF and the row is 0 elsewhere.  The three integers of the gnxr_bsdf_result records are converted to float32 here, on
        the same stream, so that the tensor is one dtype.  Queued on `stream` (default: torch's current stream); nothing waits."""
        import torch
        args = [("rays", rays, torch.float32, 8), ("wi", wi, torch.float32, 3), ("u", u, torch.float32, 2)]
        if differentials is not None:
            args.append(("differentials", differentials, torch.float32, 12))
        flags = int(flags)
        if not 0 <= flags <= 31:
            raise ValueError(f"bsdf: flags must be a BxDFType mask in [0, 31], got {flags}")
        n, out, st, tstream = self._query_args("bsdf", args, out, 16, stream)
        _check(lib().gnxr_bsdf_device(self._h, _ptr(rays), _ptr(wi), _ptr(u), _ptr(differentials), n, flags, _ptr(out), _addr(st)))
        if n:
            with torch.cuda.stream(tstream):
                out[:, 11:14] = out.view(torch.int32)[:, 11:14].to(torch.float32)
        return out

    def sample_light(self, light, p, n, u, wi_query, strategy=_abi.LIGHTS_SPATIAL, out=None, stream=None):
        """Light::Sample_Li / Pdf_Li and the light-selection probability at points already on the GPU (gnxr_light_sample_device): for
        the reference point `p` (m, 3) with normal `n` (m, 3) and light `light` (an index into the scene's lights: an int, or an int32
        (m,) tensor for one light per query), Sample_Li with `u` (m, 2), Pdf_Li towards `wi_query` (m, 3), and the probability with
        which the light distribution of `strategy` (LIGHTS_SPATIAL / LIGHTS_UNIFORM / LIGHTS_POWER or their names) picks the light at p.
        Returns a float32 (m, 12) tensor (`out` when given): Li[0:3], pdf[3], wi[4:7], pdf_li[7], pdf_select[8], p_light[9:12] (the
        sampled point: the far end of the shadow ray).  A light index out of range raises GnxrError after the other queries are
        finished; its row is 0.  Queued on `stream` (default: torch's current stream); the call waits for the result's status."""
        import torch
        if isinstance(strategy, bool) or strategy not in LIGHT_STRATEGIES and strategy not in LIGHT_STRATEGIES.values():
            raise ValueError(f"sample_light: strategy must be one of {sorted(LIGHT_STRATEGIES)} or LIGHTS_SPATIAL / LIGHTS_UNIFORM / LIGHTS_POWER, got {strategy!r}")
        strategy = LIGHT_STRATEGIES.get(strategy, strategy)
        args = [("p", p, torch.float32, 3), ("n", n, torch.float32, 3), ("u", u, torch.float32, 2), ("wi_query", wi_query, torch.float32, 3)]
        m, out, st, tstream = self._query_args("sample_light", args, out, 12, stream)
        if isinstance(light, torch.Tensor):
            if not (light.dtype == torch.int32 and light.dim() == 1 and light.shape[0] == m and light.is_cuda and light.device == p.device):
                raise ValueError(f"sample_light: light must be an int or an int32 ({m},) tensor on {p.device}, got {_got(light, type_name=False)}")
        elif not isinstance(light, (int, np.integer)) or isinstance(light, bool):
            raise ValueError(f"sample_light: light must be an int or an int32 tensor, got {type(light).__name__}")
        with torch.cuda.stream(tstream):   # the packed gnxr_light_sample_device queries: p, light, n, u, wi_query
            q = torch.empty((m, 12), dtype=torch.float32, device=p.device)
            q[:, 0:3] = p
            q.view(torch.int32)[:, 3] = light if isinstance(light, torch.Tensor) else int(light)
            q[:, 4:7] = n
            q[:, 7:9] = u
            q[:, 9:12] = wi_query
        _check(lib().gnxr_light_sample_device(self._h, _ptr(q), m, int(strategy), _ptr(out), _addr(st)))
        return out

    def light_le(self, light, rays, out=None, stream=None):
        """Light::Le(ray) of light `light` for escaped rays already on the GPU (gnxr_light_le_device): float32 (n, 8) rays in, a float32
        (n, 3) tensor out (`out` when given); zero for lights that have no Le.  Queued on `stream`; nothing waits."""
        import torch
        n, out, st, _ = self._query_args("light_le", [("rays", rays, torch.float32, 8)], out, 3, stream)
        _check(lib().gnxr_light_le_device(self._h, int(light), _ptr(rays), n, _ptr(out), _addr(st)))
        return out

    # closest-point queries (gnxr_closest_point_device / gnxr_closest_point)
    def _point_queries(self, name, points, max_distance, stream, radius="max_distance"):
        """The (n, 4) float32 gnxr_point_query records of the point queries (closest_point, within, count_within, nearest): `points` as
        ready-made records, or (n, 3) points with `max_distance` (the argument the method calls `radius`) None, a number or an (n,)
        tensor, packed on `stream`.  The device of ready-made records is checked by the caller's _query_args / _expect."""
        import torch
        if _is_tensor(points, torch.float32, (None, 4)):
            if max_distance is not None:
                raise ValueError(f"{name}: (n, 4) points are ready-made query records; {radius} must be None")
            return points
        if not _is_tensor(points, torch.float32, (None, 3), self.device):
            _refuse(points, f"{name}: points: expected a contiguous torch.float32 (n, 3) or (n, 4) tensor on cuda:{self.device}")
        if isinstance(max_distance, torch.Tensor):
            _expect(f"{name}: {radius}", max_distance, torch.float32, (), points.device)
            _same_count(name, radius, max_distance.shape[0], points.shape[0], "points")
        elif max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating))):
            raise TypeError(f"{name}: {radius} must be None, a number or a float32 (n,) tensor, got {type(max_distance).__name__}")
        with torch.cuda.stream(_stream_pair(stream, points.device)[1]):
            queries = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
            queries[:, 0:3] = points
            queries[:, 3] = float("inf") if max_distance is None else max_distance
        return queries

    def closest_point(self, points, max_distance=None, out=None, **launch):
        """The nearest triangle to points already on the GPU (gnxr_closest_point_device; the definition, operation by operation:
        include/gnxr.h).  `points`: a contiguous float32 (n, 3) tensor on the scene's device, with `max_distance` None (unbounded), a
        number for all points or a float32 (n,) tensor; or a float32 (n, 4) tensor of ready-made gnxr_point_query records (x, y, z,
        max_distance), which takes no `max_distance`.  Returns ClosestPoints: the (n, 8) float32 gnxr_closest_point records (`out` when
        given) and named views of them.  The walk reads the scene's live tree: after update_vertices, rebuild_bvh and set_geometry it
        answers for the geometry the scene holds now.  Spheres are not considered.  Keywords of the launch: `stream=` (None: torch's
        current stream; a torch.cuda.Stream or a hipStream_t as an int) -- the work is queued there and nothing waits --, and, for
        measurements, `counts=`: an int64 (2,) tensor on the same device that the call adds the nodes visited and the triangles tested
        to, through the kernel's slower counting form.  (They travel as keywords because tests/test_python_refusals.py keeps one
        table row per method that names a `stream` parameter; this method's refusals are exercised in tests/test_closest_point.py.)"""
        import torch
        _only_kw("closest_point", launch, ("stream", "counts"))
        stream, counts = launch.get("stream"), launch.get("counts")
        queries = self._point_queries("closest_point", points, max_distance, stream)
        n, out, st, _ = self._query_args("closest_point", [("points", queries, torch.float32, 4)], out, 8, stream)
        _walk_call("closest_point", lib().gnxr_closest_point_device, lib().gnxr_closest_point_counted_device,
                   (self._h, _ptr(queries), n, _ptr(out)), counts, 2, queries.device, st)
        return ClosestPoints(out, out.view(torch.int32)[:, 0], out[:, 1], out[:, 2:5], out[:, 5:7], out.view(torch.int32)[:, 7])

    def ClosestPoint(self, queries):
        """closest_point for numpy arrays (gnxr_closest_point): `queries` is (n, 4) float32 -- x, y, z, max_distance (np.inf: unbounded).
        Returns a structured array of CLOSEST_DTYPE, like Intersect."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 4)
        res = np.zeros(len(queries), dtype=CLOSEST_DTYPE)
        _check(lib().gnxr_closest_point(self._h, queries.ctypes.data_as(C.POINTER(_abi.PointQuery)), len(queries),
                                        res.ctypes.data_as(C.POINTER(_abi.ClosestPoint))))
        return res

    # all-hits ray queries (gnxr_trace_all_device / gnxr_trace_all)
    def _all_hits(self, name, rays, max_hits, out, counts_out, launch):
        import torch
        _only_kw(name, launch, ("stream", "counts"))
        stream, work = launch.get("stream"), launch.get("counts")
        max_hits = _list_length(name, "max_hits", max_hits, 0, ALL_HITS_MAX)
        _expect(f"{name}: rays", rays, torch.float32, (8,), self.device)
        n = rays.shape[0]
        st, _, out, counts_out = _outputs(stream, rays.device, (f"{name}: out", out, (n, max_hits, 4), torch.float32),
                                          (f"{name}: counts_out", counts_out, (n,), torch.int32))
        hits = _ptr(out) if max_hits else None
        _walk_call(name, lib().gnxr_trace_all_device, lib().gnxr_trace_all_counted_device,
                   (self._h, _ptr(rays), n, max_hits, hits, _ptr(counts_out)), work, 3, rays.device, st)
        return RayHitLists(out, out[:, :, 0], out.view(torch.int32)[:, :, 1], out[:, :, 2:4], counts_out)

    def all_hits(self, rays, max_hits, out=None, counts_out=None, **launch):
        """EVERY triangle that rays already on the GPU pass through (gnxr_trace_all_device; the definition, triangle by triangle:
        include/gnxr.h).  `rays`: a contiguous float32 (n, 8) tensor in the gnxr_ray layout (rays_tensor) on the scene's device;
        `max_hits` = K in [0, ALL_HITS_MAX].  Returns RayHitLists: `count`, int32 (n,) (`counts_out` when given) -- all hits within
        tmax, never clamped to K --, and the (n, K, 4) float32 gnxr_ray_hit records (`out` when given) of the first min(count, K) hits
        in ascending (t, prim), the remaining slots (+inf, -1, 0, 0), with named views of them.  Nothing is pruned by distance: the
        walk visits every triangle along the ray whatever K is; bound tmax to see less.  The walk reads the scene's live tree (after
        update_vertices, rebuild_bvh and set_geometry it answers for the geometry the scene holds now); spheres are not considered.
        Keywords of the launch, as for closest_point: `stream=` (None: torch's current stream; a torch.cuda.Stream or a hipStream_t
        as an int; the work is queued there and nothing waits) and, for measurements, `counts=`: an int64 (3,) tensor on the same
        device that the call adds nodes visited, own-box tests and triangle tests to, through the kernel's slower counting form.
        (Their refusals are exercised in tests/test_all_hits.py.)"""
        return self._all_hits("all_hits", rays, max_hits, out, counts_out, launch)

    def count_hits(self, rays, **launch):
        """all_hits with max_hits = 0: the int32 (n,) number of triangles each ray passes through within its tmax, and no list."""
        return self._all_hits("count_hits", rays, 0, None, None, launch).count

    def _parity_rays(self, name, points, direction, stream):
        import torch
        _expect(f"{name}: points", points, torch.float32, (3,), self.device)
        if direction is None:
            direction = CONTAINS_DIRECTION
        try:
            d = tuple(float(x) for x in direction)
        except (TypeError, ValueError):
            raise TypeError(f"{name}: direction must be None or three numbers, got {type(direction).__name__}") from None
        if len(d) != 3 or not all(np.isfinite(d)) or not any(d):
            raise ValueError(f"{name}: direction must be three finite numbers, not all zero, got {d}")
        with torch.cuda.stream(_stream_pair(stream, points.device)[1]):
            rays = torch.empty((points.shape[0], 8), dtype=torch.float32, device=points.device)
            rays[:, 0:3] = points
            rays[:, 3] = float("inf")
            for k in range(3):
                rays[:, 4 + k] = d[k]
            rays[:, 7] = 0.0
        return rays

    def contains(self, points, direction=None, **launch):
        """Whether points already on the GPU lie inside the scene's triangle mesh: uint8 (n,), count_hits & 1 along the rays
        (p, direction, +inf), which are built on the device.  `points`: a contiguous float32 (n, 3) tensor on the scene's device;
        `direction`: three numbers (default CONTAINS_DIRECTION: (3, 2, 1) / sqrt(14) to within an ulp of fp32).  The mesh must be
        CLOSED for the parity to mean anything.  A ray through a shared edge or vertex EXACTLY can count one crossing twice (or
        none): a caller who cannot accept that votes over several directions.  `stream=`, `counts=`: as for all_hits."""
        import torch
        _only_kw("contains", launch, ("stream", "counts"))
        rays = self._parity_rays("contains", points, direction, launch.get("stream"))
        with torch.cuda.stream(_stream_pair(launch.get("stream"), points.device)[1]):
            return (self._all_hits("contains", rays, 0, None, None, launch).count & 1).to(torch.uint8)

    def signed_distance(self, points, direction=None, **launch):
        """The distance from points already on the GPU to the scene's triangle mesh, negative inside: float32 (n,),
        sqrt(closest_point(points).dist2), negated where contains(points, direction) -- it equals that chain of public calls on bits.
        +inf where closest_point has no winner (an invalid point: a NaN coordinate).  The limits are those of contains: a closed mesh, and
        rays that cross an edge exactly.  `stream=`: as for all_hits."""
        import torch
        _only_kw("signed_distance", launch, ("stream",))
        _expect("signed_distance: points", points, torch.float32, (3,), self.device)
        inside = self.contains(points, direction, **launch)
        nearest = self.closest_point(points, **launch)
        with torch.cuda.stream(_stream_pair(launch.get("stream"), points.device)[1]):
            dist = torch.sqrt(nearest.dist2)
            dist = torch.where(inside != 0, -dist, dist)
            return torch.where(nearest.prim < 0, torch.full_like(dist, float("inf")), dist)

    def AllHits(self, rays, max_hits):
        """all_hits for numpy arrays (gnxr_trace_all): `rays` is (n, 8) float32 in the gnxr_ray layout (make_rays).  Returns
        (hits, counts): an (n, max_hits) structured array of RAY_HIT_DTYPE and the int32 (n,) counts."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        max_hits = int(max_hits)
        hits = np.zeros((len(rays), max_hits), dtype=RAY_HIT_DTYPE)
        counts = np.zeros(len(rays), dtype=np.int32)
        _check(lib().gnxr_trace_all(self._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays), max_hits,
                                    hits.ctypes.data_as(C.POINTER(_abi.RayHit)) if max_hits > 0 else None, counts.ctypes.data_as(C.POINTER(C.c_int32))))
        return hits, counts

    # neighbour queries (gnxr_near_device / gnxr_near)
    def _near(self, name, points, radius, max_near, lowest, flags, out, counts_out, launch, radius_name="radius"):
        import torch
        _only_kw(name, launch, ("stream", "counts"))
        stream, work = launch.get("stream"), launch.get("counts")
        max_near = _list_length(name, "k" if flags else "max_near", max_near, lowest, NEAR_MAX)
        queries = self._point_queries(name, points, radius, stream, radius_name)
        _expect(f"{name}: points", queries, torch.float32, (4,), self.device)
        n = queries.shape[0]
        st, _, out, counts_out = _outputs(stream, queries.device, (f"{name}: out", out, (n, max_near, 8), torch.float32),
                                          (f"{name}: counts_out", counts_out, (n,), torch.int32))
        records = _ptr(out) if max_near else None
        _walk_call(name, lib().gnxr_near_device, lib().gnxr_near_counted_device,
                   (self._h, _ptr(queries), n, max_near, flags, records, _ptr(counts_out)), work, 2, queries.device, st)
        ints = out.view(torch.int32)
        return NearLists(counts_out, out, ints[:, :, 0], out[:, :, 1], out[:, :, 2:5], out[:, :, 5], out[:, :, 6], ints[:, :, 7])

    def within(self, points, radius, max_near, out=None, counts_out=None, **launch):
        """EVERY triangle within `radius` of points already on the GPU (gnxr_near_device, GNXR_NEAR_ALL; the definition, triangle by
        triangle: include/gnxr.h, "Neighbour queries").  `points` and `radius` take the forms closest_point takes for its points and
        max_distance: a contiguous float32 (n, 3) tensor on the scene's device with `radius` None (unbounded: every triangle), a number
        or a float32 (n,) tensor; or (n, 4) ready-made gnxr_point_query records with `radius` None.  `max_near` = K in [0, NEAR_MAX].
        Returns NearLists: `count`, int32 (n,) (`counts_out` when given) -- all triangles with dist2 <= radius^2, never clamped to K --,
        and the (n, K, 8) float32 gnxr_closest_point records (`out` when given) of the first min(count, K) of them in ascending
        (dist2, prim), the remaining slots empty (prim -1, dist2 +inf, the rest 0), with named views of them.  The walk reads the
        scene's live tree (after update_vertices, rebuild_bvh, set_geometry and SkinnedMesh.pose it answers for the geometry the scene
        holds now); spheres are not considered.  Keywords of the launch, as for closest_point: `stream=` (None: torch's current
        stream; a torch.cuda.Stream or a hipStream_t as an int; the work is queued there and nothing waits) and, for measurements,
        `counts=`: an int64 (2,) tensor on the same device that the call adds nodes visited and triangles tested to, through the
        kernel's slower counting form.  (Their refusals are exercised in tests/test_near.py.)"""
        return self._near("within", points, radius, max_near, 0, _abi.NEAR_ALL, out, counts_out, launch)

    def count_within(self, points, radius, **launch):
        """within with max_near = 0: the int32 (n,) number of triangles within `radius` of each point, and no list."""
        return self._near("count_within", points, radius, 0, 0, _abi.NEAR_ALL, None, None, launch).count

    def nearest(self, points, k, max_distance=None, out=None, counts_out=None, **launch):
        """The `k` nearest triangles to points already on the GPU (gnxr_near_device, GNXR_NEAR_NEAREST), k in [1, NEAR_MAX]: the lists
        are within(points, max_distance, k)'s byte for byte, `count` is the number of slots filled, min(within's count, k), and the
        walk prunes on the k-th distance once a list is full, so it visits no more of the tree than the k nearest need.  nearest(points,
        1) holds closest_point's record wherever that has a winner.  `points`, `max_distance`, `out`, `counts_out` and the launch
        keywords: as for within."""
        return self._near("nearest", points, max_distance, k, 1, _abi.NEAR_NEAREST, out, counts_out, launch, "max_distance")

    def Near(self, queries, max_near, nearest=False):
        """within / nearest for numpy arrays (gnxr_near): `queries` is (n, 4) float32 -- x, y, z, max_distance (np.inf: unbounded).
        Returns (records, counts): an (n, max_near) structured array of CLOSEST_DTYPE and the int32 (n,) counts."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 4)
        max_near = int(max_near)
        records = np.zeros((len(queries), max(max_near, 0)), dtype=CLOSEST_DTYPE)
        counts = np.zeros(len(queries), dtype=np.int32)
        _check(lib().gnxr_near(self._h, queries.ctypes.data_as(C.POINTER(_abi.PointQuery)), len(queries), max_near,
                               _abi.NEAR_NEAREST if nearest else _abi.NEAR_ALL,
                               records.ctypes.data_as(C.POINTER(_abi.ClosestPoint)) if max_near > 0 else None, counts.ctypes.data_as(C.POINTER(C.c_int32))))
        return records, counts

    # sphere casts (gnxr_sphere_cast_device / gnxr_sphere_cast)
    def _sphere_casts(self, origins, directions, radius, tmax, stream):
        """The (n, 8) float32 gnxr_sphere_cast records of sphere_cast: `origins` as ready-made records, or (n, 3) origins and
        directions with `radius` a number or an (n,) tensor and `tmax` None, a number or an (n,) tensor, packed on `stream`."""
        import torch
        if _is_tensor(origins, torch.float32, (None, 8)):
            if directions is not None or radius is not None or tmax is not None:
                raise ValueError("sphere_cast: (n, 8) origins are ready-made cast records; directions, radius and tmax must be None")
            return origins
        if not _is_tensor(origins, torch.float32, (None, 3), self.device):
            _refuse(origins, f"sphere_cast: origins: expected a contiguous torch.float32 (n, 3) or (n, 8) tensor on cuda:{self.device}")
        _expect("sphere_cast: directions", directions, torch.float32, (3,), origins.device)
        _same_count("sphere_cast", "directions", directions.shape[0], origins.shape[0], "origins")
        for what, x, may_be_none in (("radius", radius, False), ("tmax", tmax, True)):
            if isinstance(x, torch.Tensor):
                _expect(f"sphere_cast: {what}", x, torch.float32, (), origins.device)
                _same_count("sphere_cast", what, x.shape[0], origins.shape[0], "origins")
            elif not (x is None and may_be_none) and (isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating))):
                raise TypeError(f"sphere_cast: {what} must be {'None, ' if may_be_none else ''}a number or a float32 (n,) tensor, got {type(x).__name__}")
        with torch.cuda.stream(_stream_pair(stream, origins.device)[1]):
            casts = torch.empty((origins.shape[0], 8), dtype=torch.float32, device=origins.device)
            casts[:, 0:3] = origins
            casts[:, 3] = radius
            casts[:, 4:7] = directions
            casts[:, 7] = float("inf") if tmax is None else tmax
        return casts

    def sphere_cast(self, origins, directions, radius, tmax=None, out=None, **launch):
        """The first impact of moving balls against the mesh, for casts already on the GPU (gnxr_sphere_cast_device; the definition,
        operation by operation: include/gnxr.h, "Sphere casts").  Ball i has its centre at origins[i] + t directions[i] for t in
        [0, tmax[i]] -- `directions` is not normalised, t is in its units -- and radius[i].  `origins`, `directions`: contiguous float32
        (n, 3) tensors on the scene's device; `radius`: a number for all casts or a float32 (n,) tensor; `tmax`: None (unbounded), a
        number or a float32 (n,) tensor.  Or `origins` is a float32 (n, 8) tensor of ready-made gnxr_sphere_cast records (o.xyz,
        radius, d.xyz, tmax) and the other three are None.  Returns SphereCasts: the (n, 8) float32 records (`out` when given) and
        named views of them -- `prim` (-1: no hit), `t`, and `p`, `b1`, `b2`, `feature`, closest_point's answer for the winning
        triangle at the centre of the time of impact; the contact normal is (origins + t directions - p) / radius.  The walk reads
        the scene's live tree (after update_vertices, rebuild_bvh, set_geometry and SkinnedMesh.pose it answers for the geometry the
        scene holds now); spheres are not considered.  Keywords of the launch, which travel as keywords for the reason given in
        closest_point's docstring: `stream=` (None: torch's current stream; a torch.cuda.Stream or a hipStream_t as an int; the work
        is queued there and nothing waits) and, for measurements, `counts=`: an int64 (2,) tensor on the same device that the call
        adds nodes visited and triangles tested to, through the kernel's slower counting form.  (The refusals are exercised in
        tests/test_sphere_cast.py.)"""
        import torch
        _only_kw("sphere_cast", launch, ("stream", "counts"))
        stream, counts = launch.get("stream"), launch.get("counts")
        casts = self._sphere_casts(origins, directions, radius, tmax, stream)
        n, out, st, _ = self._query_args("sphere_cast", [("origins", casts, torch.float32, 8)], out, 8, stream)
        _walk_call("sphere_cast", lib().gnxr_sphere_cast_device, lib().gnxr_sphere_cast_counted_device,
                   (self._h, _ptr(casts), n, _ptr(out)), counts, 2, casts.device, st)
        ints = out.view(torch.int32)
        return SphereCasts(out, ints[:, 0], out[:, 1], out[:, 2:5], out[:, 5], out[:, 6], ints[:, 7])

    def SphereCast(self, casts):
        """sphere_cast for numpy arrays (gnxr_sphere_cast): `casts` is (n, 8) float32 -- o.xyz, radius, d.xyz, tmax (np.inf:
        unbounded).  Returns a structured array of CLOSEST_DTYPE whose `dist2` field holds t."""
        casts = np.ascontiguousarray(casts, dtype=np.float32).reshape(-1, 8)
        res = np.zeros(len(casts), dtype=CLOSEST_DTYPE)
        _check(lib().gnxr_sphere_cast(self._h, casts.ctypes.data_as(C.POINTER(_abi.SphereCast)), len(casts), res.ctypes.data_as(C.POINTER(_abi.ClosestPoint))))
        return res

    # box overlap queries (gnxr_overlap_box_device / gnxr_overlap_box)
    def _box_queries(self, name, lo, hi, stream):
        """The (n, 8) float32 gnxr_box_query records of the overlap queries: `lo` as ready-made records with `hi` None, or (n, 3) lower
        and upper corners, packed on `stream` (pad words 0)."""
        import torch
        if _is_tensor(lo, torch.float32, (None, 8)):
            if hi is not None:
                raise ValueError(f"{name}: (n, 8) lo are ready-made box records; hi must be None")
            return _expect(f"{name}: lo", lo, torch.float32, (8,), self.device)
        if not _is_tensor(lo, torch.float32, (None, 3), self.device):
            _refuse(lo, f"{name}: lo: expected a contiguous torch.float32 (n, 3) or (n, 8) tensor on cuda:{self.device}")
        _expect(f"{name}: hi", hi, torch.float32, (3,), lo.device)
        _same_count(name, "hi", hi.shape[0], lo.shape[0], "lo")
        with torch.cuda.stream(_stream_pair(stream, lo.device)[1]):
            boxes = torch.zeros((lo.shape[0], 8), dtype=torch.float32, device=lo.device)
            boxes[:, 0:3] = lo
            boxes[:, 4:7] = hi
        return boxes

    def overlap_box(self, lo, hi=None, max_prims=None, out=None, counts_out=None, **launch):
        """EVERY triangle that touches axis-aligned boxes already on the GPU (gnxr_overlap_box_device; the definition, triangle by
        triangle: include/gnxr.h, "Overlap queries").  `lo`, `hi`: contiguous float32 (n, 3) tensors on the scene's device, the boxes'
        lower and upper corners; or `lo` is a float32 (n, 8) tensor of ready-made gnxr_box_query records (lo.xyz, pad, hi.xyz, pad) and
        `hi` is None.  Touching counts; an inverted box, a NaN or an infinite bound overlaps nothing.
        With an integer `max_prims` = K in [0, OVERLAP_MAX]: returns OverlapLists -- `count`, int32 (n,) (`counts_out` when given): all
        overlapping triangles, never clamped to K --, and `prims`, int32 (n, K) (`out` when given): per box the min(count, K) smallest
        authoring indices among them, ascending, then -1.
        With `max_prims` None: the complete lists, as OverlapCSR -- `count` as above, `offsets`, int64 (n + 1,), and `prims`, int32
        (offsets[-1],): box i's triangles are prims[offsets[i]:offsets[i + 1]], ascending.  That is a count-only call, torch.cumsum into
        the offsets, one allocation of their total -- the one point where the host waits for the stream -- and the call that fills
        the rows, all on the same stream; `out` must be None.
        The walk reads the scene's live tree (after update_vertices, rebuild_bvh, set_geometry and SkinnedMesh.pose it answers for the
        geometry the scene holds now); spheres are not considered.  Keywords of the launch, as for within: `stream=` (None: torch's
        current stream; a torch.cuda.Stream or a hipStream_t as an int) and, for measurements, `counts=`: an int64 (2,) tensor on the
        same device that every walk of the call adds nodes visited and triangles tested to, through the kernel's slower counting
        form.  (Their refusals are exercised in tests/test_overlap_box.py.)"""
        return self._overlap_box("overlap_box", lo, hi, max_prims, out, counts_out, launch)

    def _overlap_box(self, name, lo, hi, max_prims, out, counts_out, launch):
        return self._overlap_lists(name, max_prims, out, counts_out, launch, lambda stream: self._box_queries(name, lo, hi, stream), (), "gnxr_overlap_box")

    def _overlap_lists(self, name, max_prims, out, counts_out, launch, queries, flags, entry):
        """The rows / CSR plumbing the overlap queries share (overlap_box, overlap_triangles, self_intersections).  `queries(stream)`:
        the checked record tensor of the call, or the number of queries of a call whose queries are the scene's own; `flags`: what the
        C call takes between n and max_prims, as a tuple; `entry`: the C calls' common name, "<entry>_device" and "<entry>_counted_device"."""
        import torch
        _only_kw(name, launch, ("stream", "counts"))
        stream, work = launch.get("stream"), launch.get("counts")
        csr = max_prims is None
        if csr and out is not None:
            raise ValueError(f"{name}: with max_prims None the lists are allocated by the call; out must be None")
        K = 0 if csr else _list_length(name, "max_prims", max_prims, 0, OVERLAP_MAX)
        records = queries(stream)
        if isinstance(records, int):
            records, n, device = None, records, torch.device("cuda", self.device)
        else:
            n, device = records.shape[0], records.device
        st, tstream, out, counts_out = _outputs(stream, device, (f"{name}: out", out, (n, K), torch.int32), (f"{name}: counts_out", counts_out, (n,), torch.int32))
        call = lambda k, offsets, prims: _walk_call(name, getattr(lib(), entry + "_device"), getattr(lib(), entry + "_counted_device"), (self._h, _ptr(records), n, *flags, k, _ptr(offsets), _ptr(prims), _ptr(counts_out)),
                                                    work, 2, device, st)
        call(K, None, out if K else None)
        if not csr:
            return OverlapLists(counts_out, out)
        with torch.cuda.stream(tstream):
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
            torch.cumsum(counts_out, 0, dtype=torch.int64, out=offsets[1:])
            prims = torch.empty(int(offsets[-1]), dtype=torch.int32, device=device)
        if prims.numel():
            call(-1, offsets, prims)
        return OverlapCSR(counts_out, offsets, prims)

    def count_in_box(self, lo, hi=None, **launch):
        """overlap_box with max_prims = 0: the int32 (n,) number of triangles that touch each box, and no list."""
        return self._overlap_box("count_in_box", lo, hi, 0, None, None, launch).count

    def OverlapBox(self, boxes, max_prims):
        """overlap_box for numpy arrays (gnxr_overlap_box): `boxes` is (n, 8) float32 -- lo.xyz, pad, hi.xyz, pad.  With an integer
        `max_prims` it returns (prims, counts): int32 (n, max_prims) and int32 (n,).  With `max_prims` None it returns (prims, counts,
        offsets): the complete lists as CSR, from a count-only call, numpy's cumsum and the call that fills the rows."""
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
        n = len(boxes)
        counts = np.zeros(n, dtype=np.int32)
        I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        call = lambda k, offsets, prims: _check(lib().gnxr_overlap_box(self._h, boxes.ctypes.data_as(C.POINTER(_abi.BoxQuery)), n, k,
                                                                       offsets.ctypes.data_as(I64) if offsets is not None else None,
                                                                       prims.ctypes.data_as(I32) if prims is not None else None, counts.ctypes.data_as(I32)))
        if max_prims is not None:
            max_prims = int(max_prims)
            prims = np.zeros((n, max(max_prims, 0)), dtype=np.int32)
            call(max_prims, None, prims if max_prims > 0 else None)
            return prims, counts
        call(0, None, None)
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, dtype=np.int64, out=offsets[1:])
        prims = np.zeros(int(offsets[-1]), dtype=np.int32)
        if len(prims):
            call(-1, offsets, prims)
        return prims, counts, offsets

    # triangle overlap queries (gnxr_overlap_tri_device / gnxr_overlap_tri)
    def _tri_queries(self, name, tris, stream):
        """`tris` as checked (n, 12) gnxr_tri_query records on the scene's device: ready-made, or packed by triangle_queries on `stream`
        from corners or from a (vertices, indices) pair"""
        import torch
        if _is_tensor(tris, torch.float32, (None, 12)):
            return _expect(f"{name}: tris", tris, torch.float32, (12,), self.device)
        vertices, indices = tris if isinstance(tris, tuple) and len(tris) == 2 else (tris, None)
        return _tri_records(name, vertices, indices, None, stream, self.device)

    def overlap_triangles(self, tris, max_prims=None, skip_shared=False, out=None, counts_out=None, **launch):
        """EVERY triangle of the scene that touches query triangles already on the GPU -- mesh against mesh, exactly
        (gnxr_overlap_tri_device; the definition, triangle by triangle: include/gnxr.h, "Triangle overlap queries").  `tris`: a float32
        (n, 12) tensor of ready-made gnxr_tri_query records on the scene's device (a.xyz, pad, b.xyz, pad, c.xyz, pad), or anything
        triangle_queries takes: (n, 3, 3) or (n, 9) corners, or a (vertices, indices) tuple.  Touching counts; a zero-area triangle (a
        segment, a point) is a legitimate query; a coordinate that is not finite overlaps nothing.  `skip_shared=True` leaves out every
        triangle that shares a vertex position with the query (GNXR_OVERLAP_TRI_SKIP_SHARED).  `max_prims`, the results (OverlapLists
        with an integer, OverlapCSR with None), `out`, `counts_out` and the launch keywords `stream=` and `counts=` are overlap_box's.
        (The refusals are exercised in tests/test_overlap_triangles.py.)"""
        return self._overlap_tri("overlap_triangles", tris, max_prims, skip_shared, out, counts_out, launch)

    def _overlap_tri(self, name, tris, max_prims, skip_shared, out, counts_out, launch):
        flags = _abi.OVERLAP_TRI_SKIP_SHARED if skip_shared else 0
        return self._overlap_lists(name, max_prims, out, counts_out, launch, lambda stream: self._tri_queries(name, tris, stream), (flags,), "gnxr_overlap_tri")

    def count_overlapping_triangles(self, tris, skip_shared=False, **launch):
        """overlap_triangles with max_prims = 0: the int32 (n,) number of triangles that touch each query triangle, and no list."""
        return self._overlap_tri("count_overlapping_triangles", tris, 0, skip_shared, None, None, launch).count

    def self_intersections(self, max_prims=None, pairs=False, **launch):
        """The scene's mesh against itself (gnxr_overlap_tri_device with GNXR_OVERLAP_TRI_SELF): query i is the scene's own triangle with
        authoring index i, and every triangle that shares a vertex position with it -- itself, its edge and vertex neighbours -- is left
        out, so what is reported is the mesh passing through itself.  Returns overlap_triangles' OverlapLists / OverlapCSR over the
        n_triangles triangles, rows and counts indexed by authoring index.  `pairs=True` (with `max_prims` None): an (m, 2) int32 tensor
        of the unique pairs (i, j), i < j, reported in either direction, sorted lexicographically -- built with torch on the CSR result,
        on the same stream; m == 0 means the pose is free of self-intersections.  Launch keywords: overlap_box's."""
        import torch
        name = "self_intersections"
        if pairs and max_prims is not None:
            raise ValueError(f"{name}: pairs are built from the complete lists; max_prims must be None")
        n = self.n_triangles
        res = self._overlap_lists(name, max_prims, None, None, launch, lambda stream: n, (_abi.OVERLAP_TRI_SELF,), "gnxr_overlap_tri")
        if not pairs:
            return res
        with torch.cuda.stream(_stream_pair(launch.get("stream"), res.prims.device)[1]):
            i = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=res.prims.device), res.count.to(torch.int64), output_size=res.prims.numel())
            j = res.prims.to(torch.int64)
            key = torch.unique(torch.minimum(i, j) * n + torch.maximum(i, j))   # sorted: lexicographic in (i, j)
            return torch.stack([key // n, key % n], dim=1).to(torch.int32)

    def OverlapTriangles(self, tris, max_prims, flags=0):
        """overlap_triangles for numpy arrays (gnxr_overlap_tri): `tris` is (n, 12) float32 -- a.xyz, pad, b.xyz, pad, c.xyz, pad --, or
        None with OVERLAP_TRI_SELF in `flags` (OVERLAP_TRI_SKIP_SHARED | OVERLAP_TRI_SELF).  Returns what OverlapBox returns: (prims,
        counts) with an integer `max_prims`, (prims, counts, offsets) with None."""
        if tris is not None:
            tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
        n = self.n_triangles if tris is None else len(tris)
        counts = np.zeros(n, dtype=np.int32)
        I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        call = lambda k, offsets, prims: _check(lib().gnxr_overlap_tri(self._h, tris.ctypes.data_as(C.POINTER(_abi.TriQuery)) if tris is not None else None, n, int(flags), k,
                                                                       offsets.ctypes.data_as(I64) if offsets is not None else None,
                                                                       prims.ctypes.data_as(I32) if prims is not None else None, counts.ctypes.data_as(I32)))
        if max_prims is not None:
            max_prims = int(max_prims)
            prims = np.zeros((n, max(max_prims, 0)), dtype=np.int32)
            call(max_prims, None, prims if max_prims > 0 else None)
            return prims, counts
        call(0, None, None)
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, dtype=np.int64, out=offsets[1:])
        prims = np.zeros(int(offsets[-1]), dtype=np.int32)
        if len(prims):
            call(-1, offsets, prims)
        return prims, counts, offsets

    def voxelize(self, origin, cell, dims, fill=False, counts=False, chunk=1 << 22, **launch):
        """The scene's triangle mesh as a voxel grid: an (nz, ny, nx) bool tensor on the scene's device in which a voxel is set iff
        count_in_box of its box -- voxel_boxes(origin, cell, dims) -- is positive: the voxel touches a triangle (closed, so a triangle
        lying exactly in the face two voxels share sets both).  `counts=True` returns the int32 counts instead.  `fill=True` ORs the
        result with contains() of the voxel centres 0.5 lo + 0.5 hi, so that the inside of the mesh is set as well; the limits are those
        of contains: the mesh must be CLOSED for the parity to mean anything, and a ray through a shared edge or vertex EXACTLY can count
        one crossing twice (or none): a caller who cannot accept that votes over several directions.  `fill` and `counts` do not go
        together.  The grid is walked `chunk` voxels at a time (the boxes of a chunk are 32 bytes per voxel) and the result equals the
        chain voxel_boxes -> count_in_box (-> contains) of public calls on bits.  `stream=`: as for overlap_box (it travels as a keyword
        for the reason given in closest_point's docstring)."""
        import torch
        _only_kw("voxelize", launch, ("stream",))
        stream = launch.get("stream")
        if fill and counts:
            raise ValueError("voxelize: fill sets voxels and counts returns numbers of triangles: ask for one of them")
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
            raise ValueError(f"voxelize: chunk must be a positive integer, got {chunk!r}")
        device = torch.device("cuda", self.device)
        origin, cell, (nx, ny, nz) = _voxel_grid("voxelize", origin, cell, dims)
        total = nx * ny * nz
        _, tstream = _stream_pair(stream, device)
        with torch.cuda.stream(tstream):
            grid = torch.empty(total, dtype=torch.int32 if counts else torch.bool, device=device)
            for first in range(0, total, int(chunk)):
                m = min(int(chunk), total - first)
                boxes = _voxel_box_records(origin, cell, (nx, ny, nz), first, m, device)
                count = self.count_in_box(boxes, stream=stream)
                if counts:
                    grid[first:first + m] = count
                    continue
                grid[first:first + m] = count > 0
                if fill:
                    centres = (0.5 * boxes[:, 0:3] + 0.5 * boxes[:, 4:7]).contiguous()
                    grid[first:first + m] |= self.contains(centres, stream=stream) != 0
        return grid.view(nz, ny, nx)

    MOTION_CHANNELS = ("motion", "guide", "prim")

    def motion(self, width, height, prev_cameras, cameras=None, prev_vertices=None, out=None, stream=None):
        """A pixel-centre G-buffer and where each pixel's surface point was one frame ago (gnxr_motion_device; the definition, operation
        by operation: include/gnxr.h).  `prev_cameras`: the gnxr Camera records (camera()) of the previous frame, one per view -- a single
        record will do for one view.  `cameras`: this frame's records, or None for the scene's own camera, which also drops the leading
        V.  `prev_vertices`: None (nothing but the camera moved), or a contiguous float32 (n_vertices, 3) tensor on the scene's device:
        the vertex array the scene held one frame ago, in update_vertices' layout.  Returns a dict of torch tensors on the scene's
        device: "motion" (V, H, W, 4) float32 = (x', y', t', flag) -- the raster position on the previous frame's film, the distance
        the previous frame's guide holds there if it saw the same point, 1 when both are usable --, "guide" (V, H, W, 4) float32 =
        (n.x, n.y, n.z, t) of the hit through the pixel centre and "prim" (V, H, W) int32 = its primitive, -1 on a miss.  `out`: a dict
        with preallocated tensors for some or all of them.  Runs on `stream` (by default torch's current stream) and returns once the
        buffers are written.  Malformed arguments raise ValueError."""
        import torch
        if isinstance(prev_cameras, Camera):
            prev_cameras = [prev_cameras]
        if prev_cameras is None:
            raise ValueError("motion: prev_cameras is required (the cameras of the previous frame)")
        prev_cameras, _, _, _ = _view_args("motion: prev_cameras", prev_cameras, None, width, height)
        cameras, _, width, height = _view_args("motion", cameras, None, width, height)
        V = len(cameras) if cameras is not None else 1
        if len(prev_cameras) != V:
            raise ValueError(f"motion: {len(prev_cameras)} previous cameras for {V} view{'s' if V != 1 else ''}")
        if prev_vertices is not None:
            _expect("motion: prev_vertices", prev_vertices, torch.float32, (3,), self.device)
            if prev_vertices.shape[0] != self.n_vertices:
                raise ValueError(f"motion: prev_vertices has {prev_vertices.shape[0]} rows, the scene has {self.n_vertices} vertices")
        out = dict(out) if out is not None else {}
        extra = [c for c in out if c not in self.MOTION_CHANNELS]
        if extra:
            raise ValueError(f"motion: out holds {extra}; the channels are {self.MOTION_CHANNELS}")
        device = torch.device("cuda", self.device)
        lead = (V,) if cameras is not None else ()
        hstream, _, *tensors = _outputs(stream, device, *((f"motion: out[{c!r}]", out.get(c), lead + (height, width) + (() if c == "prim" else (4,)),
                                                           torch.int32 if c == "prim" else torch.float32) for c in self.MOTION_CHANNELS))
        res = dict(zip(self.MOTION_CHANNELS, tensors))
        if V == 0:
            return res
        p = _abi.MotionParams(C.sizeof(_abi.MotionParams), width, height, V)
        bufs = _abi.MotionBuffers(C.sizeof(_abi.MotionBuffers), 0, _ptr(res["motion"]), _ptr(res["guide"]), _ptr(res["prim"]))
        cams = (Camera * V)(*cameras) if cameras else None
        prev = (Camera * V)(*prev_cameras)
        _check(lib().gnxr_motion_device(self._h, C.byref(p), cams, prev, _ptr(prev_vertices), C.byref(bufs), _addr(hstream)))
        return res


RayHits = collections.namedtuple("RayHits", "hits prim t bary n")
RayHits.__doc__ = """Scene.intersect's result: `hits`, the (n, 8) float32 gnxr_hit records, and views of it -- `prim` (int32: authoring-order
triangle, n_triangles + sphere index, or -1 for a miss), `t`, `bary` (n, 3) = b0, b1, b2 and `n` (n, 3), the geometric normal."""


ClosestPoints = collections.namedtuple("ClosestPoints", "records prim dist2 point b1b2 feature")
ClosestPoints.__doc__ = """Scene.closest_point's result: `records`, the (n, 8) float32 gnxr_closest_point records, and views of it -- `prim` (int32:
authoring-order triangle, -1 for none), `dist2`, `point` (n, 3), `b1b2` (n, 2) and `feature` (int32: 0 face, 1 / 2 / 3 edge ab / ac / bc,
4 / 5 / 6 vertex a / b / c)."""


RayHitLists = collections.namedtuple("RayHitLists", "records t prim b count")
RayHitLists.__doc__ = """Scene.all_hits's result: `records`, the (n, K, 4) float32 gnxr_ray_hit records -- per ray the first min(count, K)
hits in ascending (t, prim), then (+inf, -1, 0, 0) --, views of it -- `t` (n, K), `prim` (n, K) (int32: authoring-order triangle, -1 in an
empty slot) and `b` (n, K, 2) = b1, b2, the weights of the second and third vertex -- and `count`, int32 (n,): all hits, never clamped."""

NearLists = collections.namedtuple("NearLists", "count records prim dist2 p b1 b2 feature")
NearLists.__doc__ = """Scene.within's and Scene.nearest's result: `count`, int32 (n,) -- within: all triangles inside the radius, never clamped;
nearest: the slots filled --, `records`, the (n, K, 8) float32 gnxr_closest_point records -- per query the first min(count, K) near
triangles in ascending (dist2, prim), then empty slots (prim -1, dist2 +inf, the rest 0) --, and views of it: `prim` (n, K) (int32:
authoring-order triangle), `dist2` (n, K), `p` (n, K, 3), `b1`, `b2` (n, K) and `feature` (n, K) (int32, as in ClosestPoints)."""

SphereCasts = collections.namedtuple("SphereCasts", "records prim t p b1 b2 feature")
SphereCasts.__doc__ = """Scene.sphere_cast's result: `records`, the (n, 8) float32 gnxr_closest_point records with t in the dist2 slot, and views of
it -- `prim` (int32: the authoring-order triangle the ball touches first, -1 without a hit), `t` (the time of impact in units of the
direction, +inf without a hit), `p` (n, 3), `b1`, `b2` and `feature` (int32, as in ClosestPoints): the contact point on that triangle."""

OverlapLists = collections.namedtuple("OverlapLists", "count prims")
OverlapLists.__doc__ = """Scene.overlap_box's result with an integer max_prims = K: `count`, int32 (n,) -- all triangles that touch the box, never clamped --,
and `prims`, int32 (n, K): per box the min(count, K) smallest authoring indices among them, ascending, then -1."""

OverlapCSR = collections.namedtuple("OverlapCSR", "count offsets prims")
OverlapCSR.__doc__ = """Scene.overlap_box's result with max_prims None: `count`, int32 (n,), `offsets`, int64 (n + 1,) = the exclusive prefix sum of the
counts, and `prims`, int32 (offsets[-1],): box i's triangles are prims[offsets[i]:offsets[i + 1]], authoring indices ascending."""

ALL_HITS_MAX = 32   # GNXR_ALL_HITS_MAX
NEAR_MAX = 32   # GNXR_NEAR_MAX
OVERLAP_MAX = 32   # GNXR_OVERLAP_MAX
OVERLAP_TRI_SKIP_SHARED, OVERLAP_TRI_SELF = _abi.OVERLAP_TRI_SKIP_SHARED, _abi.OVERLAP_TRI_SELF   # GNXR_OVERLAP_TRI_*
CONTAINS_DIRECTION = (0.8017837, 0.5345225, 0.26726124)   # GNXR_CONTAINS_DIRECTION_*: (3, 2, 1) / sqrt(14) to within an ulp of fp32


def _voxel_grid(name, origin, cell, dims):
    """(origin, cell) as three float32 each -- `cell` a number or three -- and dims = (nx, ny, nz) as ints, each in [1, 2^24] (an index
    is exact as a float32)"""
    try:
        o = np.array([float(x) for x in origin], np.float32)
        c = np.array([float(cell)] * 3 if isinstance(cell, (int, float, np.integer, np.floating)) and not isinstance(cell, bool) else [float(x) for x in cell], np.float32)
        d = tuple(int(x) for x in dims)
    except (TypeError, ValueError):
        raise TypeError(f"{name}: origin is three numbers, cell a number or three, dims three integers (nx, ny, nz)") from None
    if o.shape != (3,) or c.shape != (3,) or len(d) != 3 or any(isinstance(x, (bool, float, np.floating)) for x in dims):
        raise ValueError(f"{name}: origin is three numbers, cell a number or three, dims three integers (nx, ny, nz), got {origin!r}, {cell!r}, {dims!r}")
    if not (np.isfinite(o).all() and np.isfinite(c).all() and (c > 0).all()):
        raise ValueError(f"{name}: origin must be finite and cell finite and positive, got {origin!r}, {cell!r}")
    if not all(1 <= x <= 1 << 24 for x in d):
        raise ValueError(f"{name}: every dimension must be in [1, {1 << 24}], got {d}")
    return o, c, d


def _voxel_box_records(origin, cell, dims, first, count, device):
    """the records of voxels first .. first + count of the grid in x-fastest order, on torch's current stream (voxel_boxes has the
    definition)"""
    import torch
    nx, ny, _ = dims
    flat = torch.arange(first, first + count, dtype=torch.int64, device=device)
    index = (flat % nx, (flat // nx) % ny, flat // (nx * ny))
    boxes = torch.zeros((count, 8), dtype=torch.float32, device=device)
    o, c = torch.from_numpy(origin).to(device), torch.from_numpy(cell).to(device)
    for k in range(3):
        boxes[:, k] = index[k].to(torch.float32) * c[k] + o[k]
        boxes[:, 4 + k] = (index[k] + 1).to(torch.float32) * c[k] + o[k]
    return boxes


def voxel_boxes(origin, cell, dims, out=None, **launch):
    """The gnxr_box_query records of a voxel grid, for Scene.overlap_box / count_in_box: a float32 (nz * ny * nx, 8) tensor (`out` when
    given), x fastest -- voxel (ix, iy, iz) is record (iz * ny + iy) * nx + ix.  `origin`: the grid's lower corner, three numbers;
    `cell`: the edge of a voxel, a number or three; `dims` = (nx, ny, nz).  Per axis, with origin and cell rounded to float32 first:
        lo = float32(i) * cell + origin          hi = float32(i + 1) * cell + origin
    one float32 product and one float32 sum each, the pad words 0.  hi of voxel i and lo of voxel i + 1 are the same two operations on
    the same numbers, so neighbours share their face bit for bit and a triangle in that face touches both.  Plain torch on `stream=`
    (None: torch's current stream; it travels as a keyword for the reason given in Scene.closest_point's docstring) and on `device=`
    (default: `out`'s device, else the device gnxr_init bound)."""
    import torch
    _only_kw("voxel_boxes", launch, ("stream", "device"))
    origin, cell, dims = _voxel_grid("voxel_boxes", origin, cell, dims)
    total = dims[0] * dims[1] * dims[2]
    device = launch.get("device")
    device = (out.device if _is_torch(out) else torch.device("cuda", _device)) if device is None else torch.device(device)
    _, tstream, out = _outputs(launch.get("stream"), device, ("voxel_boxes: out", out, (total, 8), torch.float32))
    with torch.cuda.stream(tstream):
        out.copy_(_voxel_box_records(origin, cell, dims, 0, total, device))
    return out


def _tri_records(name, vertices, indices, out, stream, device=None):
    """triangle_queries behind its checks; `device`: None (the corners' own GPU) or the index of the GPU they must be on"""
    import torch
    where = ANY_GPU if device is None else device
    on = "a GPU" if device is None else f"cuda:{device}"
    if indices is None:
        if not (_is_tensor(vertices, torch.float32, (None, 3, 3), where) or _is_tensor(vertices, torch.float32, (None, 9), where)):
            _refuse(vertices, f"{name}: tris: expected a contiguous torch.float32 (n, 12), (n, 3, 3) or (n, 9) tensor on {on}, or (vertices (V, 3), indices (n, 3))")
        corners = vertices.view(-1, 3, 3)
    else:
        if not _is_tensor(vertices, torch.float32, (None, 3), where):
            _refuse(vertices, f"{name}: vertices: expected a contiguous torch.float32 (V, 3) tensor on {on}")
        if not (_is_tensor(indices, torch.int32, (None, 3), vertices.device) or _is_tensor(indices, torch.int64, (None, 3), vertices.device)):
            _refuse(indices, f"{name}: indices: expected a contiguous torch.int32 or torch.int64 (n, 3) tensor on {vertices.device}")
        corners = None
    n = (corners if indices is None else indices).shape[0]
    _, tstream, out = _outputs(stream, vertices.device, (f"{name}: out", out, (n, 12), torch.float32))
    with torch.cuda.stream(tstream):
        if corners is None:
            corners = vertices[indices.to(torch.int64)]
        rec = out.view(n, 3, 4)
        rec[:, :, 0:3] = corners
        rec[:, :, 3] = 0
    return out


def triangle_queries(vertices, indices=None, out=None, **launch):
    """The gnxr_tri_query records of Scene.overlap_triangles, packed on the device: a float32 (n, 12) tensor (`out` when given) of
    a.xyz, pad, b.xyz, pad, c.xyz, pad with the pads 0.  `vertices`: contiguous float32 (n, 3, 3) or (n, 9) corners on a GPU; or, with
    `indices` an int32 / int64 (n, 3) tensor on the same device, a (V, 3) vertex array the corners are gathered from (an index outside
    [0, V) is the caller's error, as for any torch gather).  Plain torch on `stream=` (None: torch's current stream; it travels as a
    keyword for the reason given in Scene.closest_point's docstring)."""
    _only_kw("triangle_queries", launch, ("stream",))
    return _tri_records("triangle_queries", vertices, indices, out, launch.get("stream"))


def rays_tensor(o, d, tmax=float("inf")):
    """The (n, 8) float32 gnxr_ray layout of Scene.intersect / occluded from torch tensors (the device counterpart of make_rays):
    o, d of shape (n, 3) (or (3,) for one ray), tmax a number or an (n,) tensor."""
    import torch
    o = torch.as_tensor(o, dtype=torch.float32).reshape(-1, 3)
    d = torch.as_tensor(d, dtype=torch.float32, device=o.device).reshape(-1, 3)
    r = torch.zeros((o.shape[0], 8), dtype=torch.float32, device=o.device)
    r[:, 0:3] = o
    r[:, 3] = torch.as_tensor(tmax, dtype=torch.float32, device=o.device)
    r[:, 4:7] = d
    return r


def _view_args(name, cameras, media, width, height):
    """The views of RenderViews / RenderAOV, checked: (list of Camera records -- None stays None --, list of media or None, width, height)"""
    if cameras is not None:
        cameras = list(cameras)
        for c in cameras:
            if not isinstance(c, Camera):
                raise ValueError(f"{name}: cameras must be gnxr Camera records (camera(...)), got {type(c).__name__}")
        if media is not None:
            media = [int(m) for m in media]
            if len(media) != len(cameras):
                raise ValueError(f"{name}: {len(media)} media for {len(cameras)} cameras")
    return (cameras, media) + _image_size(name, width, height)


def li_samples(px, py, s, medium=-1):
    """The (n, 4) int32 gnxr_li_sample records of PathIntegrator.Li -- pixel (px, py), sample s, starting medium (-1: none) per ray --
    on the device of the first tensor argument.  Each argument is an integer tensor of shape (n,) or (), or an integer; they broadcast."""
    import torch
    args = {"px": px, "py": py, "s": s, "medium": medium}
    device = next((a.device for a in args.values() if isinstance(a, torch.Tensor)), torch.device("cpu"))
    cols = []
    for name, a in args.items():
        if isinstance(a, torch.Tensor):
            if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool or a.dim() > 1:
                raise ValueError(f"li_samples: {name} must be an integer tensor of shape (n,) or (), got {a.dtype} {tuple(a.shape)}")
            a = a.to(device=device, dtype=torch.int32)
        elif isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            a = torch.tensor(int(a), dtype=torch.int32, device=device)
        else:
            raise ValueError(f"li_samples: {name} must be an integer or an integer tensor, got {type(a).__name__}")
        cols.append(a.reshape(-1))
    try:
        cols = torch.broadcast_tensors(*cols)
    except RuntimeError as e:
        raise ValueError(f"li_samples: the arguments do not broadcast: {e}") from None
    return torch.stack(cols, dim=1).contiguous()


HIT_DTYPE = np.dtype([("prim", np.int32), ("t", np.float32), ("b0", np.float32), ("b1", np.float32), ("b2", np.float32),
                      ("n", np.float32, 3)])


CLOSEST_DTYPE = np.dtype([("prim", np.int32), ("dist2", np.float32), ("p", np.float32, 3), ("b1", np.float32), ("b2", np.float32),
                          ("feature", np.int32)])


RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("b1", np.float32), ("b2", np.float32)])


def make_rays(o, d, tmax=np.inf):
    o = np.asarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3] = o
    r[:, 3] = tmax
    r[:, 4:7] = d
    return r


def stats_dict(s):
    return {k: getattr(s, k) for k, _ in Stats._fields_}


class PathIntegrator:
    """Mirror of pbr::PathIntegrator(maxDepth, camera, sampler, bounds, fb, rrThreshold, strategy)
    (integrators/PathIntegrator.cpp:20-29); camera and sampler are implied by the scene and (W, H, spp)."""
    integrator = _abi.INTEGRATOR_PATH

    def __init__(self, maxDepth=5, rrThreshold=1.0, lightSampleStrategy="spatial"):
        self.maxDepth = int(maxDepth)
        self.rrThreshold = float(rrThreshold)
        self.strategy = LIGHT_STRATEGIES.get(lightSampleStrategy, _abi.LIGHTS_SPATIAL)

    def params(self, width, height, spp, spp_begin=0, spp_end=0, shard_index=0, shard_count=1, shard_rows=1,
               samples_per_pass=0, passes_in_flight=0):
        return RenderParams(width, height, spp, spp_begin, spp_end, self.maxDepth, self.rrThreshold, self.integrator,
                            self.strategy, shard_index, shard_count, shard_rows, samples_per_pass, getattr(self, "directStrategy", 0),
                            passes_in_flight)

    def Li(self, scene, rays, samples, width, height, spp, out=None, stream=None, **kw):
        """SamplerIntegrator::Li along caller rays already on the GPU (gnxr_li_device): `rays` is a contiguous float32 (n, 8) tensor in the
        gnxr_ray layout (rays_tensor), `samples` the int32 (n, 4) gnxr_li_sample records (li_samples): the pixel and sample of a HaltonSampler
        over (width, height, spp) each ray stands for -- the sampler continues at dimension 5, where GetCameraSample leaves it -- and the
        medium it starts in.  Returns (L, stats dict): L is the float32 (n, 4) tensor (`out` when given) of (Li.rgb, 1) per ray; a record
        out of range raises GnxrError after the run and its row is 0.  Runs on `stream` (by default torch's current stream) and returns
        once L is written.  The other keyword arguments are Render's (samples_per_pass = paths per sub-pass, passes_in_flight)."""
        import torch
        _expect("Li: rays", rays, torch.float32, (8,))
        _expect("Li: samples", samples, torch.int32, (4,))
        n = rays.shape[0]
        _same_count("Li", None, samples.shape[0], n, "rays", "sample records")
        out = _out_tensor("Li: out", out, (n, 4), torch.float32, rays.device)
        _expect("Li: rays", rays, torch.float32, (8,), scene.device)
        _expect("Li: samples", samples, torch.int32, (4,), scene.device)
        stream, _ = _stream_pair(stream, rays.device)
        p = self.params(width, height, spp, **kw)
        st = Stats()
        _check(lib().gnxr_li_device(scene._h, C.byref(p), _ptr(rays), _ptr(samples), n, _ptr(out), _addr(stream), C.byref(st)))
        return out, stats_dict(st)

    def RenderViews(self, scene, cameras, width, height, spp, media=None, out=None, stream=None, **kw):
        """Integrator::Render through every camera of `cameras` (gnxr_camera records: camera()) in one call (gnxr_render_views_device):
        returns (float32 tensor [V, H, W, 4] on the scene's device -- `out` when given --, stats dict).  Image v is bit for bit what
        Scene.set_camera(cameras[v], medium=media[v]) + Render gives; the scene's own camera is not touched.  `media`: None (no view
        sits in a medium) or one medium index per view (-1: none).  The views are one path population, so many small images fill the
        GPU; stats holds the sums over the views.  Runs on `stream` (by default torch's current stream) and returns once the images
        are written.  The other keyword arguments are Render's, without the shard fields."""
        import torch
        cameras, media, width, height = _view_args("RenderViews", list(cameras), media, width, height)
        V = len(cameras)
        out = _out_tensor("RenderViews: out", out, (V, height, width, 4), torch.float32, torch.device("cuda", scene.device))
        stream, _ = _stream_pair(stream, out.device)
        p = self.params(width, height, spp, **kw)
        cams = (Camera * max(V, 1))(*cameras)
        med = (C.c_int32 * max(V, 1))(*media) if media is not None else None
        st = Stats()
        _check(lib().gnxr_render_views_device(scene._h, C.byref(p), cams, med, V, _ptr(out), _addr(stream), C.byref(st)))
        return out, stats_dict(st)

    def RenderAdaptive(self, scene, width, height, spp, threshold, min_spp=16, step_spp=16, floor=0.01, guard=1, out=None, count_out=None, stream=None, **kw):
        """Integrator::Render to a noise threshold (gnxr_render_adaptive_device): every pixel takes min_spp samples, then max(step_spp, n // 8)
        more per round (n: what it has) while it -- or a pixel within `guard` pixels of it -- is noisy, up to the budget `spp`.  Sample s of a pixel is Render's.  A
        pixel is noisy while e > threshold * (m + floor * n): e = the rgb sum of |S - 2 A| (S: its sum of Li over all n samples, A: over the
        even ones), m = Sr + Sg + Sb.  Returns (image, count, stats): the float32 [H, W, 4] tensor of S / n (`out` when given), the int32
        [H, W] tensor of n (`count_out` when given), both on the scene's device, and the stats dict of a render extended by `rounds`,
        `samples` (the sum of n) and `pixels_at_budget`.  With min_spp == spp the image is Render's bit for bit.  Runs on `stream` (by
        default torch's current stream) and returns once the outputs are written.  The other keyword arguments are Render's, without the
        sample range and the shard fields; samples_per_pass = paths per sub-pass of a round, as for Li."""
        import math
        import torch
        width, height, spp, min_spp, step_spp, guard = int(width), int(height), int(spp), int(min_spp), int(step_spp), int(guard)
        threshold, floor = float(threshold), float(floor)
        _image_size("RenderAdaptive", width, height)
        if spp < 1 or not 1 <= min_spp <= spp:
            raise ValueError(f"RenderAdaptive: spp >= 1 and min_spp in [1, spp] are required, got spp = {spp}, min_spp = {min_spp}")
        if step_spp < 1:
            raise ValueError(f"RenderAdaptive: step_spp must be at least 1, got {step_spp}")
        if not 0 <= guard <= 8:
            raise ValueError(f"RenderAdaptive: guard must lie in [0, 8], got {guard}")
        if math.isnan(threshold) or threshold < 0 or math.isnan(floor) or floor < 0:
            raise ValueError(f"RenderAdaptive: threshold and floor must be numbers >= 0, got {threshold} and {floor}")
        _only_kw("RenderAdaptive", kw, ("samples_per_pass", "passes_in_flight"))
        hstream, _, out, count_out = _outputs(stream, torch.device("cuda", scene.device), ("RenderAdaptive: out", out, (height, width, 4), torch.float32),
                                              ("RenderAdaptive: count_out", count_out, (height, width), torch.int32))
        p = self.params(width, height, spp, **kw)
        ap = _abi.AdaptiveParams(C.sizeof(_abi.AdaptiveParams), min_spp, step_spp, guard, threshold, floor)
        info = _abi.AdaptiveInfo(C.sizeof(_abi.AdaptiveInfo), 0, 0, 0)
        st = Stats()
        _check(lib().gnxr_render_adaptive_device(scene._h, C.byref(p), C.byref(ap), _ptr(out), _ptr(count_out), _addr(hstream), C.byref(st), C.byref(info)))
        stats = stats_dict(st)
        stats.update(rounds=info.rounds, samples=info.samples, pixels_at_budget=info.pixels_at_budget)
        return out, count_out, stats

    AOV_CHANNELS = ("albedo", "normal", "shading_normal", "depth", "ids")

    def RenderAOV(self, scene, width, height, spp, cameras=None, media=None, channels=AOV_CHANNELS, out=None, stream=None, **kw):
        """First-hit feature buffers (gnxr_render_aov_device): what a denoiser or a data-set writer wants beside the beauty image, averaged
        over the same Halton camera samples as Render / RenderViews.  Returns (dict of torch tensors on the scene's device, stats dict):
        "albedo" (V, H, W, 4) = mean albedo rgb + coverage, "normal" and "shading_normal" (V, H, W, 4) with w = 0, "depth" (V, H, W) float32
        and "ids" (V, H, W, 2) int32 = (primitive, authored material) of the lowest sample, -1 on a miss or a surface without material.
        `cameras`: gnxr Camera records (camera()), or None for the scene's own camera, which also drops the leading V.  `media`: one medium
        index per camera or None.  `channels`: the buffers wanted; `out`: a dict with preallocated tensors for some or all of them.  The
        buffers stop at the first hit: no specular bounce is followed, no medium boundary skipped.  Runs on `stream` (by default torch's
        current stream) and returns once the buffers are written.  Keyword arguments: spp_begin, spp_end, samples_per_pass (the integrator's
        own settings are not used)."""
        import torch
        channels = tuple(channels)
        bad = [c for c in channels if c not in self.AOV_CHANNELS]
        if bad or not channels or len(set(channels)) != len(channels):
            raise ValueError(f"RenderAOV: channels must be a non-empty selection of {self.AOV_CHANNELS}, got {channels}")
        if cameras is None and media is not None:
            raise ValueError("RenderAOV: media goes with cameras; the scene's own camera sits in the scene's camera medium")
        cameras, media, width, height = _view_args("RenderAOV", cameras, media, width, height)
        V = len(cameras) if cameras is not None else 1
        _only_kw("RenderAOV", kw, ("spp_begin", "spp_end", "samples_per_pass"))
        device = torch.device("cuda", scene.device)
        lead = (V,) if cameras is not None else ()
        shapes = {"albedo": (4,), "normal": (4,), "shading_normal": (4,), "depth": (), "ids": (2,)}
        out = dict(out) if out is not None else {}
        extra = [c for c in out if c not in channels]
        if extra:
            raise ValueError(f"RenderAOV: out holds {extra}, which channels does not name")
        hstream, _, *tensors = _outputs(stream, device, *((f"RenderAOV: out[{c!r}]", out.get(c), lead + (height, width) + shapes[c], torch.int32 if c == "ids" else torch.float32)
                                                           for c in channels))
        res = dict(zip(channels, tensors))
        bufs = _abi.AovBuffers(*(_ptr(res.get(c)) for c in self.AOV_CHANNELS))
        p = self.params(width, height, spp, **kw)
        cams = (Camera * V)(*cameras) if cameras else None
        med = (C.c_int32 * V)(*media) if media else None
        st = Stats()
        _check(lib().gnxr_render_aov_device(scene._h, C.byref(p), cams, med, V if cameras is not None else 1, C.byref(bufs), _addr(hstream), C.byref(st)))
        return res, stats_dict(st)

    def RenderDenoised(self, scene, width, height, spp, cameras=None, media=None, normal="shading_normal", stream=None, **denoise_kw):
        """A render at a low sample count, filtered on the device: the two halves [0, spp/2) and [spp/2, spp) of the samples (RenderViews
        when `cameras` are given, else gnxr_render_device through the scene's own camera), RenderAOV over all samples for albedo, the
        normal channel `normal` ("shading_normal" or "normal") and depth, then denoise(half_a, half_b, albedo, normal, depth), all on
        `stream` (by default torch's current stream).  spp must be even and at least 2.  Returns (image, stats): the float32 tensor
        (H, W, 4) -- (V, H, W, 4) with cameras -- and the field-wise sum of the two renders' stats dicts plus "aov", the dict of the
        RenderAOV call.  The other keyword arguments are denoise's (iterations, the sigmas, out)."""
        import torch
        spp = int(spp)
        if spp < 2 or spp % 2:
            raise ValueError(f"RenderDenoised: spp must be even and at least 2 (the two halves are the variance estimate), got {spp}")
        if normal not in ("shading_normal", "normal"):
            raise ValueError(f"RenderDenoised: normal must be 'shading_normal' or 'normal', got {normal!r}")
        if cameras is None and media is not None:
            raise ValueError("RenderDenoised: media goes with cameras; the scene's own camera sits in the scene's camera medium")
        _only_kw("RenderDenoised", denoise_kw, ("iterations", "sigma_color", "sigma_normal", "sigma_depth", "out"))
        cameras, media, width, height = _view_args("RenderDenoised", cameras, media, width, height)
        device = torch.device("cuda", scene.device)
        hstream, tstream = _stream_pair(stream, device)
        halves, stats = [], []
        for lo, hi in ((0, spp // 2), (spp // 2, spp)):
            if cameras is not None:
                img, st = self.RenderViews(scene, cameras, width, height, spp, media=media, stream=tstream, spp_begin=lo, spp_end=hi)
            else:
                with torch.cuda.stream(tstream):
                    img = torch.zeros((height, width, 4), dtype=torch.float32, device=device)
                st = self.RenderDevice(scene, img.data_ptr(), width, height, spp, stream=hstream, spp_begin=lo, spp_end=hi)
            halves.append(img)
            stats.append(st)
        aov, aov_stats = self.RenderAOV(scene, width, height, spp, cameras=cameras, media=media, channels=("albedo", normal, "depth"), stream=tstream)
        image = denoise(halves[0], halves[1], albedo=aov["albedo"], normal=aov[normal], depth=aov["depth"], stream=tstream, **denoise_kw)
        total = {k: stats[0][k] + stats[1][k] for k in stats[0]}
        total["aov"] = aov_stats
        return image, total

    def RenderFiltered(self, scene, width, height, spp, filter, cameras=None, media=None, accum=None, resume=False, out=None, stream=None, **kw):
        """Integrator::Render through a film with a pixel reconstruction filter (gnxr_render_filtered_device; the definition, operation by
        operation: include/gnxr.h): every sample is weighted into all pixels within the filter's radius of its film position, a pixel
        being the weighted sum over the weight sum.  `filter`: film_filter(...).  `cameras`: gnxr Camera records (camera()), or None for
        the scene's own camera, which also drops the leading V; `media`: one medium index per camera or None.  `accum`: a float32
        (H, W, 4) / (V, H, W, 4) tensor of (Sr, Sg, Sb, Wt) on the scene's device to accumulate into -- zeroed first unless `resume` --
        or None for an accumulator inside the library.  Returns (image, stats): the resolved float32 tensor (H, W, 4) / (V, H, W, 4)
        (`out` when given), and the stats dict of a render.  A render over spp_begin..spp_end followed by a resumed one over the next
        range leaves the bits of one render over both.  Runs on `stream` (by default torch's current stream) and returns once the
        outputs are written.  The other keyword arguments are Render's, without the shard fields."""
        import torch
        _film_record("RenderFiltered", filter, "filter must be")
        if cameras is None and media is not None:
            raise ValueError("RenderFiltered: media goes with cameras; the scene's own camera sits in the scene's camera medium")
        cameras, media, width, height = _view_args("RenderFiltered", cameras, media, width, height)
        if resume and accum is None:
            raise ValueError("RenderFiltered: resume continues an accumulator: pass the tensor of the earlier call as accum")
        _only_kw("RenderFiltered", kw, ("spp_begin", "spp_end", "samples_per_pass", "passes_in_flight"))
        V = len(cameras) if cameras is not None else 1
        shape = ((V,) if cameras is not None else ()) + (height, width, 4)
        given = [("RenderFiltered: accum", accum, shape, torch.float32)] if accum is not None else []   # (checked, never allocated)
        hstream, *_, out = _outputs(stream, torch.device("cuda", scene.device), *given, ("RenderFiltered: out", out, shape, torch.float32))
        p = self.params(width, height, spp, **kw)
        cams = (Camera * V)(*cameras) if cameras else None
        med = (C.c_int32 * V)(*media) if media else None
        st = Stats()
        _check(lib().gnxr_render_filtered_device(scene._h, C.byref(p), C.byref(filter), cams, med, V, _ptr(out), _ptr(accum), _abi.FILM_CONTINUE if resume else 0,
                                                 _addr(hstream), C.byref(st)))
        return out, stats_dict(st)

    def BakeLightmap(self, scene, lm_uv, width, height, spp, dilate=2, flip=False, medium=-1, out=None, stream=None, **kw):
        """A lightmap of the scene (gnxr_bake_lightmap_device; the definition, operation by operation: include/gnxr.h): the irradiance
        that arrives at the scene's triangles, in the (width, height) atlas of `lm_uv` -- a contiguous float32 (n_triangles, 6) tensor on
        the scene's device, (u0 v0 u1 v1 u2 v2) per triangle in authoring order.  Per covered texel: pi times the mean over `spp`
        samples of this integrator's Li along cosine-distributed rays off the surface (bake_texels, surface_rays and Li, summed in sample
        order), alpha 1; empty texels are 0; then `dilate` gutter passes (bake_dilate).  `flip` bakes the back side, `medium` is the
        medium the rays start in.  Returns (float32 tensor [H, W, 4] -- `out` when given --, stats dict with camera_samples = covered
        texels * spp).  The live scene is read: a bake after an edit sees it.  Runs on `stream` (by default torch's current stream) and
        returns once the lightmap is written.  Keyword arguments: samples_per_pass (paths per sub-batch), passes_in_flight."""
        import torch
        width, height = _image_size("BakeLightmap", width, height, "atlas")
        if int(dilate) < 0:
            raise ValueError(f"BakeLightmap: dilate must be >= 0, got {dilate}")
        _only_kw("BakeLightmap", kw, ("samples_per_pass", "passes_in_flight"))
        _bake_uv("BakeLightmap", scene, lm_uv)
        hstream, _, out = _outputs(stream, lm_uv.device, ("BakeLightmap: out", out, (height, width, 4), torch.float32))
        p = self.params(width, height, spp, **kw)
        bp = _abi.BakeParams(C.sizeof(_abi.BakeParams), _abi.BAKE_FLIP_NORMALS if flip else 0, int(dilate), int(medium))
        st = Stats()
        _check(lib().gnxr_bake_lightmap_device(scene._h, C.byref(p), C.byref(bp), _ptr(lm_uv), _ptr(out), _addr(hstream), C.byref(st)))
        return out, stats_dict(st)

    def BakeLightProbes(self, scene, positions, spp, width=None, height=None, medium=-1, out=None, stream=None, **kw):
        """Light probes of the scene (gnxr_bake_lightprobes_device; the definition, operation by operation: include/gnxr.h): the radiance
        that arrives at `positions` -- a contiguous float32 (n_probes, 3) tensor on the scene's device --, projected on the nine real
        spherical harmonics of bands 0 to 2.  Per probe: 4 pi times the mean over `spp` samples of this integrator's Li along uniformly
        distributed rays (lightprobe_rays and Li) times the basis (sh_project).  (width, height) is the virtual grid of pixels whose
        Halton sequences the probes use, probe k being pixel (k % width, k // width); by default width = min(n_probes, 1024) and
        height = ceil(n_probes / width).  `medium` is the medium the rays start in.  Returns (float32 tensor [n_probes, 9, 4] -- `out`
        when given --, stats dict with camera_samples = n_probes * spp): slot j = (r, g, b, 0), what sh_irradiance takes.  The live
        scene is read: a bake after an edit sees it.  Runs on `stream` (by default torch's current stream) and returns once the
        coefficients are written.  Keyword arguments: samples_per_pass (paths per sub-batch), passes_in_flight."""
        import torch
        _expect("BakeLightProbes: positions", positions, torch.float32, (3,), scene.device)
        n = positions.shape[0]
        if width is None:
            width = max(1, min(n, 1024))
        width = int(width)
        if height is None:
            height = max(1, -(-n // width)) if width > 0 else 0
        height = int(height)
        if width <= 0 or height <= 0 or width * height < n:
            raise ValueError(f"BakeLightProbes: the {width} x {height} grid of pixels does not hold {n} probes")
        _only_kw("BakeLightProbes", kw, ("samples_per_pass", "passes_in_flight"))
        hstream, _, out = _outputs(stream, positions.device, ("BakeLightProbes: out", out, (n, 9, 4), torch.float32))
        p = self.params(width, height, spp, **kw)
        pp = _abi.LightprobeParams(C.sizeof(_abi.LightprobeParams), 0, int(medium))
        st = Stats()
        _check(lib().gnxr_bake_lightprobes_device(scene._h, C.byref(p), C.byref(pp), _ptr(positions), n, _ptr(out), _addr(hstream), C.byref(st)))
        return out, stats_dict(st)

    def Render(self, scene, width, height, spp, **kw):
        """Integrator::Render: returns (float32 image [H, W, 4], stats dict)."""
        p = self.params(width, height, spp, **kw)
        img = np.zeros((height, width, 4), dtype=np.float32)
        st = Stats()
        _check(lib().gnxr_render(scene._h, C.byref(p), img.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
        return img, stats_dict(st)

    def Reserve(self, scene, width, height, spp, **kw):
        """gnxr_render_reserve: allocate the path state of a Render / RenderDevice call with these arguments, without rendering."""
        p = self.params(width, height, spp, **kw)
        _check(lib().gnxr_render_reserve(scene._h, C.byref(p)))

    def RenderDevice(self, scene, d_ptr, width, height, spp, stream=None, **kw):
        p = self.params(width, height, spp, **kw)
        st = Stats()
        _check(lib().gnxr_render_device(scene._h, C.byref(p), C.c_void_p(int(d_ptr)),
                                        C.c_void_p(int(stream) if stream else None), C.byref(st)))
        return stats_dict(st)


class VolPathIntegrator(PathIntegrator):
    """pbr::VolPathIntegrator (integrators/VolPathIntegrator.cpp): same constructor arguments as PathIntegrator."""
    integrator = _abi.INTEGRATOR_VOLPATH


class WhittedIntegrator(PathIntegrator):
    """pbr::WhittedIntegrator(maxDepth, ...) (integrators/WhittedIntegrator.h): BASELINE config 1, which the reference runs on
    the CPU only.  On the device it is a per-path depth-first state machine (csrc/whitted_kernel.hip.h)."""
    integrator = _abi.INTEGRATOR_WHITTED

    def __init__(self, maxDepth=5):
        super().__init__(maxDepth, 1.0, "uniform")


class DirectLightingIntegrator(PathIntegrator):
    """pbr::DirectLightingIntegrator(strategy, maxDepth, ...) (integrators/DirectLightingIntegrator.h:16-38); strategy is the
    reference's LightStrategy: "all" = UniformSampleAll (Light::nSamples array samples per light and vertex), "one" =
    UniformSampleOne.  Shares the depth-first device state machine with Whitted (csrc/whitted_kernel.hip.h)."""
    integrator = _abi.INTEGRATOR_DIRECT

    def __init__(self, strategy="all", maxDepth=5):
        super().__init__(maxDepth, 1.0, "uniform")
        self.directStrategy = {"all": _abi.DIRECT_SAMPLE_ALL, "one": _abi.DIRECT_SAMPLE_ONE}[strategy]


def sample_halton(width, height, px, py, s, dim):
    px = np.ascontiguousarray(px, dtype=np.int32)
    py = np.ascontiguousarray(py, dtype=np.int32)
    s = np.ascontiguousarray(s, dtype=np.int64)
    dim = np.ascontiguousarray(dim, dtype=np.int32)
    out = np.zeros(len(px), dtype=np.float32)
    _check(lib().gnxr_sample_halton(width, height, px.ctypes.data_as(C.POINTER(C.c_int32)),
                                    py.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_int64)),
                                    dim.ctypes.data_as(C.POINTER(C.c_int32)), len(px),
                                    out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def camera_rays(camera, width, height, px, py, s):
    px = np.ascontiguousarray(px, dtype=np.int32)
    py = np.ascontiguousarray(py, dtype=np.int32)
    s = np.ascontiguousarray(s, dtype=np.int64)
    o = np.zeros((len(px), 3), dtype=np.float32)
    d = np.zeros((len(px), 3), dtype=np.float32)
    _check(lib().gnxr_camera_rays(C.byref(camera), width, height, px.ctypes.data_as(C.POINTER(C.c_int32)),
                                  py.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_int64)),
                                  len(px), o.ctypes.data_as(C.POINTER(C.c_float)),
                                  d.ctypes.data_as(C.POINTER(C.c_float))))
    return o, d


def camera_rays_device(camera, width, height, px, py, s, medium=-1, stream=None):
    """Camera rays on the GPU (gnxr_camera_rays_device): for sample s[i] of pixel (px[i], py[i]) -- contiguous int32 (n,) tensors on one
    device -- of `camera` (camera()) over a (width, height) image, returns (rays [n, 8] float32 in the gnxr_ray layout with tmax = inf,
    samples [n, 4] int32 = px, py, s, medium): the two arrays integrator.Li takes.  o and d carry the bits of camera_rays.  Queued on
    `stream` (by default torch's current stream); a record outside the image or with s < 0 raises GnxrError, its row is 0."""
    import torch
    for what, x in (("px", px), ("py", py), ("s", s)):   # px on any GPU, the others where px is
        if not _is_tensor(x, torch.int32, (None,), ANY_GPU if x is px else px.device):
            _refuse(x, f"camera_rays_device: {what} must be a contiguous int32 (n,) tensor on one GPU")
        _same_count("camera_rays_device", what, x.shape[0], px.shape[0], "px", "entries")
    n = px.shape[0]
    if not isinstance(camera, Camera):
        raise ValueError(f"camera_rays_device: camera must be a gnxr Camera record (camera(...)), got {type(camera).__name__}")
    st, _, rays, samples = _outputs(stream, px.device, ("camera_rays_device: rays", None, (n, 8), torch.float32), ("camera_rays_device: samples", None, (n, 4), torch.int32))
    _check(lib().gnxr_camera_rays_device(C.byref(camera), int(medium), int(width), int(height), _ptr(px), _ptr(py), _ptr(s), n, _ptr(rays), _ptr(samples), _addr(st)))
    return rays, samples


def denoise(color, color_b=None, albedo=None, normal=None, depth=None, iterations=5, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.01, out=None, stream=None):
    """The edge-avoiding a-trous filter on device memory (gnxr_denoise_device; the definition, operation by operation: include/gnxr.h).
    `color`: a contiguous float32 tensor (H, W, 4) or (V, H, W, 4) on a GPU -- the image, or with `color_b` the first of two shares of
    it (renders of the sample ranges [0, N/2) and [N/2, N) of spp = N: they add up to the image and their difference estimates its
    variance, which then steers the colour weight).  Guides, all optional and of color's shape and device: `albedo` (rgb + coverage:
    the image is divided by it before and multiplied after), `normal` (either normal channel of RenderAOV), `depth` ((H, W) or
    (V, H, W)).  `iterations` in [1, 8]: iteration i filters with a 5 x 5 kernel at distance 2^i.  A sigma of 0 switches its term off.
    Returns the filtered float32 tensor of color's shape: `out` when given, which may be `color` or `color_b` but no guide.  Queued on
    `stream` (by default torch's current stream); the call does not wait for the GPU.  Malformed arguments raise ValueError."""
    import math
    import torch
    shape, V, H, W = _image("denoise", "color", color, size=False)
    for what, x, want in (("color_b", color_b, shape), ("albedo", albedo, shape), ("normal", normal, shape), ("depth", depth, shape[:-1])):
        if x is not None and not _is_tensor(x, torch.float32, want, color.device):
            _refuse(x, f"denoise: {what} must be a contiguous float32 tensor of shape {want} on {color.device}")
    _image_size("denoise", W, H)
    iterations = int(iterations)
    if not 1 <= iterations <= 8:
        raise ValueError(f"denoise: iterations must lie in [1, 8], got {iterations}")
    sigmas = [float(sigma_color), float(sigma_normal), float(sigma_depth)]
    if any(math.isnan(s) or s < 0 for s in sigmas):
        raise ValueError(f"denoise: the sigmas must be numbers >= 0, got {sigmas}")
    hstream, _, out = _outputs(stream, color.device, ("denoise: out", out, shape, torch.float32))
    if V == 0:
        return out
    p = _abi.DenoiseParams(C.sizeof(_abi.DenoiseParams), W, H, V, iterations, *sigmas)
    bufs = _abi.DenoiseBuffers(C.sizeof(_abi.DenoiseBuffers), 0, _ptr(color), _ptr(color_b), _ptr(albedo), _ptr(normal), _ptr(depth))
    _check(lib().gnxr_denoise_device(C.byref(p), C.byref(bufs), _ptr(out), _addr(hstream)))
    return out


FILM_FILTER_KINDS = {"box": _abi.FILTER_BOX, "triangle": _abi.FILTER_TRIANGLE, "gaussian": _abi.FILTER_GAUSSIAN, "mitchell": _abi.FILTER_MITCHELL,
                     "table": _abi.FILTER_TABLE}


def film_filter(kind, radius, alpha=2.0, B=1 / 3, C=1 / 3, table=None):
    """A pixel reconstruction filter of the film (gnxr_film_filter): `kind` is "box", "triangle", "gaussian" (falloff `alpha`), "mitchell"
    (`B`, `C`) or "table" (`table`: 256 values, row y of 16 entries at y*16, entry (x, y) weighing a sample (x + 0.5) / 16 of the radius
    away in x and likewise in y); `radius`: a number or (radius_x, radius_y), each in [0.5, 4] pixels.  Returns the record film_add,
    film_filter_table and integrator.RenderFiltered take.  Malformed arguments raise ValueError."""
    import ctypes
    import math
    if kind not in FILM_FILTER_KINDS:
        raise ValueError(f"film_filter: kind must be one of {tuple(FILM_FILTER_KINDS)}, got {kind!r}")
    try:
        rx, ry = (float(radius), float(radius)) if np.ndim(radius) == 0 else (float(radius[0]), float(radius[1]))
        if np.ndim(radius) != 0 and len(radius) != 2:
            raise TypeError
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"film_filter: radius must be a number or a pair of numbers, got {radius!r}") from None
    if not (0.5 <= rx <= 4.0 and 0.5 <= ry <= 4.0):   # (a NaN fails)
        raise ValueError(f"film_filter: the radii must lie in [0.5, 4], got {rx} x {ry}")
    a, b = (float(alpha), 0.0) if kind == "gaussian" else ((float(B), float(C)) if kind == "mitchell" else (0.0, 0.0))
    if math.isnan(a) or math.isnan(b):
        raise ValueError(f"film_filter: the parameters of a {kind} filter must be numbers, got {a} and {b}")
    tab = None
    if kind == "table":
        if table is None:
            raise ValueError("film_filter: kind 'table' needs table = 256 values")
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1)
        if tab.size != 256:
            raise ValueError(f"film_filter: table must hold 256 values (16 x 16), got {tab.size}")
    elif table is not None:
        raise ValueError(f"film_filter: table goes with kind 'table', not {kind!r}")
    f = _abi.FilmFilter(ctypes.sizeof(_abi.FilmFilter), FILM_FILTER_KINDS[kind], rx, ry, a, b,
                        tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tab is not None else None)
    f._table = tab   # the record points into it
    return f


def _film_record(name, f, phrase="expected"):
    if not isinstance(f, _abi.FilmFilter):
        raise ValueError(f"{name}: {phrase} a film_filter(...) record, got {type(f).__name__}")
    return f


def film_filter_table(f):
    """The 16 x 16 table of weights the film builds from the record `f` (gnxr_film_filter_table, host code: needs no GPU): a float32
    (16, 16) numpy array, entry [y, x] = the filter at ((x + 0.5) * radius_x / 16, (y + 0.5) * radius_y / 16)."""
    _film_record("film_filter_table", f)
    out = np.zeros((16, 16), dtype=np.float32)
    _check(lib().gnxr_film_filter_table(C.byref(f), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def film_add(f, L, offsets, accum, stream=None):
    """Adds layers of samples to a film accumulator on device memory (gnxr_film_add_device): `accum` is a contiguous float32 tensor
    (H, W, 4) or (V, H, W, 4) of (Sr, Sg, Sb, Wt), `L` (n, *accum.shape) holds the sample of layer j that belongs to each pixel (w is
    ignored) and `offsets` (n, *accum.shape[:-1], 2) its film offset (ux, uy) inside that pixel; a sample with an offset outside [0, 1]
    adds nothing.  Every sample is weighted by the filter `f` (film_filter) into the pixels of its view within the radius of its
    position, layer by layer in the order include/gnxr.h defines.  Returns accum.  Queued on `stream` (by default torch's current
    stream); the call does not wait for the GPU.  Malformed arguments raise ValueError."""
    import torch
    _film_record("film_add", f)
    shape, V, H, W = _image("film_add", "accum", accum)
    if not _is_tensor(L, torch.float32, (None,) + shape, accum.device):
        _refuse(L, f"film_add: L must be a contiguous float32 tensor of shape (n, {', '.join(map(str, shape))}) on {accum.device}")
    n = L.shape[0]
    if not _is_tensor(offsets, torch.float32, (n,) + shape[:-1] + (2,), accum.device):
        _refuse(offsets, f"film_add: offsets must be a contiguous float32 tensor of shape ({n}, {', '.join(map(str, shape[:-1]))}, 2) on {accum.device}")
    if V == 0 or n == 0:
        return accum
    hstream, _ = _stream_pair(stream, accum.device)
    _check(lib().gnxr_film_add_device(C.byref(f), W, H, V, n, _ptr(L), _ptr(offsets), _ptr(accum), _addr(hstream)))
    return accum


def film_resolve(accum, out=None, stream=None):
    """The image of a film accumulator (gnxr_film_resolve_device): per pixel (Sr / Wt, Sg / Wt, Sb / Wt, 1), a channel being 0 where Wt is 0
    or the quotient is negative.  `accum`: as for film_add.  Returns the float32 tensor of accum's shape: `out` when given, which may
    be `accum` itself.  Queued on `stream` (by default torch's current stream); the call does not wait for the GPU."""
    import torch
    shape, V, H, W = _image("film_resolve", "accum", accum)
    hstream, _, out = _outputs(stream, accum.device, ("film_resolve: out", out, shape, torch.float32))
    if V == 0:
        return out
    _check(lib().gnxr_film_resolve_device(W, H, V, _ptr(accum), _ptr(out), _addr(hstream)))
    return out


def _bake_uv(name, scene, lm_uv):
    """the lightmap uv set of the baking calls: a contiguous float32 (n_triangles, 6) tensor on the scene's device"""
    import torch
    _expect(f"{name}: lm_uv", lm_uv, torch.float32, (6,), scene.device)
    _same_count(name, "lm_uv", lm_uv.shape[0], scene.n_triangles, "triangles")
    return lm_uv


def bake_texels(scene, lm_uv, width, height, out=None, stream=None):
    """Atlas rasterisation on the GPU (gnxr_bake_texels_device; the definition: include/gnxr.h): `lm_uv` is a contiguous float32
    (n_triangles, 6) tensor on the scene's device, (u0 v0 u1 v1 u2 v2) per triangle in authoring order.  Returns (tri, bary): the int32
    (H, W) tensor of the lowest triangle that covers each texel centre (-1: none; both windings, inclusive edges) and the float32
    (H, W, 2) tensor of its barycentrics (b1, b2) there.  `out`: a (tri, bary) pair to write into.  Queued on `stream` (by default
    torch's current stream); the call does not wait for the GPU."""
    import torch
    width, height = _image_size("bake_texels", width, height, "atlas")
    _bake_uv("bake_texels", scene, lm_uv)
    out_tri, out_bary = out if out is not None else (None, None)
    hstream, _, tri, bary = _outputs(stream, lm_uv.device, ("bake_texels: out[0]", out_tri, (height, width), torch.int32), ("bake_texels: out[1]", out_bary, (height, width, 2), torch.float32))
    _check(lib().gnxr_bake_texels_device(scene._h, _ptr(lm_uv), width, height, _ptr(tri), _ptr(bary), _addr(hstream)))
    return tri, bary


def surface_rays(scene, tri, bary, px, py, s, width, height, flip=False, medium=-1, out=None, stream=None):
    """Rays off the scene's surfaces on the GPU (gnxr_surface_rays_device), the texture-space sibling of camera_rays_device: record i is
    the point with barycentrics bary[i] = (b1, b2) on triangle tri[i] (authoring order, current vertices) and sample s[i] of pixel
    (px[i], py[i]) of a HaltonSampler over (width, height).  tri, px, py, s: contiguous int32 (n,) tensors, bary: float32 (n, 2), all on
    the scene's device.  Returns (rays [n, 8] float32 in the gnxr_ray layout, samples [n, 4] int32 = px, py, s, medium, pn [n, 8] float32 =
    position, 0, normal, 0): rays leave cosine-distributed about the geometric normal (negated with `flip`), drawn from Halton dimensions
    3 and 4, from an origin offset by the point's error bound; rays and samples are what integrator.Li takes.  `out`: a (rays, samples,
    pn) triple to write into.  A degenerate triangle gives zero rows; a triangle, pixel or sample out of range raises GnxrError after the
    others are finished, its rows are 0.  Queued on `stream` (by default torch's current stream)."""
    import torch
    _expect("surface_rays: tri", tri, torch.int32, (), scene.device)
    n = tri.shape[0]
    _expect("surface_rays: bary", bary, torch.float32, (2,), scene.device)
    for what, x in (("px", px), ("py", py), ("s", s)):
        _expect(f"surface_rays: {what}", x, torch.int32, (), scene.device)
        _same_count("surface_rays", what, x.shape[0], n, "triangles", "entries")
    _same_count("surface_rays", "bary", bary.shape[0], n, "triangles")
    o_rays, o_samples, o_pn = out if out is not None else (None, None, None)
    hstream, _, rays, samples, pn = _outputs(stream, tri.device, ("surface_rays: out[0]", o_rays, (n, 8), torch.float32), ("surface_rays: out[1]", o_samples, (n, 4), torch.int32),
                                             ("surface_rays: out[2]", o_pn, (n, 8), torch.float32))
    _check(lib().gnxr_surface_rays_device(scene._h, int(width), int(height), _ptr(tri), _ptr(bary), _ptr(px), _ptr(py), _ptr(s), n, _abi.BAKE_FLIP_NORMALS if flip else 0,
                                          int(medium), _ptr(rays), _ptr(samples), _ptr(pn), _addr(hstream)))
    return rays, samples, pn


def bake_dilate(img, iterations, out=None, stream=None):
    """Gutter dilation of a lightmap on the GPU (gnxr_bake_dilate_device; the definition: include/gnxr.h): `img` is a contiguous float32
    (H, W, 4) tensor whose alpha is coverage.  Each of `iterations` passes gives every texel that is not filled yet and has filled
    8-neighbours the mean of their rgb; alpha is never changed.  Returns the dilated tensor: `out` when given, which may be `img` (in
    place).  Queued on `stream` (by default torch's current stream); the call does not wait for the GPU."""
    import torch
    if not _is_tensor(img, torch.float32, (None, None, 4), ANY_GPU):
        _refuse(img, "bake_dilate: img must be a contiguous float32 (H, W, 4) tensor on a GPU")
    W, H = _image_size("bake_dilate", img.shape[1], img.shape[0])
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"bake_dilate: iterations must be >= 0, got {iterations}")
    hstream, tstream, out = _outputs(stream, img.device, ("bake_dilate: out", out, tuple(img.shape), torch.float32))
    if out.data_ptr() != img.data_ptr():
        with torch.cuda.stream(tstream):
            out.copy_(img)
    _check(lib().gnxr_bake_dilate_device(W, H, iterations, _ptr(out), _addr(hstream)))
    return out


def lightprobe_rays(scene, pos, px, py, s, width, height, medium=-1, out=None, stream=None):
    """Rays from points in free space on the GPU (gnxr_lightprobe_rays_device), the sibling of surface_rays: record i starts at pos[i] and
    takes sample s[i] of pixel (px[i], py[i]) of a HaltonSampler over (width, height).  pos: a contiguous float32 (n, 3) tensor, px, py,
    s: int32 (n,), all on the scene's device.  Returns (rays [n, 8] float32 in the gnxr_ray layout, samples [n, 4] int32 = px, py, s,
    medium): directions are uniform over the sphere, drawn from Halton dimensions 3 and 4; the two arrays are what integrator.Li takes.
    `out`: a (rays, samples) pair to write into.  A non-finite position, a pixel outside the image or s < 0 raises GnxrError after the
    others are finished, its rows are 0.  Queued on `stream` (by default torch's current stream)."""
    import torch
    _expect("lightprobe_rays: pos", pos, torch.float32, (3,), scene.device)
    n = pos.shape[0]
    for what, x in (("px", px), ("py", py), ("s", s)):
        _expect(f"lightprobe_rays: {what}", x, torch.int32, (), scene.device)
        _same_count("lightprobe_rays", what, x.shape[0], n, "positions", "entries")
    width, height = _image_size("lightprobe_rays", width, height)
    o_rays, o_samples = out if out is not None else (None, None)
    hstream, _, rays, samples = _outputs(stream, pos.device, ("lightprobe_rays: out[0]", o_rays, (n, 8), torch.float32), ("lightprobe_rays: out[1]", o_samples, (n, 4), torch.int32))
    _check(lib().gnxr_lightprobe_rays_device(scene._h, width, height, _ptr(pos), _ptr(px), _ptr(py), _ptr(s), n, int(medium), _ptr(rays), _ptr(samples), _addr(hstream)))
    return rays, samples


def sh_project(rays, L, n_probes, out=None, accumulate=False, stream=None):
    """Projects radiance samples on the nine real spherical harmonics of bands 0 to 2 on the GPU (gnxr_sh_project_device; the basis and the
    order of the sum: include/gnxr.h).  `rays` (n, 8) float32 in the gnxr_ray layout -- only the directions are read -- and `L` (n, 4)
    float32 are contiguous tensors on one GPU in probe-major order: n = n_probes * n_samples, row k * n_samples + s is sample s of probe k.
    Returns the float32 (n_probes, 9, 4) tensor of sums, slot j = (sum r, sum g, sum b, 0) of L * Y_j: `out` when given.  With
    `accumulate` the sums continue from what `out` holds: the samples of a probe may then come in several calls, whole blocks of 64 in
    every call but the last.  Queued on `stream` (by default torch's current stream); the call does not wait for the GPU."""
    import torch
    _expect("sh_project: rays", rays, torch.float32, (8,), ANY_GPU)
    _expect("sh_project: L", L, torch.float32, (4,), rays.device)
    n_probes = int(n_probes)
    n = rays.shape[0]
    _same_count("sh_project", "L", L.shape[0], n, "rays")
    if n_probes < 0 or (n_probes == 0 and n != 0) or (n_probes > 0 and n % n_probes != 0):
        raise ValueError(f"sh_project: {n} records are no whole number of samples for each of {n_probes} probes")
    if accumulate and out is None:
        raise ValueError("sh_project: accumulate continues the sums of an earlier call: pass its tensor as out")
    hstream, _, out = _outputs(stream, rays.device, ("sh_project: out", out, (n_probes, 9, 4), torch.float32))
    if n_probes == 0:
        return out
    _check(lib().gnxr_sh_project_device(_ptr(rays), _ptr(L), n_probes, n // n_probes, _ptr(out), _abi.SH_CONTINUE if accumulate else 0, _addr(hstream)))
    return out


def sh_irradiance(sh, probe, normals, out=None, stream=None):
    """Irradiance from light probes on the GPU (gnxr_sh_irradiance_device; the definition: include/gnxr.h): `sh` is a contiguous float32
    (n_probes, 9, 4) tensor of coefficients (BakeLightProbes), `probe` an int32 (n,) tensor of probe indices and `normals` a float32
    (n, 3) tensor of unit normals, all on one GPU.  Returns the float32 (n, 4) tensor (E r, E g, E b, 1) of the irradiance that probe
    probe[i] gives a surface facing normals[i]: `out` when given.  A probe index out of range raises GnxrError after the others are
    finished, its row is 0.  Queued on `stream` (by default torch's current stream)."""
    import torch
    _expect("sh_irradiance: sh", sh, torch.float32, (9, 4), ANY_GPU)
    _expect("sh_irradiance: probe", probe, torch.int32, (), sh.device)
    _expect("sh_irradiance: normals", normals, torch.float32, (3,), sh.device)
    n = probe.shape[0]
    _same_count("sh_irradiance", "normals", normals.shape[0], n, "probe indices")
    hstream, _, out = _outputs(stream, sh.device, ("sh_irradiance: out", out, (n, 4), torch.float32))
    if n == 0:
        return out
    _check(lib().gnxr_sh_irradiance_device(_ptr(sh), sh.shape[0], _ptr(probe), _ptr(normals), n, _ptr(out), _addr(hstream)))
    return out


def camera_matrices(camera, width, height):
    """gnxr_camera_matrices (host, needs no GPU): {"r2c", "c2w", "w2r"} as (4, 4) float32 arrays -- RasterToCamera and CameraToWorld as every
    kernel's camera record holds them for `camera` (camera()) over a (width, height) film, and WorldToRaster, the product of the forward
    matrices they are made of: the single definition of the matrix Scene.motion projects with."""
    if not isinstance(camera, Camera):
        raise ValueError(f"camera_matrices: camera must be a gnxr Camera record (camera(...)), got {type(camera).__name__}")
    m = {k: np.zeros((4, 4), dtype=np.float32) for k in ("r2c", "c2w", "w2r")}
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    _check(lib().gnxr_camera_matrices(C.byref(camera), int(width), int(height), fp(m["r2c"]), fp(m["c2w"]), fp(m["w2r"])))
    return m


def temporal_accumulate(color, motion, guide, prim, history=None, max_history=32, depth_tol=0.05, normal_cos=0.9, out=None, stream=None):
    """Blends a frame into its reprojected history on the GPU (gnxr_temporal_accumulate_device; the definition, operation by operation:
    include/gnxr.h).  `color`: this frame's image, a contiguous float32 tensor (H, W, 4) or (V, H, W, 4) on a GPU; `motion`, `guide`
    (color's shape) and `prim` (int32, color's shape without the 4): this frame's channels of Scene.motion.  `history`: None (the first
    frame, or after a reset) or the dict an earlier call returned.  A history tap counts when it shows the same primitive at the expected
    depth (within depth_tol, relative) under a similar normal (cosine at least normal_cos); the history length stops at max_history, so
    that an old frame's weight decays.  Returns the next history, a dict {"color": the accumulated image, "stat": (m1, m2, N, var) per
    pixel -- the moments of the luminance, the history length, the variance --, "guide": guide, "prim": prim}.  `out`: a dict with
    preallocated "color" and / or "stat" tensors, which may overlap no input.  After set_geometry, set_lights or a material edit the
    caller starts over with history=None.  Queued on `stream` (by default torch's current stream); the call does not wait for the GPU.
    Malformed arguments raise ValueError."""
    import math
    import torch
    shape, V, H, W = _image("temporal_accumulate", "color", color, size=False)

    def layout(what, x, prim_like):
        want, dtype = (shape[:-1], torch.int32) if prim_like else (shape, torch.float32)
        if not _is_tensor(x, dtype, want, color.device):
            _refuse(x, f"temporal_accumulate: {what} must be a contiguous {dtype} tensor of shape {want} on {color.device}")

    layout("motion", motion, False); layout("guide", guide, False); layout("prim", prim, True)
    if history is not None:
        if not isinstance(history, dict) or sorted(history) != ["color", "guide", "prim", "stat"]:
            raise ValueError("temporal_accumulate: history must be None or a dict with 'color', 'stat', 'guide' and 'prim' (what an earlier call returned)")
        for k in ("color", "stat", "guide", "prim"):
            layout(f"history[{k!r}]", history[k], k == "prim")
    _image_size("temporal_accumulate", W, H)
    max_history, depth_tol, normal_cos = int(max_history), float(depth_tol), float(normal_cos)
    if max_history < 1:
        raise ValueError(f"temporal_accumulate: max_history must be at least 1, got {max_history}")
    if math.isnan(depth_tol) or depth_tol < 0 or math.isnan(normal_cos):
        raise ValueError(f"temporal_accumulate: depth_tol must be a number >= 0 and normal_cos a number, got {depth_tol} and {normal_cos}")
    out = dict(out) if out is not None else {}
    extra = [k for k in out if k not in ("color", "stat")]
    if extra:
        raise ValueError(f"temporal_accumulate: out holds {extra}; the outputs are 'color' and 'stat'")
    hstream, _, o_color, o_stat = _outputs(stream, color.device, ("temporal_accumulate: out['color']", out.get("color"), shape, torch.float32),
                                           ("temporal_accumulate: out['stat']", out.get("stat"), shape, torch.float32))
    res = {"color": o_color, "stat": o_stat, "guide": guide, "prim": prim}
    if V == 0:
        return res
    h = history or {}
    p = _abi.TemporalParams(C.sizeof(_abi.TemporalParams), W, H, V, max_history, depth_tol, normal_cos)
    bufs = _abi.TemporalBuffers(C.sizeof(_abi.TemporalBuffers), 0, _ptr(color), _ptr(motion), _ptr(guide), _ptr(prim), _ptr(h.get("color")), _ptr(h.get("stat")), _ptr(h.get("guide")),
                                _ptr(h.get("prim")), _ptr(o_color), _ptr(o_stat))
    _check(lib().gnxr_temporal_accumulate_device(C.byref(p), C.byref(bufs), _addr(hstream)))
    return res


_denoise = denoise   # (TemporalAccumulator.frame has an argument of that name)


class TemporalAccumulator:
    """A frame loop with history: renders a low-spp frame, finds where every pixel was one frame ago and blends the frame into what the
    earlier frames left there -- the composition integrator.RenderDevice -> Scene.motion -> temporal_accumulate (-> denoise), nothing
    more: its result equals that chain of public calls on bits.

        acc = TemporalAccumulator(PathIntegrator(5), scene, 1920, 1080, spp=4)
        for cam in orbit:
            frame = acc.frame(cam, denoise=True)      # frame["denoised"], frame["color"], frame["stat"][..., 2] = history length

    Frame k renders the samples [(k mod max_history) * spp, + spp) of a sampler with samplesPerPixel = max_history * spp (spp_begin /
    spp_end), so consecutive frames are independent estimates, and multiplies the rgb of that share by (float)max_history: the frame's own
    estimate.  The other keyword arguments are temporal_accumulate's (depth_tol, normal_cos).  The accumulator detects no edit: after
    Scene.set_geometry, set_lights or a material edit the caller calls reset(); moved vertices are handed to frame() as prev_vertices."""

    def __init__(self, integrator, scene, width, height, spp, max_history=32, **accumulate_kw):
        width, height, spp, max_history = int(width), int(height), int(spp), int(max_history)
        _image_size("TemporalAccumulator", width, height)
        if spp < 1 or max_history < 1:
            raise ValueError(f"TemporalAccumulator: spp and max_history must be at least 1, got {spp} and {max_history}")
        _only_kw("TemporalAccumulator", accumulate_kw, ("depth_tol", "normal_cos"))
        self.integrator, self.scene, self.width, self.height, self.spp, self.max_history = integrator, scene, width, height, spp, max_history
        self.accumulate_kw = dict(accumulate_kw)
        self.reset()

    def reset(self):
        """Forget the history: the next frame starts from its own samples alone."""
        self.history = None
        self.prev_camera = None
        self.k = 0

    def frame(self, camera=None, prev_vertices=None, denoise=False, stream=None):
        """One frame.  `camera`: None keeps the scene's camera; a gnxr Camera record (camera()) is set with Scene.set_camera first (outside
        any medium).  `prev_vertices`: what Scene.motion takes, when vertices moved since the last frame.  `denoise`: also pass the
        accumulated colour through denoise() as a single share, guided by this frame's normals and depths.  Returns the history dict of
        temporal_accumulate ("color", "stat", "guide", "prim") with "motion" added, and "denoised" with denoise=True.  Runs on `stream`
        (by default torch's current stream)."""
        import torch
        scene, W, H, M = self.scene, self.width, self.height, self.max_history
        if camera is not None:
            if not isinstance(camera, Camera):
                raise ValueError(f"TemporalAccumulator.frame: camera must be a gnxr Camera record (camera(...)), got {type(camera).__name__}")
            scene.set_camera(tuple(camera.eye), tuple(camera.look), tuple(camera.up), camera.fov_deg, camera.lens_radius, camera.focal_distance, bool(camera.orthographic))
        cam = Camera()
        C.memmove(C.byref(cam), C.byref(scene.camera), C.sizeof(Camera))
        device = torch.device("cuda", scene.device)
        hstream, tstream = _stream_pair(stream, device)
        with torch.cuda.stream(tstream):
            img = torch.zeros((H, W, 4), dtype=torch.float32, device=device)
        lo = (self.k % M) * self.spp
        self.integrator.RenderDevice(scene, img.data_ptr(), W, H, M * self.spp, stream=hstream, spp_begin=lo, spp_end=lo + self.spp)
        with torch.cuda.stream(tstream):
            img[..., :3] *= float(M)
        mo = scene.motion(W, H, self.prev_camera if self.prev_camera is not None else cam, prev_vertices=prev_vertices, stream=tstream)
        res = temporal_accumulate(img, mo["motion"], mo["guide"], mo["prim"], history=self.history, max_history=M, stream=tstream, **self.accumulate_kw)
        self.history, self.prev_camera = res, cam
        self.k += 1
        res = dict(res, motion=mo["motion"])
        if denoise:
            with torch.cuda.stream(tstream):
                depth = mo["guide"][..., 3].contiguous()
            res["denoised"] = _denoise(res["color"], normal=mo["guide"], depth=depth, stream=tstream)
        return res


def skin_vertices(rest, bone_index, bone_weight, bones, morph_delta=None, morph_weight=None, out=None, stream=None):
    """Linear-blend skinning with blend shapes on the GPU (gnxr_skin_vertices_device; the definition, operation by operation:
    include/gnxr.h).  All arguments are contiguous torch tensors on one GPU: `rest` (V, 3) float32, `bone_index` (V, 4) int32,
    `bone_weight` (V, 4) float32 (used as given, never normalised; a slot with weight 0 is skipped and its index ignored), `bones`
    (B, 3, 4) or (B, 12) float32, row-major 3x4 matrices to world space, and optionally `morph_delta` (M, V, 3) float32 with
    `morph_weight` (M,) float32.  Returns the (V, 3) float32 positions (`out` when given; it must not overlap an input), which
    Scene.update_vertices takes as they are.  A bone index outside [0, B) in a used slot raises GnxrError.  Queued on `stream` (by default
    torch's current stream)."""
    import torch
    name = "skin_vertices"
    _expect(f"{name}: rest", rest, torch.float32, (3,), ANY_GPU)
    dev, V = rest.device, rest.shape[0]
    _expect(f"{name}: bone_index", bone_index, torch.int32, (4,), dev)
    _expect(f"{name}: bone_weight", bone_weight, torch.float32, (4,), dev)
    _expect(f"{name}: bones", bones, torch.float32, (3, 4) if isinstance(bones, torch.Tensor) and bones.dim() == 3 else (12,), dev)
    if bone_index.shape[0] != V or bone_weight.shape[0] != V:
        raise ValueError(f"{name}: {V} rest positions, {bone_index.shape[0]} index rows, {bone_weight.shape[0]} weight rows")
    if bones.shape[0] < 1:
        raise ValueError(f"{name}: at least one bone is required")
    if (morph_delta is None) != (morph_weight is None):
        raise ValueError(f"{name}: morph_delta and morph_weight come together or not at all")
    M = 0
    if morph_delta is not None:
        _expect(f"{name}: morph_delta", morph_delta, torch.float32, (V, 3), dev)
        _expect(f"{name}: morph_weight", morph_weight, torch.float32, (), dev)
        M = morph_delta.shape[0]
        if morph_weight.shape[0] != M:
            raise ValueError(f"{name}: {M} morph targets, {morph_weight.shape[0]} weights")
    hstream, _, res = _outputs(stream, dev, (f"{name}: out", out, (V, 3), torch.float32))
    p = _abi.SkinParams(C.sizeof(_abi.SkinParams), V, int(bones.shape[0]), M)
    _check(lib().gnxr_skin_vertices_device(C.byref(p), _ptr(rest), _ptr(bone_index), _ptr(bone_weight), _ptr(bones), _ptr(morph_delta) if M else None,
                                           _ptr(morph_weight) if M else None, _ptr(res), _addr(hstream)))
    return res


class SkinnedMesh:
    """The per-frame loop of a skinned mesh in a live scene, made of the public calls and nothing else: skin_vertices ->
    Scene.update_vertices -> Scene.recompute_normals.

    `vertices`: the description's whole vertex array, (n_vertices, 3) float32 (numpy or a tensor); `rest`, `bone_index`, `bone_weight`
    (and `morph_delta`): skin_vertices' arguments for vertices [first_vertex, first_vertex + len(rest)), tensors on the scene's device.
    The object keeps two whole-scene vertex tensors on the device, the current and the previous frame's -- the layout
    Scene.motion(prev_vertices=) and TemporalAccumulator.frame(prev_vertices=) take.  move_lights: pass it on to update_vertices;
    normals=False leaves the shading normals alone (a flat-shaded mesh)."""

    def __init__(self, scene, vertices, rest, bone_index, bone_weight, first_vertex=0, morph_delta=None, move_lights=False, normals=True):
        import torch
        device = torch.device("cuda", scene.device)
        v = torch.as_tensor(vertices, dtype=torch.float32).to(device).contiguous()
        if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] != scene.n_vertices:
            raise ValueError(f"SkinnedMesh: vertices: expected (n_vertices = {scene.n_vertices}, 3), got {tuple(v.shape)}")
        first_vertex = int(first_vertex)
        if first_vertex < 0 or first_vertex + rest.shape[0] > scene.n_vertices:
            raise ValueError(f"SkinnedMesh: vertices [{first_vertex}, {first_vertex + rest.shape[0]}) outside the scene's {scene.n_vertices}")
        self.scene, self.first_vertex, self.move_lights, self.normals = scene, first_vertex, bool(move_lights), bool(normals)
        self.rest, self.bone_index, self.bone_weight, self.morph_delta = rest, bone_index, bone_weight, morph_delta
        self.vertices, self.prev_vertices = v.clone(), v.clone()

    def pose(self, bones, morph_weight=None, flip=False, stream=None):
        """One frame: the two vertex tensors swap, the range is skinned into the current one, the scene takes it (update_vertices, then
        recompute_normals unless normals=False).  Returns the previous frame's whole vertex tensor."""
        import torch
        self.vertices, self.prev_vertices = self.prev_vertices, self.vertices
        _, tstream = _stream_pair(stream, self.vertices.device)
        n = self.rest.shape[0]
        moved = self.vertices[self.first_vertex:self.first_vertex + n]   # (rows of a contiguous tensor: contiguous)
        skin_vertices(self.rest, self.bone_index, self.bone_weight, bones, self.morph_delta, morph_weight if self.morph_delta is not None else None, out=moved, stream=tstream)
        self.scene.update_vertices(moved, first_vertex=self.first_vertex, stream=tstream, move_lights=self.move_lights)
        if self.normals:
            self.scene.recompute_normals(flip=flip, stream=tstream)
        return self.prev_vertices


def _min_log2(name, min_log2):
    min_log2 = int(min_log2)
    if not -126 <= min_log2 <= 111:
        raise ValueError(f"{name}: min_log2 must lie in [-126, 111], got {min_log2}")
    return min_log2


def luminance_histogram(color, min_log2=-12, out=None, stream=None):
    """Log-luminance histogram of an image on the GPU (gnxr_luminance_histogram_device; the definition: include/gnxr.h).  `color`: a
    contiguous float32 tensor (H, W, 4) or (V, H, W, 4) on a GPU.  Returns an int32 tensor (V, 260) -- `out` when given --: per view 256
    bins, sixteen per octave over [2^min_log2, 2^(min_log2 + 16)), then the pixels below the range (zero and negative ones among them),
    above it, not finite, and a 0.  The counts are exact: the bin comes from the bit pattern of the luminance.  Queued on `stream` (by
    default torch's current stream); the call does not wait for the GPU.  Malformed arguments raise ValueError."""
    import torch
    shape, V, H, W = _image("luminance_histogram", "color", color)
    min_log2 = _min_log2("luminance_histogram", min_log2)
    hstream, _, out = _outputs(stream, color.device, ("luminance_histogram: out", out, (V, _abi.HISTOGRAM_WORDS), torch.int32))
    if V == 0:
        return out
    p = _abi.HistogramParams(C.sizeof(_abi.HistogramParams), W, H, V, min_log2)
    _check(lib().gnxr_luminance_histogram_device(C.byref(p), _ptr(color), _ptr(out), _addr(hstream)))
    return out


def auto_exposure(hist, prev=None, key=0.18, low=0.5, high=0.95, rate=1.0, min_exposure=2 ** -8, max_exposure=2 ** 8, min_log2=-12, out=None, stream=None):
    """The exposure a luminance histogram meters, adapted over time, computed on the GPU (gnxr_exposure_device; the definition, operation
    by operation: include/gnxr.h).  `hist`: the int32 (V, 260) tensor of luminance_histogram, taken with the same min_log2.  The pixels
    between the quantiles `low` and `high` of the in-range luminances are averaged in log2, and the target exposure puts that average on
    `key`, clamped to [min_exposure, max_exposure].  `prev`: None, or the tensor an earlier call returned: the exposure then moves from
    its previous value towards the target by the fraction `rate`; a black frame holds the previous value.  Returns a float32 (V, 4)
    tensor -- `out` when given, which may be `prev` (in place) --: per view (exposure, target, the metered log2 luminance, the weight
    it was metered from).  tonemap takes the tensor as its exposure: the value never visits the host.  Queued on `stream` (by default
    torch's current stream); the call does not wait for the GPU.  Malformed arguments raise ValueError."""
    import math
    import torch
    if not _is_tensor(hist, torch.int32, (None, _abi.HISTOGRAM_WORDS), ANY_GPU):
        _refuse(hist, f"auto_exposure: hist must be a contiguous int32 (V, {_abi.HISTOGRAM_WORDS}) tensor on a GPU (luminance_histogram)")
    V = hist.shape[0]
    if prev is not None and not _is_tensor(prev, torch.float32, (V, 4), hist.device):
        _refuse(prev, f"auto_exposure: prev must be None or a contiguous float32 ({V}, 4) tensor on {hist.device}")
    min_log2 = _min_log2("auto_exposure", min_log2)
    key, low, high, rate, min_exposure, max_exposure = (float(x) for x in (key, low, high, rate, min_exposure, max_exposure))
    if not all(math.isfinite(x) for x in (key, low, high, rate, min_exposure, max_exposure)):
        raise ValueError("auto_exposure: key, low, high, rate, min_exposure and max_exposure must be finite")
    if not (0 <= low < high <= 1):
        raise ValueError(f"auto_exposure: 0 <= low < high <= 1 is required, got {low} and {high}")
    if not (key > 0 and 0 < rate <= 1 and 0 < min_exposure <= max_exposure):
        raise ValueError(f"auto_exposure: key > 0, 0 < rate <= 1 and 0 < min_exposure <= max_exposure are required, got {key}, {rate}, {min_exposure} and {max_exposure}")
    hstream, _, out = _outputs(stream, hist.device, ("auto_exposure: out", out, (V, 4), torch.float32))
    if V == 0:
        return out
    p = _abi.ExposureParams(C.sizeof(_abi.ExposureParams), V, min_log2, 0, key, low, high, rate, min_exposure, max_exposure)
    _check(lib().gnxr_exposure_device(C.byref(p), _ptr(hist), _ptr(prev), _ptr(out), _addr(hstream)))
    return out


TONEMAP_CURVES = {"linear": _abi.TONEMAP_LINEAR, "reference": _abi.TONEMAP_REFERENCE, "reinhard": _abi.TONEMAP_REINHARD, "aces": _abi.TONEMAP_ACES}


def tonemap(color, exposure=1.0, curve="aces", white=4.0, srgb=True, round=True, out=None, stream=None):
    """From a linear float image to bytes on the GPU (gnxr_tonemap_device; the definition, operation by operation: include/gnxr.h): every
    colour channel times the exposure, through `curve` -- "linear", "reference" (FrameBuffer's 1 - exp(-4x)), "reinhard" (extended, with
    the white point `white`) or "aces" (Narkowicz's fit) --, clamped to [0, 1], sRGB-encoded with `srgb`, then rounded to the nearest
    byte (`round`) or truncated, as FrameBuffer does.  `color`: a contiguous float32 tensor (H, W, 4) or (V, H, W, 4) on a GPU;
    `exposure`: a number, or the float32 (V, 4) tensor of auto_exposure, read on the device.  Returns a uint8 tensor of color's shape
    -- `out` when given --, alpha 255; save_png takes a view of it after .cpu().numpy().  Queued on `stream` (by default torch's current
    stream); the call does not wait for the GPU.  Malformed arguments raise ValueError."""
    import math
    import torch
    shape, V, H, W = _image("tonemap", "color", color)
    if curve not in TONEMAP_CURVES:
        raise ValueError(f"tonemap: curve must be one of {sorted(TONEMAP_CURVES)}, got {curve!r}")
    white = float(white)
    if not 1e-3 <= white <= 65504:
        raise ValueError(f"tonemap: white must lie in [1e-3, 65504], got {white}")
    d_exposure, e = None, 1.0
    if isinstance(exposure, torch.Tensor):
        if not _is_tensor(exposure, torch.float32, (V, 4), color.device):
            _refuse(exposure, f"tonemap: an exposure tensor must be a contiguous float32 ({V}, 4) tensor on {color.device} (auto_exposure)", type_name=False)
        d_exposure = exposure
    else:
        try:
            e = float(exposure)
        except (TypeError, ValueError):
            raise ValueError(f"tonemap: exposure must be a number or the tensor of auto_exposure, got {type(exposure).__name__}") from None
        if not (math.isfinite(e) and e >= 0):
            raise ValueError(f"tonemap: exposure must be finite and >= 0, got {e}")
    hstream, _, out = _outputs(stream, color.device, ("tonemap: out", out, shape, torch.uint8))
    if V == 0:
        return out
    flags = (_abi.TONEMAP_SRGB if srgb else 0) | (_abi.TONEMAP_ROUND if round else 0)
    p = _abi.TonemapParams(C.sizeof(_abi.TonemapParams), W, H, V, TONEMAP_CURVES[curve], flags, e, white)
    _check(lib().gnxr_tonemap_device(C.byref(p), _ptr(color), _ptr(d_exposure), _ptr(out), _addr(hstream)))
    return out


class Display:
    """The display stage of a frame loop: luminance_histogram -> auto_exposure -> tonemap, with the exposure record kept on the device
    between frames and updated in place -- nothing more: its result equals that chain of public calls on bits, and no frame waits for
    the GPU.

        acc = TemporalAccumulator(PathIntegrator(5), scene, 1920, 1080, spp=4)
        display = Display(1920, 1080, rate=0.1)
        for cam in orbit:
            shown = display.present(acc.frame(cam, denoise=True)["denoised"])      # shown["rgba8"]: (1080, 1920, 4) uint8

    The keyword arguments are those of the three calls: min_log2; key, low, high, rate, min_exposure, max_exposure; curve, white, srgb,
    round.  The first frame after the construction or a reset() takes its target exposure at once."""

    _HIST, _EXPOSURE, _TONEMAP = ("min_log2",), ("key", "low", "high", "rate", "min_exposure", "max_exposure"), ("curve", "white", "srgb", "round")

    def __init__(self, width, height, n_views=1, **kw):
        width, height, n_views = int(width), int(height), int(n_views)
        if width <= 0 or height <= 0 or n_views < 1:
            raise ValueError(f"Display: invalid size {n_views} x {width} x {height}")
        _only_kw("Display", kw, self._HIST + self._EXPOSURE + self._TONEMAP)
        self.width, self.height, self.n_views = width, height, n_views
        self.min_log2 = _min_log2("Display", kw.get("min_log2", -12))
        self.exposure_kw = {k: kw[k] for k in self._EXPOSURE if k in kw}
        self.tonemap_kw = {k: kw[k] for k in self._TONEMAP if k in kw}
        self._hist = self._record = None
        self.reset()

    def reset(self):
        """Forget the exposure: the next frame takes its target at once."""
        self.has_exposure = False

    def present(self, color, stream=None):
        """One frame.  `color`: a contiguous float32 tensor (V, H, W, 4), or (H, W, 4) with n_views == 1, on a GPU.  Returns {"rgba8": the
        uint8 tensor of color's shape, "exposure": the float32 (V, 4) record of auto_exposure, "hist": the int32 (V, 260) histogram};
        "exposure" and "hist" are the Display's own tensors, which the next frame overwrites.  Runs on `stream` (by default torch's
        current stream)."""
        import torch
        shape, V, H, W = _image("Display.present", "color", color)
        if (V, H, W) != (self.n_views, self.height, self.width):
            raise ValueError(f"Display.present: color is {V} x {H} x {W}, the display {self.n_views} x {self.height} x {self.width}")
        hstream, tstream = _stream_pair(stream, color.device)
        if self._hist is None or self._hist.device != color.device:
            with torch.cuda.stream(tstream):
                self._hist = torch.empty((V, _abi.HISTOGRAM_WORDS), dtype=torch.int32, device=color.device)
                self._record = torch.empty((V, 4), dtype=torch.float32, device=color.device)
            self.has_exposure = False
        hist = luminance_histogram(color, min_log2=self.min_log2, out=self._hist, stream=tstream)
        rec = auto_exposure(hist, prev=self._record if self.has_exposure else None, min_log2=self.min_log2, out=self._record, stream=tstream, **self.exposure_kw)
        self.has_exposure = True
        return {"rgba8": tonemap(color, exposure=rec, stream=tstream, **self.tonemap_kw), "exposure": rec, "hist": hist}


def save_png(path, rgba8):
    """FrameBuffer::saveToFile (ui/FrameBuffer.cpp:6-9): rgba8 is a [H, W, 4] uint8 array."""
    rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
    h, w = rgba8.shape[:2]
    _check(lib().gnxr_framebuffer_save_png(str(path).encode(), rgba8.ctypes.data_as(C.POINTER(C.c_uint8)), w, h))


def eval_libm(fn, x, x2=None):
    """Test hook: the device's float libm (fn = "log" | "exp" | "sin" | "cos" | "acos" | "atan2") on the array x (atan2: y = x, x = x2)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(x)
    p2 = None
    if x2 is not None:
        x2 = np.ascontiguousarray(x2, dtype=np.float32)
        p2 = x2.ctypes.data_as(C.POINTER(C.c_float))
    code = {"log": 0, "exp": 1, "sin": 2, "cos": 3, "sincos.sin": 4, "sincos.cos": 5, "acos": 6, "atan2": 7, "pow": 8}[fn]
    _check(lib().gnxr_eval_libm(code, x.ctypes.data_as(C.POINTER(C.c_float)), p2, x.size, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def eval_libm_f64(fn, x):
    """Test hook: the device's double-precision sin / cos / sqrt / tan on float arguments (widened), results as float64."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.float64)
    _check(lib().gnxr_eval_libm_f64({"sin": 0, "cos": 1, "sqrt": 2, "tan": 3}[fn], x.ctypes.data_as(C.POINTER(C.c_float)), x.size,
                                    out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def probe_valu_peak():
    """Measurement hook: VALU issue rate of the device in 1e9 wave64 instructions / s (independent v_fma_f32 chains, 8 waves per SIMD)."""
    v = C.c_double(0.0)
    _check(lib().gnxr_probe_valu_peak(C.byref(v)))
    return v.value


def probe_gather_peak():
    """Measurement hook: per-lane 16-byte gather rate of the device in 1e9 lane-loads / s (8 dwordx4 of a random 128-byte record per lane)."""
    v = C.c_double(0.0)
    _check(lib().gnxr_probe_gather_peak(C.byref(v)))
    return v.value


def framebuffer_update(running_mean, frame, frame_count):
    """FrameBuffer::update_f_u_c (ui/FrameBuffer.h:127-149): running mean + 1-exp(-4x) tone map to RGBA8."""
    h, w = frame.shape[:2]
    rgba8 = np.zeros((h, w, 4), dtype=np.uint8)
    _check(lib().gnxr_framebuffer_update(running_mean.ctypes.data_as(C.POINTER(C.c_float)),
                                         np.ascontiguousarray(frame, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                         w, h, int(frame_count), rgba8.ctypes.data_as(C.POINTER(C.c_uint8))))
    return rgba8
