"""ctypes mirror of include/gnxr.h (the C ABI of libgnxr.so).

Only data layout and prototypes live here; no compute.  The structures must match
include/gnxr.h field for field (tests/test_abi.py checks sizes and exported symbols).
"""
import ctypes as C

GNXR_ABI_VERSION = 5

# gnxr_status
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_OOM, ERR_UNSUPPORTED, ERR_IO, ERR_RUNTIME = 0, -1, -2, -3, -4, -5, -6
# gnxr_material_type
MAT_NONE, MAT_MATTE, MAT_MIRROR, MAT_GLASS, MAT_METAL, MAT_PLASTIC, MAT_DISNEY = range(7)
# gnxr_light_type
LIGHT_AREA_TRI, LIGHT_INFINITE, LIGHT_SKYBOX, LIGHT_POINT, LIGHT_SPOT, LIGHT_DISTANT = 1, 2, 3, 4, 5, 6
# gnxr_integrator / gnxr_light_strategy
INTEGRATOR_PATH, INTEGRATOR_VOLPATH, INTEGRATOR_WHITTED, INTEGRATOR_DIRECT = 0, 1, 2, 3
DIRECT_SAMPLE_ALL, DIRECT_SAMPLE_ONE = 0, 1
LIGHTS_SPATIAL, LIGHTS_UNIFORM, LIGHTS_POWER = 0, 1, 2
MEDIUM_HOMOGENEOUS, MEDIUM_GRID = 1, 2
NEAR_ALL, NEAR_NEAREST = 0, 1   # GNXR_NEAR_*: the flag word of gnxr_near_device
DMEDIUM_BYTES = 128   # one record of gnxr_scene_media_tables(which = 0): sizeof(DMedium), csrc/gnxr_device_types.h
DLIGHT_BYTES = 112   # one record of gnxr_scene_light_tables(which = 0): sizeof(DLight), csrc/gnxr_device_types.h
DTEXTURE_BYTES = 112   # one record of gnxr_scene_texture_tables(which = 0): sizeof(DTexture), csrc/gnxr_device_types.h
# flags of gnxr_scene_update_vertices_ex
UPDATE_MOVE_LIGHTS = 1

f32, i32, u8, i64, u32, u64 = C.c_float, C.c_int32, C.c_uint8, C.c_int64, C.c_uint32, C.c_uint64


class Material(C.Structure):
    _fields_ = [
        ("type", i32), ("has_bump", i32), ("remap_roughness", i32), ("disney_thin", i32),
        ("kd", f32 * 3), ("ks", f32 * 3), ("kr", f32 * 3), ("kt", f32 * 3), ("eta", f32 * 3), ("k", f32 * 3),
        ("sigma", f32), ("urough", f32), ("vrough", f32),
        ("disney_metallic", f32), ("disney_spec_trans", f32), ("disney_spec_tint", f32), ("disney_sheen", f32),
        ("disney_sheen_tint", f32), ("disney_clearcoat", f32), ("disney_clearcoat_gloss", f32),
        ("disney_anisotropic", f32), ("disney_roughness", f32), ("disney_flatness", f32), ("disney_diff_trans", f32),
        ("disney_scatter_distance", f32 * 3), ("kd_texture", i32), ("ks_texture", i32),
    ]


class Light(C.Structure):
    _fields_ = [
        ("type", i32), ("tri", i32), ("two_sided", i32), ("n_samples", i32),
        ("le", f32 * 3), ("radius", f32), ("center", f32 * 3), ("falloff_start", f32), ("light_to_world", f32 * 16),
    ]


class Camera(C.Structure):
    _fields_ = [("eye", f32 * 3), ("look", f32 * 3), ("up", f32 * 3), ("fov_deg", f32), ("lens_radius", f32),
                ("focal_distance", f32), ("orthographic", i32)]


class Medium(C.Structure):
    _fields_ = [("type", i32), ("nx", i32), ("ny", i32), ("nz", i32), ("sigma_a", f32 * 3), ("sigma_s", f32 * 3),
                ("g", f32), ("_pad", f32), ("medium_to_world", f32 * 16), ("density_offset", i64)]


class Sphere(C.Structure):
    _fields_ = [("center", f32 * 3), ("radius", f32), ("material", i32), ("medium_inside", i32), ("medium_outside", i32), ("_pad", i32)]


class Texture(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("texel_offset", i64), ("su", f32), ("sv", f32), ("du", f32), ("dv", f32),
                ("max_aniso", f32), ("scale", f32), ("trilinear", i32), ("wrap", i32), ("gamma", i32), ("_pad", i32)]


WRAP_REPEAT, WRAP_BLACK, WRAP_CLAMP = 0, 1, 2


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("n_vertices", i32), ("n_triangles", i32), ("n_materials", i32), ("n_lights", i32),
        ("n_media", i32), ("env_width", i32), ("env_height", i32),
        ("vertices", C.POINTER(f32)), ("indices", C.POINTER(i32)), ("tri_material", C.POINTER(i32)),
        ("tri_light", C.POINTER(i32)), ("tri_medium_inside", C.POINTER(i32)), ("tri_medium_outside", C.POINTER(i32)),
        ("materials", C.POINTER(Material)), ("lights", C.POINTER(Light)), ("media", C.POINTER(Medium)),
        ("grid_density", C.POINTER(f32)), ("env_rgb", C.POINTER(f32)),
        ("camera", Camera), ("camera_medium", i32), ("n_spheres", i32), ("spheres", C.POINTER(Sphere)),
        ("n_textures", i32), ("_pad", i32), ("textures", C.POINTER(Texture)), ("texels", C.POINTER(f32)),
        ("tri_uv", C.POINTER(f32)), ("tri_n", C.POINTER(f32)), ("tri_s", C.POINTER(f32)),
        ("bvh_split_method", i32), ("_pad2", i32),
    ]


class RenderParams(C.Structure):
    _fields_ = [
        ("width", i32), ("height", i32), ("spp", i32), ("spp_begin", i32), ("spp_end", i32), ("max_depth", i32),
        ("rr_threshold", f32), ("integrator", i32), ("light_strategy", i32),
        ("shard_index", i32), ("shard_count", i32), ("shard_rows", i32), ("samples_per_pass", i32), ("direct_strategy", i32),
        ("passes_in_flight", i32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("rays_closest", u64), ("rays_any", u64), ("camera_samples", u64), ("nodes_visited", u64), ("tris_tested", u64),
        ("seconds_render", C.c_double), ("seconds_trace", C.c_double), ("seconds_total", C.c_double),
        ("kernel_launches", u32), ("passes", u32),
        ("seconds_closest", C.c_double), ("seconds_nee", C.c_double), ("seconds_shade", C.c_double),
        ("launches_closest", u32), ("launches_nee", u32), ("rays_closest_nee", u64),
        ("media_segments", u64), ("media_steps", u64), ("leaf_retests", u64), ("nodes_from_memory", u64),
        ("passes_in_flight", u32), ("loop_iterations", u32), ("state_bytes", u64),
    ]


class Ray(C.Structure):
    _fields_ = [("o", f32 * 3), ("tmax", f32), ("d", f32 * 3), ("_pad", f32)]


class Hit(C.Structure):
    _fields_ = [("prim", i32), ("t", f32), ("b0", f32), ("b1", f32), ("b2", f32), ("n", f32 * 3)]


class PointQuery(C.Structure):   # gnxr_point_query (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("p", f32 * 3), ("max_distance", f32)]


class ClosestPoint(C.Structure):   # gnxr_closest_point (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("prim", i32), ("dist2", f32), ("p", f32 * 3), ("b1", f32), ("b2", f32), ("feature", i32)]


class RayHit(C.Structure):   # gnxr_ray_hit (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("t", f32), ("prim", i32), ("b1", f32), ("b2", f32)]


class SphereCast(C.Structure):   # gnxr_sphere_cast (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("o", f32 * 3), ("radius", f32), ("d", f32 * 3), ("tmax", f32)]


class BoxQuery(C.Structure):   # gnxr_box_query (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("lo", f32 * 3), ("_pad0", f32), ("hi", f32 * 3), ("_pad1", f32)]


OVERLAP_TRI_SKIP_SHARED, OVERLAP_TRI_SELF = 1, 2   # GNXR_OVERLAP_TRI_*: the flags of gnxr_overlap_tri_device


class TriQuery(C.Structure):   # gnxr_tri_query (no struct_size; not in gnxr_abi_sizeof's list)
    _fields_ = [("a", f32 * 3), ("_pad0", f32), ("b", f32 * 3), ("_pad1", f32), ("c", f32 * 3), ("_pad2", f32)]


class LiSample(C.Structure):
    _fields_ = [("px", i32), ("py", i32), ("s", i32), ("medium", i32)]


class BsdfResult(C.Structure):
    _fields_ = [("f", f32 * 3), ("pdf", f32), ("sample_f", f32 * 3), ("sample_pdf", f32), ("sample_wi", f32 * 3), ("sampled_type", i32),
                ("n_components", i32), ("valid", i32), ("dudx", f32), ("dvdy", f32)]


class AovBuffers(C.Structure):
    _fields_ = [("d_albedo", C.c_void_p), ("d_normal", C.c_void_p), ("d_shading_normal", C.c_void_p), ("d_depth", C.c_void_p), ("d_ids", C.c_void_p)]


class LightResult(C.Structure):
    _fields_ = [("Li", f32 * 3), ("pdf", f32), ("wi", f32 * 3), ("pdf_li", f32), ("pdf_select", f32), ("p_light", f32 * 3)]


class TracePlan(C.Structure):   # gnxr_trace_plan (gnxr_scene_trace_plan)
    _fields_ = [("wide", i32), ("stack_entries", i32), ("lds_entries", i32), ("n_top", i32), ("hot_bytes", i32), ("blocks", i32), ("blocks_per_cu", i32), ("_pad", i32),
                ("lds_bytes", i64)]


class Geometry(C.Structure):   # gnxr_geometry: the arrays are host or device addresses (not in gnxr_abi_sizeof's list: it carries struct_size)
    _fields_ = [("struct_size", i32), ("n_vertices", i32), ("n_triangles", i32), ("_pad", i32),
                ("vertices", C.c_void_p), ("indices", C.c_void_p), ("tri_material", C.c_void_p), ("tri_light", C.c_void_p),
                ("tri_medium_inside", C.c_void_p), ("tri_medium_outside", C.c_void_p), ("tri_uv", C.c_void_p), ("tri_n", C.c_void_p), ("tri_s", C.c_void_p)]


class AdaptiveParams(C.Structure):   # gnxr_adaptive_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("min_spp", i32), ("step_spp", i32), ("guard", i32), ("threshold", f32), ("floor", f32)]


class AdaptiveInfo(C.Structure):   # gnxr_adaptive_info (carries struct_size)
    _fields_ = [("struct_size", i32), ("rounds", i32), ("samples", i64), ("pixels_at_budget", i64)]


class DenoiseParams(C.Structure):   # gnxr_denoise_params (carries struct_size)
    _fields_ = [("struct_size", i32), ("width", i32), ("height", i32), ("n_views", i32), ("iterations", i32),
                ("sigma_color", f32), ("sigma_normal", f32), ("sigma_depth", f32)]


class DenoiseBuffers(C.Structure):   # gnxr_denoise_buffers (carries struct_size): device addresses, NULL = not given
    _fields_ = [("struct_size", i32), ("_pad", i32), ("d_color", C.c_void_p), ("d_color_b", C.c_void_p), ("d_albedo", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_depth", C.c_void_p)]


class FilmFilter(C.Structure):   # gnxr_film_filter (carries struct_size): table is host memory, 256 floats, or NULL
    _fields_ = [("struct_size", i32), ("kind", i32), ("radius_x", f32), ("radius_y", f32), ("a", f32), ("b", f32), ("table", C.POINTER(f32))]


class BakeParams(C.Structure):   # gnxr_bake_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("flags", u32), ("dilate", i32), ("medium", i32)]


BAKE_FLIP_NORMALS = 1   # flags of gnxr_surface_rays_device / gnxr_bake_params


class LightprobeParams(C.Structure):   # gnxr_lightprobe_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("flags", u32), ("medium", i32)]


SH_CONTINUE = 1   # flags of gnxr_sh_project_device


class MotionParams(C.Structure):   # gnxr_motion_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("width", i32), ("height", i32), ("n_views", i32)]


class MotionBuffers(C.Structure):   # gnxr_motion_buffers (carries struct_size): device addresses, NULL = channel not wanted
    _fields_ = [("struct_size", i32), ("_pad", i32), ("d_motion", C.c_void_p), ("d_guide", C.c_void_p), ("d_prim", C.c_void_p)]


class TemporalParams(C.Structure):   # gnxr_temporal_params (carries struct_size)
    _fields_ = [("struct_size", i32), ("width", i32), ("height", i32), ("n_views", i32), ("max_history", i32), ("depth_tol", f32), ("normal_cos", f32)]


class TemporalBuffers(C.Structure):   # gnxr_temporal_buffers (carries struct_size): device addresses; the history is all set or all NULL
    _fields_ = [("struct_size", i32), ("_pad", i32), ("d_color", C.c_void_p), ("d_motion", C.c_void_p), ("d_guide", C.c_void_p), ("d_prim", C.c_void_p),
                ("d_hist_color", C.c_void_p), ("d_hist_stat", C.c_void_p), ("d_hist_guide", C.c_void_p), ("d_hist_prim", C.c_void_p),
                ("d_out_color", C.c_void_p), ("d_out_stat", C.c_void_p)]


class HistogramParams(C.Structure):   # gnxr_histogram_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("width", i32), ("height", i32), ("n_views", i32), ("min_log2", i32)]


class ExposureParams(C.Structure):   # gnxr_exposure_params (carries struct_size)
    _fields_ = [("struct_size", i32), ("n_views", i32), ("min_log2", i32), ("_pad", i32), ("key", f32), ("low", f32), ("high", f32), ("rate", f32),
                ("min_exposure", f32), ("max_exposure", f32)]


class TonemapParams(C.Structure):   # gnxr_tonemap_params (carries struct_size)
    _fields_ = [("struct_size", i32), ("width", i32), ("height", i32), ("n_views", i32), ("curve", i32), ("flags", u32), ("exposure", f32), ("white", f32)]


HISTOGRAM_WORDS = 260   # uint32 per view of gnxr_luminance_histogram_device: 256 bins, below, above, not finite, 0
TONEMAP_LINEAR, TONEMAP_REFERENCE, TONEMAP_REINHARD, TONEMAP_ACES = range(4)   # curve of gnxr_tonemap_params
TONEMAP_SRGB, TONEMAP_ROUND = 1, 2   # flags of gnxr_tonemap_params

class SkinParams(C.Structure):   # gnxr_skin_params (carries struct_size: not in gnxr_abi_sizeof's list)
    _fields_ = [("struct_size", i32), ("n_vertices", i32), ("n_bones", i32), ("n_morphs", i32)]


NORMALS_FLIP = 1   # flags of gnxr_scene_recompute_normals

# kind of gnxr_film_filter / flags of gnxr_render_filtered_device
FILTER_BOX, FILTER_TRIANGLE, FILTER_GAUSSIAN, FILTER_MITCHELL, FILTER_TABLE = range(5)
FILM_CONTINUE = 1

P = C.POINTER
VP = C.c_void_p

# name -> (restype, argtypes); every symbol include/gnxr.h declares
PROTOTYPES = {
    "gnxr_abi_version": (C.c_int, []),
    "gnxr_abi_sizeof": (C.c_int, [C.c_int]),
    "gnxr_init": (C.c_int, [C.c_int]),
    "gnxr_shutdown": (None, []),
    "gnxr_last_error": (C.c_char_p, []),
    "gnxr_init_devices": (C.c_int, [i32, P(i32)]),
    "gnxr_set_profiling": (C.c_int, [C.c_int]),
    "gnxr_probe_valu_peak": (C.c_int, [P(C.c_double)]),
    "gnxr_probe_gather_peak": (C.c_int, [P(C.c_double)]),
    "gnxr_scene_create": (C.c_int, [P(SceneDesc), P(VP)]),
    "gnxr_scene_destroy": (None, [VP]),
    "gnxr_scene_info": (C.c_int, [VP, P(i32), P(i32), P(i32)]),
    "gnxr_scene_update_vertices": (C.c_int, [VP, i32, i32, VP, VP]),   # xyz: host or device address
    "gnxr_scene_update_vertices_ex": (C.c_int, [VP, i32, i32, VP, u32, VP]),   # ..., flags (UPDATE_MOVE_LIGHTS), hipStream_t
    "gnxr_scene_update_lights": (C.c_int, [VP, i32, i32, P(Light)]),
    "gnxr_scene_set_lights": (C.c_int, [VP, P(Light), i32, VP]),   # scene, records, count, hipStream_t
    "gnxr_scene_light_tables": (C.c_int, [VP, i32, VP, i64, P(i64)]),   # scene, which, out, capacity in bytes, size in bytes
    "gnxr_scene_rebuild_bvh": (C.c_int, [VP, VP]),   # scene, hipStream_t
    "gnxr_scene_set_geometry": (C.c_int, [VP, P(Geometry), VP]),   # scene, record of host or device arrays, hipStream_t
    "gnxr_scene_update_environment": (C.c_int, [VP, P(Light), VP, i32, i32, VP]),   # scene, record, host or device fp32 map (or NULL), width, height, hipStream_t
    "gnxr_scene_env_tables": (C.c_int, [VP, i32, VP, i64, P(i64)]),   # scene, which, out, capacity in bytes, size in bytes
    "gnxr_scene_update_media": (C.c_int, [VP, i32, i32, P(Medium), VP, VP]),   # scene, first, n, records, host or device fp32 grids (or NULL), hipStream_t
    "gnxr_scene_media_tables": (C.c_int, [VP, i32, i32, VP, i64, P(i64)]),   # scene, which, medium, out, capacity in bytes, size in bytes
    "gnxr_scene_update_textures": (C.c_int, [VP, i32, i32, P(Texture), VP, VP]),   # scene, first, n, records, host or device fp32 texels (or NULL), hipStream_t
    "gnxr_scene_texture_tables": (C.c_int, [VP, i32, i32, VP, i64, P(i64)]),   # scene, which, texture, out, capacity in bytes, size in bytes
    "gnxr_scene_update_materials": (C.c_int, [VP, i32, i32, P(Material)]),
    "gnxr_scene_set_triangle_materials": (C.c_int, [VP, i32, i32, VP, VP]),   # scene, first, n, host or device int32 ids, hipStream_t
    "gnxr_scene_triangle_materials": (C.c_int, [VP, P(i32), P(C.c_uint8), C.c_int64]),
    "gnxr_scene_set_camera": (C.c_int, [VP, P(Camera), i32]),
    "gnxr_render": (C.c_int, [VP, P(RenderParams), P(f32), P(Stats)]),
    "gnxr_render_device": (C.c_int, [VP, P(RenderParams), VP, VP, P(Stats)]),
    "gnxr_render_reserve": (C.c_int, [VP, P(RenderParams)]),
    "gnxr_scene_nee_apply_counts": (C.c_int, [VP, P(u64), P(u64)]),
    "gnxr_scene_hot_leaf_counts": (C.c_int, [VP, P(u64), P(u64)]),
    "gnxr_scene_trace_plan": (C.c_int, [VP, i64, P(TracePlan)]),
    "gnxr_trace_closest": (C.c_int, [VP, P(Ray), i64, P(Hit)]),
    "gnxr_trace_any": (C.c_int, [VP, P(Ray), i64, P(u8)]),
    "gnxr_trace_closest_device": (C.c_int, [VP, VP, i64, VP, VP]),   # device addresses + hipStream_t
    "gnxr_trace_any_device": (C.c_int, [VP, VP, i64, VP, VP]),
    "gnxr_closest_point_device": (C.c_int, [VP, VP, i64, VP, VP]),   # device addresses + hipStream_t
    "gnxr_closest_point_counted_device": (C.c_int, [VP, VP, i64, VP, VP, VP]),   # ..., two uint64 on the device, hipStream_t
    "gnxr_closest_point": (C.c_int, [VP, P(PointQuery), i64, P(ClosestPoint)]),
    "gnxr_trace_all_device": (C.c_int, [VP, VP, i64, i32, VP, VP, VP]),   # rays, n, max_hits, hits, counts: device addresses + hipStream_t
    "gnxr_trace_all_counted_device": (C.c_int, [VP, VP, i64, i32, VP, VP, VP, VP]),   # ..., three uint64 on the device, hipStream_t
    "gnxr_trace_all": (C.c_int, [VP, P(Ray), i64, i32, P(RayHit), P(i32)]),
    "gnxr_near_device": (C.c_int, [VP, VP, i64, i32, u32, VP, VP, VP]),   # queries, n, max_near, flags, records, counts: device addresses + hipStream_t
    "gnxr_near_counted_device": (C.c_int, [VP, VP, i64, i32, u32, VP, VP, VP, VP]),   # ..., two uint64 on the device, hipStream_t
    "gnxr_near": (C.c_int, [VP, P(PointQuery), i64, i32, u32, P(ClosestPoint), P(i32)]),
    "gnxr_sphere_cast_device": (C.c_int, [VP, VP, i64, VP, VP]),   # casts, n, records: device addresses + hipStream_t
    "gnxr_sphere_cast_counted_device": (C.c_int, [VP, VP, i64, VP, VP, VP]),   # ..., two uint64 on the device, hipStream_t
    "gnxr_sphere_cast": (C.c_int, [VP, P(SphereCast), i64, P(ClosestPoint)]),
    "gnxr_overlap_box_device": (C.c_int, [VP, VP, i64, i32, VP, VP, VP, VP]),   # boxes, n, max_prims, offsets (or NULL), prims, counts: device addresses + hipStream_t
    "gnxr_overlap_box_counted_device": (C.c_int, [VP, VP, i64, i32, VP, VP, VP, VP, VP]),   # ..., two uint64 on the device, hipStream_t
    "gnxr_overlap_box": (C.c_int, [VP, P(BoxQuery), i64, i32, P(i64), P(i32), P(i32)]),
    "gnxr_overlap_tri_device": (C.c_int, [VP, VP, i64, u32, i32, VP, VP, VP, VP]),   # tris (NULL with SELF), n, flags, max_prims, offsets (or NULL), prims, counts: device addresses + hipStream_t
    "gnxr_overlap_tri_counted_device": (C.c_int, [VP, VP, i64, u32, i32, VP, VP, VP, VP, VP]),   # ..., two uint64 on the device, hipStream_t
    "gnxr_overlap_tri": (C.c_int, [VP, P(TriQuery), i64, u32, i32, P(i64), P(i32), P(i32)]),
    "gnxr_li_device": (C.c_int, [VP, P(RenderParams), VP, VP, i64, VP, VP, P(Stats)]),   # device addresses + hipStream_t
    "gnxr_render_views_device": (C.c_int, [VP, P(RenderParams), P(Camera), P(i32), i32, VP, VP, P(Stats)]),   # cameras, media: host; images: device
    "gnxr_render_aov_device": (C.c_int, [VP, P(RenderParams), P(Camera), P(i32), i32, P(AovBuffers), VP, P(Stats)]),   # cameras, media: host; buffers: device
    "gnxr_render_adaptive_device": (C.c_int, [VP, P(RenderParams), P(AdaptiveParams), VP, VP, VP, P(Stats), P(AdaptiveInfo)]),   # image, counts: device; hipStream_t
    "gnxr_denoise_device": (C.c_int, [P(DenoiseParams), P(DenoiseBuffers), VP, VP]),   # buffers, image: device; hipStream_t
    "gnxr_film_filter_table": (C.c_int, [P(FilmFilter), P(f32)]),   # host: record -> the 16 x 16 table
    "gnxr_film_add_device": (C.c_int, [P(FilmFilter), i32, i32, i32, i32, VP, VP, VP, VP]),   # width, height, views, layers; L, offsets, accum: device; hipStream_t
    "gnxr_film_resolve_device": (C.c_int, [i32, i32, i32, VP, VP, VP]),   # width, height, views; accum, image: device; hipStream_t
    "gnxr_render_filtered_device": (C.c_int, [VP, P(RenderParams), P(FilmFilter), P(Camera), P(i32), i32, VP, VP, u32, VP, P(Stats)]),   # cameras, media: host; image, accum: device; flags
    "gnxr_bake_texels_device": (C.c_int, [VP, VP, i32, i32, VP, VP, VP]),   # scene; lightmap uvs: device; width, height; tri, bary: device; hipStream_t
    "gnxr_surface_rays_device": (C.c_int, [VP, i32, i32, VP, VP, VP, VP, VP, i64, u32, i32, VP, VP, VP, VP]),   # scene, width, height; tri, bary, px, py, s; n, flags, medium; rays, samples, pn; hipStream_t
    "gnxr_bake_dilate_device": (C.c_int, [i32, i32, i32, VP, VP]),   # width, height, iterations; image: device; hipStream_t
    "gnxr_bake_lightmap_device": (C.c_int, [VP, P(RenderParams), P(BakeParams), VP, VP, VP, P(Stats)]),   # lightmap uvs, image: device; hipStream_t
    "gnxr_lightprobe_rays_device": (C.c_int, [VP, i32, i32, VP, VP, VP, VP, i64, i32, VP, VP, VP]),   # scene, width, height; pos, px, py, s; n, medium; rays, samples; hipStream_t
    "gnxr_sh_project_device": (C.c_int, [VP, VP, i32, i64, VP, u32, VP]),   # rays, L: device; n_probes, n_samples; sums: device; flags; hipStream_t
    "gnxr_bake_lightprobes_device": (C.c_int, [VP, P(RenderParams), P(LightprobeParams), VP, i32, VP, VP, P(Stats)]),   # positions; n_probes; coefficients: device; hipStream_t
    "gnxr_sh_irradiance_device": (C.c_int, [VP, i32, VP, VP, i64, VP, VP]),   # coefficients; n_probes; probe, normals; n; E: device; hipStream_t
    "gnxr_camera_matrices": (C.c_int, [P(Camera), i32, i32, P(f32), P(f32), P(f32)]),   # host: r2c, c2w, w2r (16 floats each, any may be NULL)
    "gnxr_motion_device": (C.c_int, [VP, P(MotionParams), P(Camera), P(Camera), VP, P(MotionBuffers), VP]),   # cameras, previous cameras: host; previous vertices: device; hipStream_t
    "gnxr_temporal_accumulate_device": (C.c_int, [P(TemporalParams), P(TemporalBuffers), VP]),   # buffers: device; hipStream_t
    "gnxr_luminance_histogram_device": (C.c_int, [P(HistogramParams), VP, VP, VP]),   # image, histogram: device; hipStream_t
    "gnxr_exposure_device": (C.c_int, [P(ExposureParams), VP, VP, VP, VP]),   # histogram, previous records (or NULL), records: device; hipStream_t
    "gnxr_tonemap_device": (C.c_int, [P(TonemapParams), VP, VP, VP, VP]),   # image, exposure records (or NULL), RGBA8: device; hipStream_t
    "gnxr_scene_update_attributes": (C.c_int, [VP, i32, i32, VP, VP, VP, VP]),   # scene, first, n, host or device fp32 uv / normal / tangent rows (or NULL), hipStream_t
    "gnxr_scene_triangle_attributes": (C.c_int, [VP, i32, P(f32), i64, P(i64)]),   # scene, which, out, capacity in floats, size in floats
    "gnxr_scene_recompute_normals": (C.c_int, [VP, u32, VP]),   # scene, flags (NORMALS_FLIP), hipStream_t
    "gnxr_skin_vertices_device": (C.c_int, [P(SkinParams), VP, VP, VP, VP, VP, VP, VP, VP]),   # rest, bone index, bone weight, bones, morph deltas, morph weights, out: device; hipStream_t
    "gnxr_material_albedo": (C.c_int, [P(Material), P(f32)]),
    "gnxr_camera_rays_device": (C.c_int, [P(Camera), i32, i32, i32, VP, VP, VP, i64, VP, VP, VP]),   # device addresses + hipStream_t
    "gnxr_bsdf_device": (C.c_int, [VP, VP, VP, VP, VP, i64, i32, VP, VP]),   # device addresses + hipStream_t
    "gnxr_light_sample_device": (C.c_int, [VP, VP, i64, i32, VP, VP]),
    "gnxr_light_le_device": (C.c_int, [VP, i32, VP, i64, VP, VP]),
    "gnxr_sample_halton": (C.c_int, [i32, i32, P(i32), P(i32), P(i64), P(i32), i64, P(f32)]),
    "gnxr_camera_rays": (C.c_int, [P(Camera), i32, i32, P(i32), P(i32), P(i64), i64, P(f32), P(f32)]),
    "gnxr_framebuffer_update": (C.c_int, [P(f32), P(f32), i32, i32, i32, P(u8)]),
    "gnxr_framebuffer_save_png": (C.c_int, [C.c_char_p, P(u8), i32, i32]),
    "gnxr_light_grid_table": (C.c_int, [VP, i32, i32, P(f32), i64, P(i64)]),
    "gnxr_eval_libm": (C.c_int, [i32, P(f32), P(f32), i64, P(f32)]),
    "gnxr_eval_libm_f64": (C.c_int, [i32, P(f32), i64, P(C.c_double)]),
    "gnxr_builder_create": (C.c_int, [P(VP)]),
    "gnxr_builder_set_camera_medium": (C.c_int, [VP, i32]),
    "gnxr_builder_add_sphere": (C.c_int, [VP, P(f32), f32, i32, i32, i32]),
    "gnxr_builder_destroy": (None, [VP]),
    "gnxr_builder_add_material": (C.c_int, [VP, P(Material)]),
    "gnxr_builder_matte": (C.c_int, [VP, P(f32), f32]),
    "gnxr_builder_mirror": (C.c_int, [VP, P(f32)]),
    "gnxr_builder_purple_plastic": (C.c_int, [VP]),
    "gnxr_builder_yellow_metal": (C.c_int, [VP]),
    "gnxr_builder_white_glass": (C.c_int, [VP]),
    "gnxr_builder_add_mesh": (C.c_int, [VP, P(f32), i32, P(i32), i32, P(f32), i32, i32, i32]),
    "gnxr_builder_add_model_3d": (C.c_int, [VP, C.c_char_p, i32]),
    "gnxr_builder_add_cornell": (C.c_int, [VP, i32, i32, i32]),
    "gnxr_builder_add_floor": (C.c_int, [VP, i32]),
    "gnxr_builder_add_area_light": (C.c_int, [VP, i32]),
    "gnxr_builder_add_sky_light": (C.c_int, [VP]),
    "gnxr_builder_add_inf_light": (C.c_int, [VP, C.c_char_p]),
    "gnxr_builder_add_inf_light_data": (C.c_int, [VP, P(f32), i32, i32, P(f32), P(f32)]),
    "gnxr_builder_add_medium": (C.c_int, [VP, P(Medium), P(f32)]),
    "gnxr_builder_add_volume_file": (C.c_int, [VP, C.c_char_p, f32, f32, P(f32)]),
    "gnxr_builder_add_emissive_mesh": (C.c_int, [VP, P(f32), i32, P(i32), i32, P(f32), i32, P(f32), i32]),
    "gnxr_builder_add_spot_light": (C.c_int, [VP]),
    "gnxr_builder_add_dist_light": (C.c_int, [VP]),
    "gnxr_builder_add_light": (C.c_int, [VP, P(Light)]),
    "gnxr_builder_add_texture_data": (C.c_int, [VP, P(Texture), P(f32), i32, i32]),
    "gnxr_builder_add_texture_file": (C.c_int, [VP, P(Texture), C.c_char_p]),
    "gnxr_builder_set_material_texture": (C.c_int, [VP, i32, i32, i32]),
    "gnxr_builder_set_triangle_uv": (C.c_int, [VP, i32, i32, P(f32)]),
    "gnxr_builder_set_triangle_normals": (C.c_int, [VP, i32, i32, P(f32)]),
    "gnxr_builder_set_triangle_tangents": (C.c_int, [VP, i32, i32, P(f32)]),
    "gnxr_builder_set_bvh_split_method": (C.c_int, [VP, i32]),
    "gnxr_scene_bvh": (C.c_int, [VP, P(f32), P(i32), P(i32), i64, P(i64)]),
    "gnxr_scene_bvh4": (C.c_int, [VP, VP, i64, P(i64), P(i32), P(i32)]),
    "gnxr_builder_set_camera": (C.c_int, [VP, P(Camera)]),
    "gnxr_builder_desc": (C.c_int, [VP, P(SceneDesc)]),
    "gnxr_write_synthetic_3d": (C.c_int, [C.c_char_p, i32, u32]),
}


ABI_STRUCTS = [Material, Light, Camera, Medium, SceneDesc, RenderParams, Stats, Ray, Hit, Sphere, Texture, LiSample]
# gnxr_abi_sizeof(12), gnxr_abi_sizeof(13): the records of the shading queries.  A table of their own: index i of ABI_STRUCTS is
# gnxr_abi_sizeof(i) and tests/test_li_device.py pins gnxr_li_sample as its last entry.
ABI_STRUCTS_SHADING = {12: BsdfResult, 13: LightResult}


def bind(lib):
    """Attach prototypes; raises AttributeError naming the first missing symbol."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
