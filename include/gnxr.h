/*
 * gnxr.h -- C ABI of the MI355X wavefront path-tracing core (libgnxr.so).
 *
 * This is the drop-in boundary for the reference's render hot path.  The reference
 * (zhouxuguang/GNXRayTracer) has no FFI of its own; its two seams are C++ virtuals:
 *
 *   - Integrator seam : pbr::Integrator::Render(const Scene&, double& timeConsume)
 *                       core/Integrator.h:17-23, called from ui/RenderThread.cpp:175
 *   - Aggregate seam  : pbr::Primitive::Intersect / IntersectP
 *                       core/Primitive.h:13-27, reached via core/Scene.h:32-35
 *
 * A live pbr::Scene cannot be flattened from outside (all members private), so the
 * scene crosses the boundary where it is *authored* (ui/ModelList.cpp, ui/MaterialList.cpp,
 * ui/RenderThread.cpp:46-187) as plain arrays: gnxr_scene_desc below.
 *
 * Conventions: extern "C", plain pointers and sizes, no C++/torch types.  The caller owns
 * every input and output buffer; the library copies what it needs at gnxr_scene_create and
 * owns the device memory behind the opaque handle.  Every entry point returns 0 on success
 * and a negative gnxr_status on failure; gnxr_last_error() returns a thread-local message.
 * Nothing throws across the boundary (the reference builds with exceptions disabled on
 * Apple, CMakeLists.txt:252-253).  There is NO CPU fallback: without a HIP device every
 * compute entry point fails with GNXR_ERR_NO_DEVICE.
 */
#ifndef GNXR_H
#define GNXR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNXR_ABI_VERSION 5   /* 5: gnxr_render_params::passes_in_flight; gnxr_stats::passes_in_flight / loop_iterations / state_bytes */

typedef enum gnxr_status {
    GNXR_OK = 0,
    GNXR_ERR_INVALID = -1,    /* bad argument / inconsistent description            */
    GNXR_ERR_NO_DEVICE = -2,  /* no HIP device (or no such device); there is no CPU fallback */
    GNXR_ERR_OOM = -3,        /* host or device allocation failed                     */
    GNXR_ERR_UNSUPPORTED = -4,/* feature present in the description but not built    */
    GNXR_ERR_IO = -5,         /* file could not be read / written                     */
    GNXR_ERR_RUNTIME = -6     /* a HIP call failed at run time (launch, copy, synchronise); message in gnxr_last_error() */
} gnxr_status;

/* ---- materials: materials/{Matte,Mirror,Glass,Metal,Plastic,Disney}Material.cpp ---- */
typedef enum gnxr_material_type {
    GNXR_MAT_NONE = 0,     /* null material: medium boundary, PathIntegrator.cpp:121-126 */
    GNXR_MAT_MATTE = 1,    /* MatteMaterial.cpp:14-32   (Lambert / OrenNayar)            */
    GNXR_MAT_MIRROR = 2,   /* MirrorMaterial.cpp:13-24                                   */
    GNXR_MAT_GLASS = 3,    /* GlassMaterial.cpp:14-61                                    */
    GNXR_MAT_METAL = 4,    /* MetalMaterial.cpp:28-49                                    */
    GNXR_MAT_PLASTIC = 5,  /* PlasticMaterial.cpp:15-41                                  */
    GNXR_MAT_DISNEY = 6    /* DisneyMaterial.cpp:467-581 (BSSRDF branch out of scope)    */
} gnxr_material_type;

/* Textures are ConstantTexture (textures/ConstantTexture.h:13-23) except Kd / Ks of MATTE and
 * PLASTIC, which may be an ImageTexture (kd_texture / ks_texture below; the reference's
 * getSmileFacePlasticMaterial, ui/MaterialList.cpp:31-46), so a material is a POD of
 * constants plus two texture references.  Field use per type:
 *   MATTE  : kd, sigma (degrees)
 *   MIRROR : kr
 *   GLASS  : kr, kt, eta[0] (index), urough, vrough, remap_roughness
 *   METAL  : eta (rgb), k (rgb), urough, vrough, remap_roughness
 *   PLASTIC: kd, ks, urough (roughness), remap_roughness
 *   DISNEY : kd (color), eta[0], and the disney_* block (DisneyMaterial.h:21-36)
 * bump: every reference material carries a non-null ConstantTexture<float>(0) bump map
 * (ui/RenderThread.cpp:90, ui/MaterialList.cpp:44,54,67,80) so Material::Bump
 * (core/Material.cpp:16-52) runs on every hit; has_bump=1 reproduces that.            */
typedef struct gnxr_material {
    int32_t type;
    int32_t has_bump;
    int32_t remap_roughness;
    int32_t disney_thin;
    float kd[3];
    float ks[3];
    float kr[3];
    float kt[3];
    float eta[3];
    float k[3];
    float sigma;
    float urough;
    float vrough;
    float disney_metallic;
    float disney_spec_trans;
    float disney_spec_tint;
    float disney_sheen;
    float disney_sheen_tint;
    float disney_clearcoat;
    float disney_clearcoat_gloss;
    float disney_anisotropic;
    float disney_roughness;
    float disney_flatness;
    float disney_diff_trans;
    float disney_scatter_distance[3];
    int32_t kd_texture;     /* 1 + index into desc.textures, 0 == the constant kd (MATTE, PLASTIC) */
    int32_t ks_texture;     /* 1 + index into desc.textures, 0 == the constant ks (PLASTIC)        */
} gnxr_material;

/* ---- ImageTexture<RGBSpectrum, Spectrum> + UVMapping2D + MIPMap: textures/ImageTexture.{h,cpp},
 * core/Texture.cpp:163-175, core/MIPMap.h.  The texels cross the boundary decoded (what stbi_loadf
 * returns in ImageTexture.cpp:12-38: row 0 is the TOP row; the library applies the y flip of :79-85,
 * convertIn's scale / inverse gamma, the Lanczos resample to powers of two and the pyramid).  Triangles
 * carry no per-vertex uv anywhere in the reference (ui/ModelList.cpp passes nullptr), so uv is the default
 * (0,0),(1,0),(1,1) of Triangle::GetUVs (shape/Triangle.h:60-74).  Filtering needs the camera ray
 * differentials (camera/Perspective.cpp:86-106, SurfaceInteraction::ComputeDifferentials). ---------- */
typedef enum gnxr_image_wrap { GNXR_WRAP_REPEAT = 0, GNXR_WRAP_BLACK = 1, GNXR_WRAP_CLAMP = 2 } gnxr_image_wrap; /* enum class ImageWrap, core/MIPMap.h:18 */
typedef struct gnxr_texture {
    int32_t width, height;
    int64_t texel_offset;   /* first float of this texture in desc.texels (RGB fp32, width*height*3)  */
    float su, sv, du, dv;   /* UVMapping2D(su, sv, du, dv)                                          */
    float max_aniso;        /* MIPMap::maxAnisotropy (EWA)                                          */
    float scale;            /* convertIn scale                                                      */
    int32_t trilinear;      /* doTrilinear: 0 == EWA                                                */
    int32_t wrap;           /* gnxr_image_wrap                                                      */
    int32_t gamma;          /* convertIn: InverseGammaCorrect                                       */
    int32_t _pad;
} gnxr_texture;

/* ---- lights: lights/{DiffuseAreaLight,InfiniteAreaLight,SkyBoxLight}.cpp ---------- */
typedef enum gnxr_light_type {
    GNXR_LIGHT_AREA_TRI = 1, /* one DiffuseAreaLight per emissive triangle, ModelList.cpp:140-146 */
    GNXR_LIGHT_INFINITE = 2, /* InfiniteAreaLight.cpp:12-132, uses desc.env_*                    */
    GNXR_LIGHT_SKYBOX = 3,   /* SkyBoxLight.cpp:43-85 with a failed image load (gradient)        */
    /* delta lights (LightFlags::DeltaPosition / DeltaDirection): EstimateDirect takes its IsDeltaLight branch, core/Integrator.cpp:
     * 157-158, 168.  The reference authors a spot and a distant light (AddSpotLight / AddDistLight, ui/ModelList.cpp:149-161) but
     * leaves the calls commented out (ui/RenderThread.cpp:138-141).                                                            */
    GNXR_LIGHT_POINT = 4,    /* lights/PointLight.cpp: le = I, position = light_to_world * (0,0,0)                              */
    GNXR_LIGHT_SPOT = 5,     /* lights/SpotLight.cpp: le = I, radius = totalWidth (degrees), falloff_start (degrees), axis +z   */
    GNXR_LIGHT_DISTANT = 6   /* lights/DistantLight.cpp: le = L, center = wLight in light space (Normalize(LightToWorld(w)))    */
} gnxr_light_type;

typedef struct gnxr_light {
    int32_t type;
    int32_t tri;        /* AREA_TRI: index into desc triangles (authoring order)          */
    int32_t two_sided;  /* kept for fidelity; has no effect (DiffuseAreaLight.h:24 quirk) */
    int32_t n_samples;  /* Light::nSamples (core/Light.cpp:19: max(1, n)); used by UniformSampleAllLights only */
    float le[3];        /* AREA_TRI: Lemit ; INFINITE: power scale L                      */
    float radius;       /* SKYBOX: sphere radius                                          */
    float center[3];    /* SKYBOX: sphere centre ; DISTANT: wLight                        */
    float falloff_start;/* SPOT: falloffStart in degrees (radius carries totalWidth)      */
    float light_to_world[16]; /* INFINITE: row-major 4x4 (LightToWorld, ModelList.cpp:174) */
} gnxr_light;

/* ---- camera: camera/Perspective.cpp:114-135 (fov 90, lens 0 in the reference) ------ */
typedef struct gnxr_camera {
    float eye[3];
    float look[3];
    float up[3];
    float fov_deg;
    float lens_radius;
    float focal_distance;
    int32_t orthographic;   /* 0: PerspectiveCamera (camera/Perspective.cpp) ; 1: OrthographicCamera (camera/Orthographic.cpp:
                               Orthographic(0, 10), screen window x 2 as CreateOrthographicCamera sets it; fov_deg unused) */
} gnxr_camera;

/* ---- media: media/{Homogeneous,GridDensity}Medium.cpp (VolPath, config 5) ---------- */
typedef enum gnxr_medium_type { GNXR_MEDIUM_HOMOGENEOUS = 1, GNXR_MEDIUM_GRID = 2 } gnxr_medium_type;

typedef struct gnxr_medium {
    int32_t type;
    int32_t nx, ny, nz;        /* GRID: density grid resolution                            */
    float sigma_a[3];
    float sigma_s[3];
    float g;
    float _pad;
    float medium_to_world[16]; /* GRID: row-major 4x4                                      */
    int64_t density_offset;    /* GRID: first float of this grid in desc.grid_density      */
} gnxr_medium;

/* ---- sphere: shape/Sphere.{h,cpp} is an unfinished stub in the reference (Intersect returns `discriminant > 0` and
 * fills neither tHit nor the interaction), so the quadratic sphere of pbrt-v3 -- whose file it was started from -- is
 * built instead: full sphere, ObjectToWorld = Translate(center).  Parity with the reference is UNPINNED (nothing to
 * pin against); the device is pinned against the CPU restatement and against analytic hits. ------------------------- */
typedef struct gnxr_sphere {
    float center[3];
    float radius;
    int32_t material;       /* index into materials, -1 == null material          */
    int32_t medium_inside;  /* MediumInterface, -1 == none                        */
    int32_t medium_outside;
    int32_t _pad;
} gnxr_sphere;

/* ---- scene description: what ModelList.cpp / RenderThread.cpp author --------------- */
typedef struct gnxr_scene_desc {
    int32_t abi_version;        /* GNXR_ABI_VERSION */
    int32_t n_vertices;
    int32_t n_triangles;
    int32_t n_materials;
    int32_t n_lights;
    int32_t n_media;
    int32_t env_width;          /* INFINITE light: lat-long radiance map (RGB fp32), 0 if none */
    int32_t env_height;
    const float *vertices;      /* n_vertices * 3, WORLD space (TriangleMesh ctor, Triangle.cpp:27-31) */
    const int32_t *indices;     /* n_triangles * 3; triangle order == reference prims order  */
    const int32_t *tri_material;/* n_triangles; index into materials, -1 == null material    */
    const int32_t *tri_light;   /* n_triangles; index into lights (AREA_TRI) or -1           */
    const int32_t *tri_medium_inside;  /* n_triangles or NULL; -1 == none (MediumInterface)  */
    const int32_t *tri_medium_outside; /* n_triangles or NULL                                */
    const gnxr_material *materials;
    const gnxr_light *lights;   /* order == scene.lights order (light selection index)       */
    const gnxr_medium *media;
    const float *grid_density;
    const float *env_rgb;       /* env_width*env_height*3, row-major, as decoded from .hdr   */
    gnxr_camera camera;
    int32_t camera_medium;      /* medium the camera sits in, -1 == none                     */
    int32_t n_spheres;
    const gnxr_sphere *spheres; /* tested before the triangle BVH; gnxr_hit.prim = n_triangles + sphere index */
    int32_t n_textures;
    int32_t _pad;
    const gnxr_texture *textures;
    const float *texels;
    const float *tri_uv;        /* n_triangles * 6 or NULL: (u,v) of each triangle's three corners = TriangleMesh::uv looked up through
                                   the vertex indices (Triangle::GetUVs, shape/Triangle.h:60-74); NULL == the defaults (0,0),(1,0),(1,1)
                                   every mesh of the reference gets (ui/ModelList.cpp passes uv = nullptr)                     */
    const float *tri_n;         /* n_triangles * 9 or NULL: WORLD-space shading normals of each triangle's three corners = TriangleMesh::n
                                   looked up through the vertex indices (shape/Triangle.cpp:228-297: interpolated shading normal,
                                   shading frame, dndu / dndv, geometric normal flipped onto its side); three zero vectors == the
                                   triangle has no normals.  Not allowed on emissive triangles.                                */
    const float *tri_s;         /* n_triangles * 9 or NULL: WORLD-space shading tangents of the corners = TriangleMesh::s (the `ss`
                                   of Triangle.cpp:242-250); three zero vectors == none.  Not allowed on emissive triangles.   */
    int32_t bvh_split_method;   /* gnxr_bvh_split_method: how BVHAccel(prims, 1, splitMethod) builds the tree */
    int32_t _pad2;
} gnxr_scene_desc;

/* enum class SplitMethod, accelerator/BVHAccel.h:24 (same order).  The reference builds BVHAccel(prims, 1) = SAH. */
typedef enum gnxr_bvh_split_method {
    GNXR_BVH_SAH = 0,    /* recursiveBuild with the surface-area heuristic, BVHAccel.cpp:191-367 (host)                          */
    GNXR_BVH_HLBVH = 1,  /* HLBVHBuild, BVHAccel.cpp:369-626: Morton codes + radix sort on the device, LBVH treelets and the SAH
                            upper tree over at most 4096 treelets on the host                                                   */
    GNXR_BVH_MIDDLE = 2, /* recursiveBuild, split at the midpoint of the centroid bounds, BVHAccel.cpp:243-258 (host)            */
    GNXR_BVH_EQUAL_COUNTS = 3 /* recursiveBuild, nth_element at the median, BVHAccel.cpp:259-268 (host)                          */
} gnxr_bvh_split_method;

typedef enum gnxr_integrator {
    GNXR_INTEGRATOR_PATH = 0,    /* integrators/PathIntegrator.cpp:62-208   */
    GNXR_INTEGRATOR_VOLPATH = 1, /* integrators/VolPathIntegrator.cpp:24-159 */
    GNXR_INTEGRATOR_WHITTED = 2, /* integrators/WhittedIntegrator.cpp:14-68 */
    GNXR_INTEGRATOR_DIRECT = 3   /* integrators/DirectLightingIntegrator.cpp:11-67 */
} gnxr_integrator;

/* enum class LightStrategy, integrators/DirectLightingIntegrator.h:13 (same order) */
typedef enum gnxr_direct_strategy {
    GNXR_DIRECT_SAMPLE_ALL = 0, /* UniformSampleAllLights, core/Integrator.cpp:25-55: nSamples array samples per light */
    GNXR_DIRECT_SAMPLE_ONE = 1  /* UniformSampleOneLight without a distribution, core/Integrator.cpp:57-79          */
} gnxr_direct_strategy;

typedef enum gnxr_light_strategy {
    GNXR_LIGHTS_SPATIAL = 0, /* core/LightDistribution.cpp:70-274 */
    GNXR_LIGHTS_UNIFORM = 1,
    GNXR_LIGHTS_POWER = 2
} gnxr_light_strategy;

/* Render parameters.  A render covers samples [spp_begin, spp_end) of a HaltonSampler(spp)
 * (samplers/HaltonSampler.cpp:33-60) for the image rows this shard owns:
 * row y belongs to the shard iff (y / shard_rows) % shard_count == shard_index.
 * shard_count=1 renders the whole image.                                                  */
typedef struct gnxr_render_params {
    int32_t width, height;
    int32_t spp;                /* HaltonSampler samplesPerPixel; divisor of the box average */
    int32_t spp_begin, spp_end; /* sample range rendered by this call; 0,spp == all          */
    int32_t max_depth;          /* PathIntegrator maxDepth                                   */
    float rr_threshold;         /* PathIntegrator rrThreshold                                */
    int32_t integrator;         /* gnxr_integrator                                           */
    int32_t light_strategy;     /* gnxr_light_strategy                                       */
    int32_t shard_index, shard_count, shard_rows;
    int32_t samples_per_pass;   /* 0 = auto; samples of one pixel rendered per (sub-)pass.  The image does not depend on it */
    int32_t direct_strategy;    /* gnxr_direct_strategy (GNXR_INTEGRATOR_DIRECT only)        */
    int32_t passes_in_flight;   /* GNXR_INTEGRATOR_PATH: sub-passes alive at once, each in its own region of the path state
                                   (resident state = passes_in_flight x samples_per_pass samples per pixel); staggered in time,
                                   so that a launch mixes the first bounces of one sub-pass with the thin late bounces of the
                                   others.  0 = auto (4, fewer if the call is short or memory is tight), at most 8.  The image
                                   does not depend on it.  Reference loop: core/Integrator.cpp:256-293 */
} gnxr_render_params;

typedef struct gnxr_stats {
    uint64_t rays_closest;      /* Scene::Intersect calls  (core/Scene.cpp:11-17)            */
    uint64_t rays_any;          /* Scene::IntersectP calls (core/Scene.cpp:19-24)            */
    uint64_t camera_samples;
    uint64_t nodes_visited;     /* filled only when GNXR_STATS_TRAVERSAL is requested        */
    uint64_t tris_tested;
    double seconds_render;      /* kernel pipeline, excludes scene build/upload              */
    double seconds_trace;       /* sum of HIP-event time of the traversal kernels            */
    double seconds_total;
    uint32_t kernel_launches;
    uint32_t passes;
    double seconds_closest;     /* k_closest launches (profiling bit 0)                      */
    double seconds_nee;         /* k_nee launches                                            */
    double seconds_shade;       /* k_shade launches                                          */
    uint32_t launches_closest, launches_nee;
    uint64_t rays_closest_nee;  /* closest-hit rays traced by k_nee (MIS rays)               */
    uint64_t media_segments;    /* VolPath: ray segments handed to the tracking kernel (Medium::Sample / Medium::Tr calls on rays inside a medium) */
    uint64_t media_steps;       /* VolPath: tracking-loop iterations of those segments (filled by the counting run, profiling bit 2) */
    uint64_t leaf_retests;      /* counting run, bit 2: leaf boxes re-tested against a shrunken tMax by the 4-wide walk (32 B each)  */
    uint64_t nodes_from_memory; /* counting run, bit 2: 4-wide node visits that read global memory (the rest hit the kernel's LDS copy of the top of the tree) */
    uint32_t passes_in_flight;  /* sub-passes the path loop kept alive at once (1 for the other integrators)                          */
    uint32_t loop_iterations;   /* iterations of the path loop (one trace + one shade stage each)                                     */
    uint64_t state_bytes;       /* path state resident on the device for this render (per-path arrays and queues)                      */
} gnxr_stats;

typedef struct gnxr_ray { float o[3]; float tmax; float d[3]; float _pad; } gnxr_ray;
typedef struct gnxr_hit {
    int32_t prim;               /* triangle index (authoring order) or -1                    */
    float t, b0, b1, b2;
    float n[3];                 /* geometric normal as set by Triangle::Intersect            */
} gnxr_hit;
/* The sample a caller ray of gnxr_li_device stands for: pixel (px, py) and sample s of the render's HaltonSampler, and the medium
 * the ray starts in (-1: none).  16 bytes.                                                                                        */
typedef struct gnxr_li_sample { int32_t px, py, s, medium; } gnxr_li_sample;
/* One query of gnxr_bsdf_device: BSDF::f / Pdf towards `wi`, BSDF::Sample_f with `u`, at the hit of a ray.  64 bytes.          */
typedef struct gnxr_bsdf_result {
    float f[3];                 /* BSDF::f(wo, wi, flags)                                    */
    float pdf;                  /* BSDF::Pdf(wo, wi, flags)                                  */
    float sample_f[3];          /* BSDF::Sample_f(wo, &sample_wi, u, &sample_pdf, flags, &sampled_type); 0 when sample_pdf == 0 */
    float sample_pdf;
    float sample_wi[3];         /* world space; 0 when sample_pdf == 0                       */
    int32_t sampled_type;       /* BxDFType of the sampled lobe                              */
    int32_t n_components;       /* BSDF::NumComponents(flags)                                */
    int32_t valid;              /* 1: the ray hit a surface that has a BSDF; 0 (and the whole record 0): miss or null material */
    float dudx, dvdy;           /* SurfaceInteraction::dudx / dvdy (0 without ray differentials) */
} gnxr_bsdf_result;
/* One query of gnxr_light_sample_device.  48 bytes.                                                                              */
typedef struct gnxr_light_result {
    float Li[3];                /* Light::Sample_Li(ref, u, &wi, &pdf, &vis)                 */
    float pdf;
    float wi[3];
    float pdf_li;               /* Light::Pdf_Li(ref, wi_query)                              */
    float pdf_select;           /* LightDistribution::Lookup(p)->DiscretePDF(light)          */
    float p_light[3];           /* VisibilityTester::P1().p: the sampled point on the light  */
} gnxr_light_result;

typedef struct gnxr_scene gnxr_scene;

/* -- lifecycle ---------------------------------------------------------------------- */
int gnxr_abi_version(void);
int gnxr_abi_sizeof(int which);        /* sizeof of the structs above in declaration order (binding self-check) */
int gnxr_init(int device_id);          /* binds the calling process to one HIP device    */
/* One process, several devices (`gnxr_init(int n_devices, const int *device_ids)`): scenes created afterwards are
 * replicated on every listed device and gnxr_render / gnxr_render_device deal the image rows round-robin over them, render the
 * shards concurrently (one host thread + stream per device, no exchange during rendering) and assemble the FrameBuffer on
 * device_ids[0] -- one strided peer copy per device where peer access could be enabled both ways (recorded per pair at init), a
 * pinned host buffer otherwise; GNXR_NO_PEER=1 forces the staged route -- what the reference's single `integrator->Render(scene)` call
 * (ui/RenderThread.cpp:175, core/Integrator.h:17-23) needs to use a whole node.  Results are bit-identical to one device's
 * (pixels are independent).  The same id may be listed more than once (two shards sharing a device: how this path is tested on
 * a one-GPU box; on DISTINCT devices the path has not run yet: parity unpinned there, the pool hands out one-GPU boxes only).
 * Batched trace calls and probes run on device_ids[0].  gnxr_init(d) == gnxr_init_devices(1, &d).                              */
int gnxr_init_devices(int32_t n_devices, const int32_t *device_ids);
void gnxr_shutdown(void);
const char *gnxr_last_error(void);
/* Measurement switches (process-wide).  bit 0: bracket every traversal kernel launch with HIP events on
 * the render stream and report their summed duration in gnxr_stats.seconds_trace (+ per-kernel split in
 * seconds_closest / seconds_nee); bit 1: run the counting variant of the traversal kernel on the reference's BINARY
 * tree (BVHAccel::Intersect's own node visits: comparable with the oracle's counts) and fill nodes_visited /
 * tris_tested; bit 2: count on the walk the timed kernel performs instead -- 4-wide nodes visited, speculative visits
 * included -- and the tracking-loop iterations of the medium kernel (media_steps).  Counting runs are slower; never
 * combine them with a timed run.                                                                             */
int gnxr_set_profiling(int flags);
/* Measurement hook: the VALU issue rate of this device, in 1e9 wave64 instructions per second, reached by a kernel of
 * independent v_fma_f32 chains with 8 waves on every SIMD -- the ceiling bench.py prices the traversal kernel's
 * instruction stream against.                                                                                */
int gnxr_probe_valu_peak(double *giga_wave_insts_per_s);
/* Measurement hook: the rate at which this device takes per-lane 16-byte gathers (every lane reads the 8 dwordx4 of its own random
 * 128-byte record of an 8 MB table: the access pattern of a BVH node visit), in 1e9 lane-loads per second.  On MI355X this rate
 * (~690 G/s = 1.1 lanes per clock per CU) is the same for L1-resident and L2-resident tables and at 1 to 8 blocks per CU
 * (tools/probes/gather_probe.hip): it is a ceiling of the vector-memory path, beside HBM bandwidth and VALU issue.              */
int gnxr_probe_gather_peak(double *giga_lane_loads_per_s);

/* -- scene (replaces `Scene(make_shared<BVHAccel>(prims,1), lights)`, RenderThread.cpp:155) */
int gnxr_scene_create(const gnxr_scene_desc *desc, gnxr_scene **out);
void gnxr_scene_destroy(gnxr_scene *scene);
/* Test hook: the flattened binary BVH of the scene's first device (the reference's LinearBVHNode[]: per node 6 floats of bounds
 * into `bounds6`, then offset / nPrimitives / axis into `meta3`) and the primitive order (`ordered`, n_triangles entries);
 * *n_nodes receives the node count, arrays are filled when node_capacity allows. */
int gnxr_scene_bvh(const gnxr_scene *scene, float *bounds6, int32_t *meta3, int32_t *ordered, int64_t node_capacity, int64_t *n_nodes);
/* Test hook: the 4-wide node table of the scene's first device (128 bytes per node into `nodes128`, filled when node_capacity
 * allows; *n_nodes4 receives the node count) and the quantities the traversal plan is sized from: the root reference and the
 * worst-case stack entries (either may be NULL). */
int gnxr_scene_bvh4(const gnxr_scene *scene, void *nodes128, int64_t node_capacity, int64_t *n_nodes4, int32_t *root4, int32_t *stack_need);
int gnxr_scene_info(const gnxr_scene *scene, int32_t *n_bvh_nodes, int32_t *bvh_max_depth,
                    int32_t *n_light_voxels);
/* -- editing a scene between frames (the viewer's `while (renderFlag)` loop, RenderThread.cpp:168-186): no recompilation, and the
 * path state gnxr_render_reserve allocated stays where it is.
 * Move vertices of an existing scene: positions [first_vertex, first_vertex + n_vertices) of the scene's vertex array
 * (the numbering of gnxr_scene_desc.vertices, world space) become xyz[0 .. 3 n_vertices).  xyz may be host memory or
 * device memory of the scene's (first) device; the read is ordered after work already queued on hip_stream (NULL: the null
 * stream), and the refit runs on that stream.  The BVH keeps its topology and primitive order; its boxes are refitted on the
 * device (exactly the LinearBVHNode bounds that topology has over the new vertices).  Returns when every device of the scene
 * holds the new geometry.  Per-corner uvs / shading normals / tangents, spheres, materials and lights are unchanged (a smooth mesh
 * gets normals for its new shape from gnxr_scene_recompute_normals, or rows of the caller's from gnxr_scene_update_attributes); what depends
 * on the world bound (environment and distant lights, the light-selection table) follows it.  GNXR_ERR_UNSUPPORTED (scene
 * untouched) if a vertex of an emissive (AREA_TRI) triangle would change value: area lights move through
 * gnxr_scene_update_vertices_ex with GNXR_UPDATE_MOVE_LIGHTS.  GNXR_ERR_INVALID for a null scene, a null xyz with
 * n_vertices > 0 or a range outside the scene's vertices.  Traversal quality is that of the old topology: after large
 * deformations build the scene again with gnxr_scene_create, or keep the handle and call gnxr_scene_rebuild_bvh. */
int gnxr_scene_update_vertices(gnxr_scene *scene, int32_t first_vertex, int32_t n_vertices, const float *xyz, void *hip_stream);
/* gnxr_scene_update_vertices with flags; flags == 0 is that call exactly.  GNXR_UPDATE_MOVE_LIGHTS: vertices of emissive triangles may
 * move too.  Nothing is refused for them; after the refit a kernel on the same stream rewrites corners, area and normal of EVERY
 * AREA_TRI light record from its triangle (one light per emissive triangle: a moving mesh light is thousands of records), with the
 * arithmetic gnxr_scene_create applies to them, so the records -- and every render, light sample and light-selection table after the
 * call -- are bit for bit those of a scene created from a description carrying the vertices the scene now holds (tree aside: it keeps
 * its topology), and re-sending unchanged vertices changes nothing.  A triangle moved to zero area gets the infinite inv_area and NaN
 * normal gnxr_scene_create gives it; that is not an error.  The records (112 bytes per light) come back to the host with the root box.
 * GNXR_ERR_INVALID, before any device is touched, for unknown flag bits, a null scene, a null xyz with n_vertices > 0 or a range
 * outside the scene's vertices. */
#define GNXR_UPDATE_MOVE_LIGHTS 1u
int gnxr_scene_update_vertices_ex(gnxr_scene *scene, int32_t first_vertex, int32_t n_vertices, const float *xyz, uint32_t flags, void *hip_stream);
/* Replace the parameters of lights [first_light, first_light + n_lights) of the scene's light list (the numbering of
 * gnxr_scene_desc.lights) by lights[0 .. n_lights): afterwards the scene renders, bit for bit, as a scene created from the same
 * description with those light records.  What may change: le, two_sided and n_samples of an AREA_TRI light (its corners, area and
 * normal stay those of the vertices the scene holds now, moved or not); every field of a POINT, SPOT or DISTANT light; center and
 * radius of a SKYBOX light.  GNXR_ERR_UNSUPPORTED for a record whose type differs from the light's, an AREA_TRI record whose tri
 * differs (gnxr_scene_set_lights replaces the list), or an INFINITE record that differs in any byte (the environment light changes through gnxr_scene_update_environment,
 * which rebuilds its tables);
 * GNXR_ERR_INVALID for a null scene, a null lights with n_lights > 0 or a range outside the scene's lights.  Every refusal leaves the
 * scene exactly as it was: all records are built into a copy first.  The call takes the handle's render lock, writes the records of
 * every device of the scene and returns; the BVH, textures, tables and the path state of gnxr_render_reserve stay, the light-selection
 * table is rebuilt at the next render. */
int gnxr_scene_update_lights(gnxr_scene *scene, int32_t first_light, int32_t n_lights, const gnxr_light *lights);
/* Replace the scene's light list by lights[0 .. n_lights) (host memory): lights may be added, removed and retyped, and which triangles
 * are emissive may change.  n_lights == 0 is allowed (lights may then be NULL).  Afterwards every result of the handle -- renders of all
 * integrators, the ray counters, gnxr_li_device, gnxr_light_sample_device, gnxr_light_le_device, the feature buffers, the light-selection
 * tables of all three strategies -- is bit for bit that of a scene created from the same description with this light list and the
 * tri_light array that matches it.  Kept: the tree, materials, textures, media, the environment tables, the camera and the path state of
 * gnxr_render_reserve.
 * AREA_TRI: tri is a triangle of the mesh the scene holds now, in authoring order, [0, n_triangles); no two lights may name the same one.
 * le, two_sided and n_samples come from the record; corners, area and normal from the vertices the scene holds now, computed on the
 * device as gnxr_scene_update_vertices_ex computes them.  Triangles no light names stop being emissive.  A triangle with per-vertex
 * normals or tangents cannot be emissive, as at creation.  POINT / SPOT / DISTANT / SKYBOX records are compiled against the current world
 * bound, as gnxr_scene_update_lights compiles them.  INFINITE: its tables are not rebuilt here, so the new list must hold exactly as many
 * INFINITE records as the scene has (0 or 1), byte-identical to the current one; its index may move, but whether a SKYBOX record precedes
 * it may not (that decides the row order of its texels).  Anything else is GNXR_ERR_UNSUPPORTED: gnxr_scene_update_environment changes
 * that light.
 * GNXR_ERR_INVALID: a null scene, n_lights < 0, a null lights with n_lights > 0 (all before any device is touched); an unknown type; tri
 * out of range or named twice; normals or tangents on a triangle made emissive.  GNXR_ERR_OOM.  Every record is checked before anything is
 * written, and a call that fails later puts DTri::light -- the one table written in place -- back on every device: a refused or failed
 * call leaves the scene as it was.  Limits that depend on an integrator (DirectLighting's and Whitted's 256 samples per vertex, the
 * spatial table's memory) are checked by the render that meets them, as for a created scene.
 * The AREA_TRI records are bound to their triangles on the device, on hip_stream (NULL: the null stream), in whatever leaf order the tree
 * has: no tree or triangle table crosses to the host.  The call takes the handle's render lock and returns when every device of the scene
 * holds the new list; the light-selection table is rebuilt at the next render.  To change the mesh and its emissive triangles together:
 * gnxr_scene_set_lights with the non-area lights only, gnxr_scene_set_geometry with tri_light NULL or all -1, gnxr_scene_set_lights with
 * the full list on the new triangles (three calls, not atomic: renders in between see fewer lights). */
int gnxr_scene_set_lights(gnxr_scene *scene, const gnxr_light *lights, int32_t n_lights, void *hip_stream);
/* Test hook: what the first device holds.  which 0: the light records, 112 bytes (28 words) each, n_lights of them; which 1: per triangle
 * in authoring order the light it is (int32, -1: none).  *n_bytes receives the size; the table is copied when out is not NULL and
 * capacity_bytes suffices. */
int gnxr_scene_light_tables(gnxr_scene *scene, int32_t which, void *out, int64_t capacity_bytes, int64_t *n_bytes);
/* Replace or rotate the environment map of the scene's INFINITE light.  `light` is the new record of that light: le, light_to_world and
 * n_samples may change, type must be GNXR_LIGHT_INFINITE.  rgb is the new map, width * height * 3 fp32, row-major, as decoded from .hdr
 * (the meaning of gnxr_scene_desc.env_rgb); its size may differ from the one the scene was created with.  rgb may be host memory or
 * device memory of the scene's (first) device, told apart as gnxr_scene_update_vertices tells xyz apart; the read is ordered after what
 * hip_stream holds (NULL: the null stream) and the build runs on that stream.  The texels (r * sqrt(r), r = le * rgb, rows flipped when a
 * SKYBOX light precedes the INFINITE light in the light list, as at creation), their Lanczos resample to powers of two, the pyramid behind
 * InfiniteAreaLight::Power, the 2w x 2h sampling image, its conditional and marginal distributions and the FindInterval guide tables are
 * built on the device, on every device of the scene from the raw map, with the arithmetic gnxr_scene_create applies on the host:
 * afterwards every result of the handle -- renders of all integrators, gnxr_li_device, gnxr_render_views_device, gnxr_render_aov_device,
 * gnxr_light_sample_device, gnxr_light_le_device, the light-selection tables of all three strategies, the ray counters of gnxr_stats -- is
 * bit for bit that of a scene created from the same description carrying this map and this record.
 * rgb == NULL (width and height ignored) is a rotation-only edit: le must equal the current record's bytes, only the transforms, the
 * light record and the light-selection table change and no kernel runs; with a changed le it is GNXR_ERR_INVALID -- send the map again,
 * the raw map is not retained.
 * The call takes the handle's render lock.  Each device builds into fresh buffers and no copy swaps until every copy has built, so a
 * refused or failed call leaves the scene exactly as it was, on all devices.  It returns when every device holds the new tables.  The
 * light-selection table is rebuilt at the next render; the BVH, materials, textures, media, sampler tables, the camera and the path state
 * of gnxr_render_reserve stay where they are.  Besides the map, the Lanczos weights (one record per resampled row and column) and the
 * light records go to the device; the at most 21 texels of the pyramid's top three levels and the marginal's integral come back; no table
 * crosses the host when rgb is device memory.
 * GNXR_ERR_INVALID, before any device is touched, for a null scene, a null light, a type other than GNXR_LIGHT_INFINITE, rgb with
 * width <= 0 or height <= 0, a size whose guide-table entries would not fit uint16_t (2 * round_up_pow2(size) + 1 > 65535: more than
 * 16384 texels per side) and the le rule above; GNXR_ERR_UNSUPPORTED for a scene without an INFINITE light (neither this call nor
 * gnxr_scene_set_lights adds one); GNXR_ERR_OOM. */
int gnxr_scene_update_environment(gnxr_scene *scene, const gnxr_light *light, const float *rgb, int32_t width, int32_t height, void *hip_stream);
/* Rebuild the triangle BVH of an existing scene over the vertices it currently holds on the device (the state after any number of
 * gnxr_scene_update_vertices calls), entirely on the device: the tree, its 4-wide form, the primitive order and everything kept in
 * that order become what gnxr_scene_create builds with bvh_split_method = GNXR_BVH_HLBVH from a description carrying those vertices,
 * whatever split method the scene was created with.  Materials, textures, environment tables, media, spheres, sampler tables, the
 * camera and the path state of gnxr_render_reserve stay where they are; the world bound is the one the refits left; the
 * light-selection table is rebuilt at the next render.  The work is ordered after what hip_stream holds (NULL: the null stream), the
 * call takes the handle's render lock and returns when every device of the scene holds the new tree.  Besides counts and flags only
 * the light records (their triangle references follow the new order) cross to the host; no node or triangle table does.  Every failure leaves the scene exactly as it was: GNXR_ERR_INVALID for a null scene or an input on which the
 * reference's HLBVH build does not terminate (coincident treelet centroids, a leaf over 65535 primitives), GNXR_ERR_UNSUPPORTED for a
 * tree deeper than the 64-entry traversal stack, GNXR_ERR_OOM. */
int gnxr_scene_rebuild_bvh(gnxr_scene *scene, void *hip_stream);
/* Replace the triangle mesh of an existing scene: vertex count, triangle count, index array and every per-triangle array may change.  The
 * fields mean what the fields of the same names mean in gnxr_scene_desc.  The arrays are either ALL host memory or ALL device memory of
 * the scene's first device (a mix, or another device: GNXR_ERR_INVALID); they are read on hip_stream (NULL: the null stream), ordered
 * after what the caller queued there, and the call returns -- it synchronises, as gnxr_scene_rebuild_bvh does -- once every device of
 * the scene has been switched over.  struct_size must be sizeof(gnxr_geometry) (the record is not part of gnxr_abi_sizeof's list).
 *
 * After a successful call every observable result -- renders of all integrators, the ray queries, gnxr_li_device, the shading queries,
 * gnxr_render_views_device, gnxr_render_aov_device, gnxr_scene_bvh, gnxr_scene_bvh4, gnxr_scene_info, the light-selection tables -- is
 * bit for bit that of a scene created with gnxr_scene_create from the same description with the geometry fields replaced by *g,
 * gnxr_light::tri taken from tri_light and bvh_split_method = GNXR_BVH_HLBVH (binary bounds up to the sign of a zero).  Kept: materials,
 * textures, environment tables, media, spheres, camera, sampler tables, the path state of gnxr_render_reserve, and the light list's
 * length, types and parameters.  What follows the new mesh: primitive ids (gnxr_hit.prim, the ids feature buffer, a sphere's
 * n_triangles + index), the world bound and with it the environment light's bounding sphere and the distant lights' radius, the
 * light-selection table (rebuilt at the next render), the traversal stack and the choice of the traversal kernel.  Later edits
 * (gnxr_scene_update_vertices[_ex], gnxr_scene_rebuild_bvh, gnxr_scene_set_triangle_materials, gnxr_scene_update_materials,
 * gnxr_scene_update_lights) work on the new mesh.
 *
 * Lights: tri_light must name every AREA_TRI light of the scene on exactly one triangle and no other light; the records' corners, area,
 * normal and triangle reference are recomputed on the device, le / two_sided / n_samples stay.  Normals or tangents on an emissive
 * triangle are refused, as at creation.
 *
 * One pass over the triangles on the device validates the arrays and builds the scene's tables in authoring order (an index out of range
 * is reported, never dereferenced); the tree is then built by the stages of gnxr_scene_rebuild_bvh.  Of the mesh only tri_material and
 * one byte per triangle (has uvs, normals or tangents of its own) cross to the host, where the material tables are compiled; vertex and
 * index data stay on the first device (further devices of gnxr_init_devices are fed through the host).
 *
 * Every refusal is found before anything of the scene changes.  GNXR_ERR_INVALID: a null scene or record or a wrong struct_size (before
 * any device is touched); n_vertices < 1 or n_triangles < 1; a null vertices / indices / tri_material, a null tri_light in a scene with
 * AREA_TRI lights; only one of the two medium arrays; arrays on mixed sides or on another device; an index outside [0, n_vertices); a
 * material outside [-1, n_materials); a medium outside [-1, n_media); a tri_light entry that is neither -1 nor an AREA_TRI light, a
 * light named twice or not at all; what gnxr_scene_update_materials refuses; non-finite centroids or more than 65535 primitives on one
 * Morton code.  GNXR_ERR_UNSUPPORTED: a tree deeper than the 64-entry traversal stack.  GNXR_ERR_OOM. */
typedef struct gnxr_geometry {
    int32_t struct_size;               /* sizeof(gnxr_geometry): the binding's self-check */
    int32_t n_vertices, n_triangles;
    int32_t _pad;
    const float   *vertices;           /* n_vertices * 3, world space                         */
    const int32_t *indices;            /* n_triangles * 3                                     */
    const int32_t *tri_material;       /* n_triangles, -1 == null material                    */
    const int32_t *tri_light;          /* n_triangles or NULL (allowed only if no AREA_TRI light) */
    const int32_t *tri_medium_inside;  /* n_triangles or NULL; both or neither                */
    const int32_t *tri_medium_outside;
    const float   *tri_uv;             /* n_triangles * 6 or NULL                             */
    const float   *tri_n;              /* n_triangles * 9 or NULL                             */
    const float   *tri_s;              /* n_triangles * 9 or NULL                             */
} gnxr_geometry;
int gnxr_scene_set_geometry(gnxr_scene *scene, const gnxr_geometry *g, void *hip_stream);
/* Replace material records [first_material, first_material + n_materials) of the scene's material list (the numbering of
 * gnxr_scene_desc.materials) by materials[0 .. n_materials).  Every field may change, the type included: MATTE -> GLASS changes which shade
 * kernels the next render launches, a BSDF material -> GNXR_MAT_NONE turns its triangles (and spheres) into medium boundaries, and back;
 * kd_texture / ks_texture may name any texture the scene was created with.  The number of materials and the number of textures are fixed.
 * Afterwards every result of the handle -- renders of all integrators, gnxr_li_device, gnxr_render_views_device, gnxr_render_aov_device,
 * gnxr_bsdf_device, the ray queries, the ray counters of gnxr_stats -- is bit for bit that of a scene created from the same description
 * carrying the edited records (tree aside: it keeps its topology).  The records are validated as gnxr_scene_create validates them
 * (unknown type, texture reference beyond n_textures, image textures on other than MATTE / PLASTIC or on a sphere's material) and
 * compiled into a copy first: GNXR_ERR_INVALID leaves the scene exactly as it was, also for a null scene (before any device is touched),
 * a null materials with n_materials > 0 or a range outside the scene's materials.  n_materials == 0 is a no-op.  The call takes the
 * handle's render lock, writes every device of the scene -- the material tables, then one kernel over the triangles, which hold their
 * material's internal index and shade class -- and returns when all hold the edit; a failed upload puts the old state back on the devices
 * already written.  The BVH, lights, light-selection table, textures, media and the path state of gnxr_render_reserve are not touched. */
int gnxr_scene_update_materials(gnxr_scene *scene, int32_t first_material, int32_t n_materials, const gnxr_material *materials);
/* Replace tri_material[first_triangle, first_triangle + n_triangles) (triangles in authoring order, the numbering of
 * gnxr_scene_desc.tri_material) by material[0 .. n_triangles): values in [-1, n_materials), -1 == no material.  material may be host
 * memory or device memory of the scene's (first) device; the read is ordered after what hip_stream holds (NULL: the null stream) and the
 * kernel runs on that stream.  The ids cross to the host (4 bytes per edited triangle) and are validated there before anything is
 * written.  Emissive triangles may change material.  Contract, error codes, locking and what stays untouched are those of
 * gnxr_scene_update_materials; GNXR_ERR_INVALID also for an id out of range. */
int gnxr_scene_set_triangle_materials(gnxr_scene *scene, int32_t first_triangle, int32_t n_triangles, const int32_t *material, void *hip_stream);
/* Test hook: per triangle in authoring order, read from the scene's first device, the authored material index the triangle currently
 * shows (-1 where it has no BSDF) and its shade-class byte.  Returns the number of triangles (or a negative gnxr_status); the arrays are
 * filled when both are given and capacity allows. */
int gnxr_scene_triangle_materials(gnxr_scene *scene, int32_t *material_out, uint8_t *shade_class_out, int64_t capacity);
/* Test hook: one environment table as the scene's first device holds it.  which 0 .. 7: env_texels4 (float4 per level-0 texel),
 * env_cond_func, env_cond_cdf, env_cond_int, env_marg_func, env_marg_cdf (fp32), env_marg_guide, env_cond_guide (uint16_t); 8: the DEnv
 * record every render is given (sizes, transforms, bounding sphere, the marginal's integral); 9: the three floats of the Power lookup.
 * *n_bytes receives the table's size (0 for a scene without an INFINITE light); out is filled when given and capacity_bytes allows. */
int gnxr_scene_env_tables(gnxr_scene *scene, int32_t which, void *out, int64_t capacity_bytes, int64_t *n_bytes);
/* Replace medium records [first_medium, first_medium + n_media) of the scene's medium list (the numbering of gnxr_scene_desc.media) by
 * media[0 .. n_media).  Every field may change: sigma_a, sigma_s, g, medium_to_world, the grid resolution and the type (HOMOGENEOUS <->
 * GRID).  The number of media and the medium interfaces of triangles and spheres are fixed.  density is the source of the new grids:
 * each GRID record's density_offset indexes into it (the meaning of gnxr_scene_desc.grid_density, local to this call; fp32, x fastest;
 * ranges of two records may overlap or coincide).  density may be host memory or device memory of the scene's (first) device, told apart
 * as gnxr_scene_update_vertices tells xyz apart; the read is ordered after what hip_stream holds (NULL: the null stream) and the kernel
 * runs on that stream.  Each new grid is copied into a fresh packed grid buffer by one kernel that finds its maximum -- the fold from +0
 * of GridDensityMedium.h:28-31, which skips NaNs and never yields -0 -- in the same pass; grids of media the call leaves alone are copied
 * device to device.  Afterwards every result of the handle -- renders of all integrators, gnxr_li_device, gnxr_render_views_device,
 * gnxr_render_aov_device, the queries, the ray counters and media_segments of gnxr_stats -- is bit for bit that of a scene created from
 * the same description carrying these media and grids (tree aside).
 * density == NULL is a coefficients-only edit: every GRID record of the call must name a medium that is GRID now, with the same nx, ny,
 * nz; its grid and its maximum stay, its density_offset is ignored and no kernel runs.
 * The call takes the handle's render lock.  Records are validated and compiled into a copy first, each device builds into a fresh buffer
 * and no copy swaps until every copy has built, so a refused or failed call leaves the scene exactly as it was, on all devices.  It
 * returns when every device holds the edit.  The BVH, materials, lights, the light-selection table, textures, environment tables, sampler
 * tables, the camera (its medium index included) and the path state of gnxr_render_reserve stay where they are.  Besides the grids the
 * medium records go to the device; one float per new grid (its maximum) comes back; no grid crosses the host when density is device
 * memory.
 * GNXR_ERR_INVALID, before any device is touched, for a null scene, a null media with n_media > 0, a range outside the scene's media, an
 * unknown type, nx, ny or nz <= 0 on a GRID record, a density_offset that is negative or 2^60 or more with density != NULL, the density == NULL rule above,
 * grids whose packed total (every grid starts 16-byte aligned) would reach 2^31 floats, and a density in device memory of a device other
 * than the scene's first; GNXR_ERR_UNSUPPORTED for a scene created without media (the medium list is fixed); GNXR_ERR_OOM.  n_media == 0
 * is a no-op. */
int gnxr_scene_update_media(gnxr_scene *scene, int32_t first_medium, int32_t n_media, const gnxr_medium *media, const float *density, void *hip_stream);
/* Test hook, read from the scene's first device.  which 0: the device's medium records of all media (`medium` ignored; 32 words per
 * medium: type, nx, ny, nz, sigma_a, g, sigma_s, sigma_t, the world-to-medium matrix, 1 / the grid's maximum, then density_offset --
 * written as 0: where a grid sits in the library's buffer is layout, not result -- and padding); which 1: the nx * ny * nz floats of
 * grid `medium`, read through its record's offset (size 0 for a HOMOGENEOUS medium).  *n_bytes receives the size; out is filled when
 * given and capacity_bytes allows.  GNXR_ERR_INVALID for null arguments, which outside {0, 1} or, with which 1, a medium outside the list. */
int gnxr_scene_media_tables(gnxr_scene *scene, int32_t which, int32_t medium, void *out, int64_t capacity_bytes, int64_t *n_bytes);
/* Replace texture records [first_texture, first_texture + n_textures) of the scene's texture list (the numbering of
 * gnxr_scene_desc.textures) by textures[0 .. n_textures).  Every field may change: width, height, the mapping (su, sv, du, dv),
 * max_aniso, scale, trilinear, wrap, gamma -- and with them the padded size and the number of MIP levels.  The number of textures is
 * fixed, and so is which material references which texture (gnxr_scene_update_materials changes that).  texels is the source: each
 * record's texel_offset indexes into it (the meaning of gnxr_scene_desc.texels, local to this call: RGB fp32, width * height * 3, row 0
 * the TOP row; ranges of two records may overlap or coincide).  texels may be host memory or device memory of the scene's (first)
 * device, told apart as gnxr_scene_update_media tells density apart; the read is ordered after what hip_stream holds (NULL: the null
 * stream) and the kernels run on that stream.  The pyramid is built on the device as gnxr_scene_create builds it on the host -- y flip,
 * convertIn (scale, inverse gamma), the Lanczos resample to powers of two under the wrap mode, the clamp, the box-filtered levels through
 * MIPMap::Texel -- into a fresh packed texel buffer (textures in index order, levels 0 .. n - 1 of each in order, no padding); textures
 * the call leaves alone are copied device to device.  Afterwards every result of the handle -- renders of all integrators,
 * gnxr_li_device, gnxr_render_views_device, gnxr_render_aov_device, gnxr_bsdf_device with and without differentials, the ray counters of
 * gnxr_stats -- is bit for bit that of a scene created from the same description carrying these records and texels (tree aside), and
 * the device's texture records and texels are byte for byte that scene's.  Texels are finite: NaN and infinite values are outside what
 * is pinned.
 * texels == NULL is a parameters-only edit: su, sv, du, dv, max_aniso and trilinear may change; width, height, wrap, gamma and scale are
 * baked into the texels and must equal the texture's current values (GNXR_ERR_INVALID otherwise: send the texels); texel_offset is
 * ignored, no kernel runs and only the texture records are written.
 * The call takes the handle's render lock.  Records are validated and compiled into a copy first, each device builds into a fresh buffer
 * and no copy swaps until every copy has built; the texture records and the address of the new buffer are written last and the old ones
 * put back if that fails, so a refused or failed call leaves the scene exactly as it was, on all devices.  It returns when every device
 * holds the edit.  The EWA weight table, the BVH, the materials and their shade classes, lights, the light-selection table, media,
 * environment tables, sampler tables, the camera and the path state of gnxr_render_reserve stay where they are.  Besides the texels the
 * Lanczos weights of a resampled texture and the texture records go to the device; nothing comes back, and no texel crosses the host
 * when texels is device memory.
 * GNXR_ERR_INVALID, before any device is touched, for a null scene, a null textures with n_textures > 0, a range outside the scene's
 * textures, width or height <= 0, an unknown wrap, more than 16 MIP levels (a side above 32768), a texel_offset that is negative or 2^60
 * or more with texels != NULL, the texels == NULL rule above, a packed total of 2^31 texels or more, and texels in device memory of a
 * device other than the scene's first; GNXR_ERR_UNSUPPORTED for a scene created without textures (the texture list is fixed);
 * GNXR_ERR_OOM.  n_textures == 0 is a no-op. */
int gnxr_scene_update_textures(gnxr_scene *scene, int32_t first_texture, int32_t n_textures, const gnxr_texture *textures, const float *texels, void *hip_stream);
/* Test hook, read from the scene's first device.  which 0: the device's texture records of all textures (`texture` ignored; 28 words per
 * texture: n_levels, the padded w0 and h0, wrap, trilinear, max_aniso, su, sv, du, dv, the first texel of each of 16 levels in the
 * packed buffer, two words of padding); which 1: the float4 (rgb_) texels of all levels of texture `texture`, level after level, each
 * read through its record's offset.  *n_bytes receives the size; out is filled when given and capacity_bytes allows.  GNXR_ERR_INVALID
 * for null arguments, which outside {0, 1} or, with which 1, a texture outside the list. */
int gnxr_scene_texture_tables(gnxr_scene *scene, int32_t which, int32_t texture, void *out, int64_t capacity_bytes, int64_t *n_bytes);
/* Replace the camera (and the medium it sits in, -1 == none) for later renders; same checks as gnxr_scene_create. */
int gnxr_scene_set_camera(gnxr_scene *scene, const gnxr_camera *camera, int32_t camera_medium);

/* -- Integrator seam (replaces integrator->Render(*worldScene, frameTime), RenderThread.cpp:175).
 * rgba_out: width*height*4 fp32, row-major, pixel (x,y) at (x + y*width)*4, the layout of
 * FrameBuffer::fbuffer (ui/FrameBuffer.h:136); A is written as 1.  With shard_count>1 only
 * the shard's rows are written.                                                          */
int gnxr_render(gnxr_scene *scene, const gnxr_render_params *params, float *rgba_out,
                gnxr_stats *stats);
/* Same, output stays in device memory (d_rgba_out is a HIP device pointer, e.g. the data_ptr
 * of a torch tensor) and the work is enqueued on `hip_stream` (a hipStream_t, may be NULL). */
int gnxr_render_device(gnxr_scene *scene, const gnxr_render_params *params, void *d_rgba_out,
                       void *hip_stream, gnxr_stats *stats);

/* Allocates, on every device of the handle, the path state a render with these parameters needs, without rendering anything: the
 * first gnxr_render / gnxr_render_device call with them then runs at its steady-state speed (the reference has no counterpart: its
 * per-thread MemoryArena grows inside Render, core/Integrator.cpp:262).  State buffers only ever grow; they are released with the scene.
 * It covers the path state of gnxr_render_adaptive_device with the same parameters too, but not that call's 26 bytes per pixel of
 * its own (sums over the even samples, state bytes, lists) nor its pinned count word: the first adaptive call of a size allocates
 * them inside the call -- run one small-budget adaptive call up front where the first frame must not allocate. */
int gnxr_render_reserve(gnxr_scene *scene, const gnxr_render_params *params);

/* Diagnostics of the handle's last PathIntegrator render: how many light-sampling vertices had their estimate added to the path's radiance
 * inside the traversal launch that traced their rays, and how many by the pass after it.  The two sum to the vertices the render queued;
 * with GNXR_NO_TRACE_NEE_APPLY set in the environment the first is 0.  Either pointer may be NULL.  (Not part of gnxr_stats: its layout is fixed.) */
int gnxr_scene_nee_apply_counts(gnxr_scene *scene, uint64_t *in_trace, uint64_t *by_sweep);

/* Diagnostics of the handle's last render under gnxr_set_profiling(4) (the counting 4-wide traversal): the triangles its traversal launches
 * loaded (gnxr_stats::tris_tested) and how many of them came from the block-local copy of the leaves next to the root of the tree.
 * Both are 0 after a render without the counting traversal.  Either pointer may be NULL. */
int gnxr_scene_hot_leaf_counts(gnxr_scene *scene, uint64_t *tris_from_lds, uint64_t *tris_loaded);

/* Diagnostics: the shape of the traversal launches of a render of this scene, for a launch of `total` work items, as the library sizes it.
 * stack_entries: the deepest traversal stack the walk can need; lds_entries: how many of them live in LDS (the others spill to memory);
 * lds_bytes: dynamic LDS per block of 256 threads; n_top: 4-wide nodes served from the block's LDS copy; hot_bytes: LDS bytes for the leaves
 * those nodes reference (0: none); blocks: blocks of the launch; blocks_per_cu: the blocks a compute unit is meant to hold at once
 * (lds_bytes and 1 KB kept back per block must fit that many times into its 160 KB); wide: the scene uses the 4-wide walk. */
typedef struct gnxr_trace_plan {
    int32_t wide, stack_entries, lds_entries, n_top, hot_bytes, blocks, blocks_per_cu, _pad;
    int64_t lds_bytes;
} gnxr_trace_plan;
int gnxr_scene_trace_plan(const gnxr_scene *scene, int64_t total, gnxr_trace_plan *plan);

/* -- Aggregate seam (replaces Scene::Intersect / Scene::IntersectP), batched ------------ */
int gnxr_trace_closest(gnxr_scene *scene, const gnxr_ray *rays, int64_t n, gnxr_hit *hits);
int gnxr_trace_any(gnxr_scene *scene, const gnxr_ray *rays, int64_t n, uint8_t *occluded);
/* Scene::Intersect / IntersectP for rays in DEVICE memory, ordered on the caller's stream; returns without waiting for the GPU.
 * d_rays: n gnxr_ray records in device memory (hipMalloc, a torch tensor's data_ptr), 16-byte aligned.  d_hits (4-byte aligned) /
 * d_occluded: n results in device memory of the same device.  Per ray the results are exactly those of gnxr_trace_closest /
 * gnxr_trace_any (same gnxr_hit fields, bit for bit; occluded = 1 when anything is hit in (0, tmax)).  The work is queued on
 * hip_stream (a hipStream_t; NULL: the null stream) after what the caller queued there: no synchronisation, no read-back, and no
 * allocation whose size depends on n (the call's scratch comes from the stream-ordered allocator on hip_stream).  Calls on different
 * streams against one handle may run at the same time, also while a gnxr_render_device of that handle is in flight.  With
 * gnxr_init_devices the call runs on the copy of the scene on the device that holds the pointers.  n == 0 is a no-op.
 * GNXR_ERR_INVALID, before anything is queued, for a null scene, a null pointer with n > 0, n < 0, pointers that are not device
 * memory (host memory, registered or not, goes through the two calls above), pointers on a device without a copy of the scene,
 * or a misaligned pointer.  The results may be read once the stream has reached them.                                            */
int gnxr_trace_closest_device(gnxr_scene *scene, const gnxr_ray *d_rays, int64_t n, gnxr_hit *d_hits, void *hip_stream);
int gnxr_trace_any_device(gnxr_scene *scene, const gnxr_ray *d_rays, int64_t n, uint8_t *d_occluded, void *hip_stream);

/* -- Radiance seam (SamplerIntegrator::Li, core/Integrator.h), batched on device memory ---------------------------------
 * For ray i, d_L[4i .. 4i+3] = (Li.r, Li.g, Li.b, 1): the Li of params->integrator along d_rays[i] (o, d; tmax bounds the first
 * Intersect; _pad is ignored), with the sampler of a render with these params -- HaltonSampler(spp, [0,width) x [0,height)) --
 * standing where Render leaves it after GetCameraSample: pixel (px, py), sample s of d_samples[i], dimension 5.  The ray starts in
 * d_samples[i].medium (-1: none; only VolPath reads it).  Render is this Li on the camera rays, summed in sample order and divided
 * by spp (core/Integrator.cpp:256-293), so a camera ray and its record give exactly the L that Render adds for that sample.
 * max_depth, rr_threshold, integrator, light_strategy, direct_strategy and passes_in_flight mean what they mean for gnxr_render;
 * samples_per_pass is the number of paths per sub-pass (0 = auto); spp_begin, spp_end and shard_index must be 0, shard_count and
 * shard_rows 0 or 1.  The work is ordered after what hip_stream holds; the call returns once d_L is written (stats needs the
 * device counters).  stats is filled as by a render, with camera_samples = n.  One render or Li call per handle at a time; path
 * state comes from the handle's buffers.  With gnxr_init_devices the call runs on the copy of the scene on the arrays' device.
 * GNXR_ERR_INVALID, before anything is queued: null scene or params, a null pointer with n > 0, n < 0, arrays that are not device
 * memory, on a device without a copy of the scene, on different devices or not 16-byte aligned, invalid params.
 * GNXR_ERR_UNSUPPORTED: spp beyond the 32-bit Halton indices of gnxr_render; Whitted, DirectLighting or VolPath on a scene with
 * image textures (their first texture lookup needs camera ray differentials).  A record out of range (px, py outside the image,
 * s outside [0, spp), medium outside [-1, n_media)) gets L = (0, 0, 0, 0); the other rays are finished and the call returns
 * GNXR_ERR_INVALID naming the first such record.  n == 0 is a no-op.                                                         */
int gnxr_li_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_ray *d_rays, const gnxr_li_sample *d_samples, int64_t n,
                   float *d_L, void *hip_stream, gnxr_stats *stats);

/* -- Many cameras in one render, on device memory ------------------------------------------------------------------------
 * gnxr_render_views_device renders n_views images of one scene in one call.  cameras (host memory, n_views records) and
 * camera_media (host memory, n_views entries in [-1, n_media); NULL: all -1) name each view's camera and the medium it sits in;
 * d_rgba_out is device memory for n_views images of width*height*4 fp32, image v at v*width*height*4, each in the layout of
 * gnxr_render_device.  Image v is, bit for bit, what gnxr_scene_set_camera(scene, &cameras[v], camera_media[v]) followed by
 * gnxr_render_device(scene, params, ...) writes; the scene's own camera is neither read nor changed.  The views are one path
 * population (a pixel index that carries the view number), so sub-passes are sized on n_views*width*height pixels: many small
 * images fill the device where one would not.  spp_begin / spp_end, samples_per_pass (samples of EVERY view per sub-pass),
 * passes_in_flight, max_depth, the integrator and the strategies mean what they mean for gnxr_render_device; all four
 * integrators are supported.  shard_index must be 0, shard_count and shard_rows 0 or 1 (a caller that shards splits the list of
 * views).  stats carries the sums of the ray counters and of camera_samples over the views.  Locking and ordering as for
 * gnxr_render_device: one render, Li or views call per handle at a time, queued after what hip_stream holds, back when the images
 * are written.  With gnxr_init_devices the call runs on the copy of the scene on the device that holds d_rgba_out.  n_views == 0
 * is a no-op.
 * GNXR_ERR_INVALID, before anything is queued: null scene or params; null cameras with n_views > 0; n_views < 0; an output that is
 * null, not device memory, on a device without a copy of the scene or not 16-byte aligned; invalid params or shard fields; a
 * medium outside [-1, n_media); n_views*width*height beyond the 32-bit path indexing (at most (2^32 - 1) / 3 pixels per call).
 * GNXR_ERR_UNSUPPORTED: what gnxr_render_device refuses, and VolPath on a scene with image textures (its shade kernels recompute
 * the camera's ray differentials at the first surface; Whitted and DirectLighting store them per path at raygen and render views
 * of textured scenes, PathIntegrator does not use them).
 *
 * gnxr_camera_rays_device is the device-memory form of gnxr_camera_rays and needs no scene: for sample d_s[i] of pixel
 * (d_px[i], d_py[i]) of a HaltonSampler over [0,width) x [0,height) it writes the camera ray into d_rays[i] -- o and d with the
 * bits gnxr_camera_rays gives, tmax = +inf, _pad = 0 -- and {px, py, s, camera_medium} into d_samples[i]: the two arrays
 * gnxr_li_device takes.  All five arrays are device memory of one device; d_rays and d_samples 16-byte aligned, the int arrays
 * 4-byte aligned.  The kernel runs on hip_stream after what the caller queued there; no allocation grows with n (the sampler
 * tables are uploaded once per device, the status word comes from the stream-ordered allocator).  A record with px, py outside
 * the image or s < 0 gets a zeroed ray and sample; the other records are finished and the call returns GNXR_ERR_INVALID naming
 * the first such record.  That status has to come back, so the call waits for its own kernel (hip_stream is synchronised)
 * before it returns, as gnxr_light_sample_device does.  n == 0 is a no-op.  GNXR_ERR_INVALID, before anything is queued: a null
 * camera, a null array with n > 0, n < 0, width or height <= 0, camera_medium < -1, arrays that are not device memory, on
 * different devices or misaligned.                                                                                            */
int gnxr_render_views_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_camera *cameras, const int32_t *camera_media,
                             int32_t n_views, void *d_rgba_out, void *hip_stream, gnxr_stats *stats);
int gnxr_camera_rays_device(const gnxr_camera *camera, int32_t camera_medium, int32_t width, int32_t height, const int32_t *d_px,
                            const int32_t *d_py, const int32_t *d_s, int64_t n, gnxr_ray *d_rays, gnxr_li_sample *d_samples, void *hip_stream);

/* -- First-hit feature buffers on device memory: depth, normals, albedo and ids per view -----------------------------------
 * gnxr_render_aov_device writes, for n_views images of one scene, the buffers a denoiser or a data-set writer wants beside the beauty
 * image, anti-aliased exactly as the beauty image is: for view v, pixel (x, y) and every sample s of [spp_begin, spp_end) (0, 0 = all)
 * the camera ray is the one gnxr_camera_rays_device writes for cameras[v] -- the one gnxr_render_views_device traces -- and the hit is
 * Scene::Intersect on it with the bits of gnxr_trace_closest_device (spheres included).  cameras == NULL with n_views == 1 means the
 * scene's own camera and camera medium (camera_media is then not read).  Per channel the per-sample values are added in fp32 in
 * increasing sample order, starting from 0, and the sum is divided by (float)spp -- what the render does with L -- so a call over
 * [a, b) returns that range's share of the mean and the shares of disjoint ranges add up.  A miss adds 0 to every channel.  Image v of
 * a channel sits at v*width*height*stride, pixel (x, y) at x + y*width.
 *   d_albedo          the albedo of the hit's material (gnxr_material_albedo; where kd_texture != 0 the kd is the UNFILTERED lookup of
 *                     that texture at the hit's uv: the lookup PathIntegrator's shade kernel makes, hasDifferentials == false);
 *                     w = coverage: 1 added per sample that hit anything
 *   d_normal          gnxr_hit.n: the geometric normal, flipped onto the shading side on triangles with normals or tangents; w = 0
 *   d_shading_normal  the shading normal the shade kernels build the BSDF on: interpolated per-vertex normals, the SetShadingGeometry
 *                     flip, Material::Bump with the zero map (has_bump), a sphere's own; w = 0
 *   d_depth           gnxr_hit.t
 *   d_ids             not averaged: {gnxr_hit.prim, material} of the LOWEST sample of the call's range (spp_begin), {-1, -1} on a miss.
 *                     The material is the index into desc.materials as authored (spheres[i].material for a sphere), never the
 *                     internal copy triangles with uvs or normals of their own are given; -1 where the surface has no material
 *                     (index -1 or a GNXR_MAT_NONE material: a medium boundary)
 * FIRST HIT ONLY: a null-material surface is a hit like any other (material -1, albedo 0, its own depth and normals); the buffers
 * neither follow specular bounces nor step through medium boundaries.
 * params: width, height, spp, spp_begin, spp_end as for gnxr_render_views_device; samples_per_pass = samples of EVERY view per
 * sub-pass (0 = auto: sized from the free device memory; the buffers do not depend on it); integrator, max_depth, rr_threshold, the
 * strategies and passes_in_flight are ignored; shard_index must be 0, shard_count and shard_rows 0 or 1.  The call keeps 32 bytes per
 * camera sample of a sub-pass (the ray; the hit's leaf code travels in its pad word) and 16 to 48 bytes per pixel of running sums, all
 * from the stream-ordered allocator: nothing of the path state gnxr_render_reserve allocates is touched.  stats receives
 * camera_samples, rays_closest, passes, kernel_launches, state_bytes and the seconds.  Locking, stream ordering, the choice of the
 * copy under gnxr_init_devices (the device that holds the buffers) and n_views == 0 (a no-op) are as for gnxr_render_views_device;
 * the call returns when the buffers are written.
 * GNXR_ERR_INVALID, before anything is queued: a null scene, params or out; all five channels NULL; a channel that is not device
 * memory, on a device without a copy of the scene or on another device than the others; a four-float channel that is not 16-byte
 * aligned, depth or ids not 4-byte aligned; n_views < 0; null cameras with n_views > 1; a medium outside [-1, n_media); invalid
 * params or shard fields; n_views*width*height beyond the limit of gnxr_render_views_device.  GNXR_ERR_UNSUPPORTED: spp beyond the
 * 32-bit Halton indices of gnxr_render.
 *
 * gnxr_material_albedo (host, needs no device) is the single definition of a material's albedo; the device table is built with it.
 *   MATTE, PLASTIC, DISNEY : kd, each channel clamped to [0, inf) as the materials clamp it (Spectrum::Clamp)
 *   MIRROR                 : kr, clamped the same way
 *   GLASS                  : (1, 1, 1)
 *   METAL                  : the conductor's reflectance at normal incidence, per channel in fp32, every operation rounded on its own
 *                            (no fused multiply-add), in this order:
 *                                a = eta - 1;  b = eta + 1;  k2 = k * k;  num = a * a + k2;  den = b * b + k2;  albedo = num / den
 *   NONE                   : 0
 * A kd_texture does not change the value returned here (the texture is looked up per hit on the device).  GNXR_ERR_INVALID for a
 * null pointer or an unknown type.                                                                                              */
typedef struct gnxr_aov_buffers {   /* device pointers; NULL = channel not wanted */
    float   *d_albedo;          /* V*W*H*4: mean albedo rgb, w = coverage (fraction of the spp samples that hit anything) */
    float   *d_normal;          /* V*W*H*4: mean geometric normal (the bits of gnxr_hit.n per sample), w = 0 */
    float   *d_shading_normal;  /* V*W*H*4: mean shading normal (the ns the shade kernels build the BSDF on), w = 0 */
    float   *d_depth;           /* V*W*H:   mean gnxr_hit.t */
    int32_t *d_ids;             /* V*W*H*2: {gnxr_hit.prim, material index} of the LOWEST sample of the call's range; -1,-1 on a miss */
} gnxr_aov_buffers;
int gnxr_render_aov_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_camera *cameras, const int32_t *camera_media,
                           int32_t n_views, const gnxr_aov_buffers *out, void *hip_stream, gnxr_stats *stats);
int gnxr_material_albedo(const gnxr_material *m, float rgb[3]);

/* -- Adaptive sampling on device memory: render to a noise threshold, per-pixel sample counts ------------------------------
 * gnxr_render_adaptive_device renders the scene's camera like gnxr_render_device, but lets every pixel stop as soon as its two
 * half estimates agree.  params->spp is the sample budget and the samplesPerPixel of the HaltonSampler: sample s of pixel (x, y)
 * is the camera sample of gnxr_render_device -- the same Halton index, camera ray and Li.
 * Per pixel: S = rgb fp32 sums of Li over its samples s = 0, 1, 2, ... in that order from +0 (what a render accumulates), A = the
 * same sums over the even s only, n = samples taken, active = true.  Round 0 gives every pixel samples [0, min_spp); each later
 * round gives every active pixel, which has n samples, its next max(step_spp, n / 8) samples (integer division), cut at spp: the
 * steps grow with n once n exceeds 8 step_spp, so that the number of rounds -- each ends with a drain of the device -- stays
 * logarithmic in spp / step_spp, and a late decision comes at most an eighth of a pixel's samples late.  After a round every pixel that was active in it computes,
 * in single fp32 operations in the written order (no fused multiply-add, no division, no square root):
 *     e = (|Sr - (Ar + Ar)| + |Sg - (Ag + Ag)|) + |Sb - (Ab + Ab)|
 *     m = (Sr + Sg) + Sb
 *     bound = threshold * (m + floor * (float)n)
 *     noisy = !(e <= bound)                                   (a NaN keeps the pixel sampling)
 * and then active' = active && n < spp && (some pixel q with |qx - x| <= guard and |qy - y| <= guard inside the image has
 * active_q && noisy_q).  A pixel that has stopped never restarts; the call ends when no pixel is active.  Note that threshold = 0
 * still stops a pixel whose e is exactly 0.
 * Outputs (device memory): d_rgba_out, (H, W, 4) fp32 in the layout of gnxr_render_device, pixel = (Sr / (float)n, Sg / (float)n,
 * Sb / (float)n, 1); d_count_out, (H, W) int32 = n, may be NULL.  With min_spp == spp the image and the ray counters are those of
 * gnxr_render_device bit for bit.  info (host memory, required): rounds run, samples = the sum of n, pixels_at_budget = pixels with
 * n == spp.  stats is filled as by a render: camera_samples = the sum of n, the ray counters are the sums over all rounds.
 * Of params: spp_begin and spp_end must be 0; shard_index 0, shard_count and shard_rows 0 or 1; samples_per_pass = PATHS per
 * sub-pass of a round, as for gnxr_li_device (0 = auto: a round is one sub-pass while it fits the path state of a render with these params, else that render's sub-passes);
 * passes_in_flight keeps its meaning; the results depend on neither.  All four integrators are supported; on a scene with image
 * textures PathIntegrator is supported, Whitted, DirectLighting and VolPath return GNXR_ERR_UNSUPPORTED (their shade kernels
 * find the camera's ray differentials through the slot of a path, as for gnxr_li_device).
 * Memory: 42 bytes per pixel of state (S and n, A, two state bytes, two list entries), of which 26 are allocated by the handle's
 * first adaptive call of a size; nothing grows with width*height*spp.  Path state comes from the handle's buffers, sized for the
 * largest round, and never exceeds what gnxr_render_reserve allocates for the same gnxr_render_params.  The host reads one
 * 4-byte count per round (the size of the next round) and nothing else.
 * Locking, ordering and device selection as for gnxr_render_views_device: one render per handle at a time, queued after what
 * hip_stream holds, back when the outputs are written; with gnxr_init_devices the call runs on the copy of the scene on the
 * device that holds d_rgba_out.
 * GNXR_ERR_INVALID, before anything is queued (the outputs stay untouched): a null scene, params, adaptive, d_rgba_out or info; a
 * struct_size other than sizeof of its record; an output that is not device memory, on a device without a copy of the scene, on
 * another device than the other, or misaligned (16 bytes for d_rgba_out, 4 for d_count_out); invalid params or shard fields;
 * min_spp outside [1, spp], step_spp < 1, guard outside [0, 8], threshold or floor negative or NaN.
 * The two records carry struct_size, like gnxr_geometry; they are not part of gnxr_abi_sizeof's list.                          */
typedef struct gnxr_adaptive_params { int32_t struct_size, min_spp, step_spp, guard; float threshold, floor; } gnxr_adaptive_params;
typedef struct gnxr_adaptive_info { int32_t struct_size, rounds; int64_t samples; int64_t pixels_at_budget; } gnxr_adaptive_info;
int gnxr_render_adaptive_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_adaptive_params *adaptive, void *d_rgba_out,
                                int32_t *d_count_out, void *hip_stream, gnxr_stats *stats, gnxr_adaptive_info *info);

/* -- Edge-aware image denoiser on device memory, guided by the feature buffers ----------------------------------------------
 * gnxr_denoise_device filters n_views images of width x height pixels with an edge-avoiding a-trous wavelet filter (Dammertz et al.
 * 2010) whose colour weight is the variance-guided one of SVGF, the variance estimated from two independent half renders.  It is a
 * pure image operation: no scene handle; the device is the one that holds d_color (as gnxr_camera_rays_device finds it); the work is
 * queued on hip_stream after what the stream holds and the call returns without waiting for the GPU; scratch, 48 bytes per pixel
 * (two ping-pong work records and one guide record), comes from the stream-ordered allocator.  d_rgba_out may be d_color or
 * d_color_b (in place: the same address); it may not overlap a share at any other offset, nor a guide.  n_views == 0 is a no-op.  Image v of a buffer sits at v*width*height*stride,
 * pixel (x, y) at x + y*width; no tap crosses from one view into another.
 * "Shares": d_color alone is the image.  With d_color_b the two are the shares of the image that two renders of disjoint sample
 * ranges return (spp_begin / spp_end: samples [0, N/2) and [N/2, N) of spp = N): they add up to the image, and with equal halves
 * (a - b)^2 estimates the variance of the mean.
 * The definition.  Every operation is a single fp32 operation in the written order (no fused multiply-add; division and sqrt are
 * IEEE); expf is glibc's (the bits of gnxr_eval_libm, fn = 1).  lum(x) = (0.212671f*x.r + 0.715160f*x.g) + 0.072169f*x.b.
 *   Prepare, per pixel:
 *     div_c = max(albedo_c + (1 - coverage), 1/1024) per channel (t > 1/1024 ? t : 1/1024: a NaN gives 1/1024), or 1 without
 *             d_albedo -- a missed sample counts as albedo 1, so an environment background is not divided away
 *     with d_color_b:     c_c = (a_c + b_c) / div_c;   d = lum(a / div) - lum(b / div);   v = d * d
 *     without:            c_c = a_c / div_c;   v = 0
 *     a pixel with a non-finite c_c or v is INVALID, its work record (0, 0, 0, -1); otherwise the record is (c.r, c.g, c.b, v).
 *     The guide record is (n.x, n.y, n.z, depth), zeros for absent guides.
 *   Host constants: inv_sn = 1 / (sigma_normal * sigma_normal), inv_sc = 1 / (sigma_color * sigma_color).  A sigma of 0 or an absent
 *     guide switches that term off (the term is +0).
 *   Iteration i = 0 .. iterations-1, step s = 2^i, per pixel p of view v:
 *     the colour term is used when sigma_color > 0.  With d_color_b: vbar_p = (sum g*v_q) / (sum g) over the valid in-image pixels
 *     q of the 3 x 3 window at distance 1 (dy outer -1..1, dx inner -1..1; g = 1/4 at the centre, 1/8 at the edges, 1/16 at the
 *     corners; 0 when the window has no valid pixel) and inv_c = 1 / (sigma_color * sqrt(vbar_p) + 1e-6f).  With d_depth and
 *     sigma_depth > 0: inv_z = 1 / ((sigma_depth * (float)s) * z_p + 1e-20f).
 *     Taps in the order dy = -2..2 outer, dx = -2..2 inner, q = p + s*(dx, dy); a tap outside the image of view v or on an invalid q
 *     is skipped; h = k[|dy|] * k[|dx|] with k = {3/8, 1/4, 1/16}.  x_c is 0 when p is invalid, else
 *       with d_color_b:   x_c = |lum(c_p) - lum(c_q)| * inv_c
 *       without:          dc = c_p - c_q;  x_c = ((dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b) * (inv_sc * 4^i)
 *       dn = n_p - n_q;   x_n = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_sn
 *       x_z = |z_p - z_q| * inv_z
 *       w = h * expf(-((x_c + x_n) + x_z))
 *     A tap with !(w > 0) is skipped (NaN included).  Otherwise, from +0: sum_c += w * c_q per channel; sum_w += w;
 *     sum_v += (w*w) * v_q.  If sum_w > 0: c' = sum_c / sum_w, v' = sum_v / (sum_w*sum_w) and the pixel is valid from here on;
 *     otherwise its record is kept as it is.
 *   Output: out.rgb = c * div; out.w = d_color.w of that pixel; a pixel that is still invalid gets a.rgb (a.rgb + b.rgb with a
 *     second image), unchanged.
 * GNXR_ERR_INVALID, before anything is queued (the output stays untouched): a null params, in, d_color or d_rgba_out; a struct_size
 * other than sizeof of its record; width or height < 1, n_views < 0; iterations outside [1, 8]; a negative or NaN sigma; a pointer
 * that is not device memory or is on another device than d_color; a four-float buffer that is not 16-byte aligned, a d_depth that
 * is not 4-byte aligned; d_rgba_out overlapping a guide, or a share at another address than its own; n_views*width*height beyond the limit of gnxr_render_views_device.
 * The two records carry struct_size; they are not part of gnxr_abi_sizeof's list.                                               */
typedef struct gnxr_denoise_params { int32_t struct_size, width, height, n_views, iterations;
                                     float sigma_color, sigma_normal, sigma_depth; } gnxr_denoise_params;
typedef struct gnxr_denoise_buffers { int32_t struct_size, pad;
    const float *d_color;    /* V*H*W*4, required: the image, or the first of two shares of it            */
    const float *d_color_b;  /* V*H*W*4 or NULL: the second share (an independent estimate, see above)    */
    const float *d_albedo;   /* V*H*W*4 or NULL: rgb + coverage, the layout of gnxr_aov_buffers.d_albedo  */
    const float *d_normal;   /* V*H*W*4 or NULL: either normal channel of gnxr_aov_buffers                */
    const float *d_depth;    /* V*H*W   or NULL                                                           */
} gnxr_denoise_buffers;
int gnxr_denoise_device(const gnxr_denoise_params *params, const gnxr_denoise_buffers *in, float *d_rgba_out, void *hip_stream);

/* -- Film: pixel reconstruction filters for renders on device memory ---------------------------------------------------------
 * gnxr_render_device forms a pixel as the unweighted mean of its own samples.  The film forms it as pbrt-v3's Film does
 * (Film::AddSample / WriteImage): every sample is weighted into all pixels within the filter's radius of its position on the film,
 * a pixel being the weighted sum over the weight sum.  It is defined here operation by operation in fp32, with an order of
 * accumulation, so that a restatement reproduces it bit for bit.  Every operation is a single fp32 operation in the written order
 * (no fused multiply-add; division is IEEE).
 *
 * The filter record.  kind: GNXR_FILTER_BOX, _TRIANGLE, _GAUSSIAN (a = alpha), _MITCHELL (a = B, b = C) or _TABLE (table = 256 floats
 * in host memory, read during the call); radius_x, radius_y in [0.5, 4].  The record carries struct_size and is not part of
 * gnxr_abi_sizeof's list.
 *
 * The filter table.  gnxr_film_filter_table (host, needs no device) is the single definition of the 16 x 16 table every other call
 * of this block builds from the record: out[y*16 + x] = Evaluate(px, py) with px = (((float)x + 0.5f) * radius_x) / 16.f and py
 * likewise (rx = radius_x, ry = radius_y):
 *   BOX       1
 *   TRIANGLE  max(0, rx - |px|) * max(0, ry - |py|)
 *   GAUSSIAN  G(px, expX) * G(py, expY);  G(d, e) = max(0.f, expf(((-a) * d) * d) - e);  expX = expf(((-a) * rx) * rx), expY likewise
 *             (GaussianFilter.h:16-32); expf is the host C library's
 *   MITCHELL  M(px / rx) * M(py / ry) with pbrt-v3's Mitchell1D, written out:
 *               x = |2.f * t|
 *               x > 1:  ((((((-B - 6.f*C) * x) * x) * x + (((6.f*B + 30.f*C) * x) * x)) + ((-12.f*B - 48.f*C) * x)) + (8.f*B + 24.f*C)) * (1.f / 6.f)
 *               else:   (((((12.f - 9.f*B) - 6.f*C) * x) * x) * x + ((((-18.f + 12.f*B) + 6.f*C) * x) * x) + (6.f - 2.f*B)) * (1.f / 6.f)
 *             (sums left to right; in the second form: (cubic + quadratic) + constant)
 *   TABLE     a copy of the caller's 256 values
 *
 * Adding samples.  gnxr_film_add_device adds n_layers layers of samples to an accumulator; all three arrays are device memory of
 * one device.  With npix = n_views*width*height and pixel lp = v*width*height + x + y*width:
 *   d_L        (n_layers, npix, 4) fp32: the sample of layer j that belongs to pixel lp at (j*npix + lp)*4; w is ignored
 *   d_offsets  (n_layers, npix, 2) fp32: its film offset (ux, uy) inside that pixel
 *   d_accum    (npix, 4) fp32, read and written: (Sr, Sg, Sb, Wt)
 * For layer j ascending, then source row qy ascending, then source column qx ascending, a sample with both offsets in [0, 1] has
 *     dx = ((float)qx + ux) - 0.5f;   x0 = (int)ceilf(dx - rx);   x1 = (int)floorf(dx + rx) + 1;        the same in y
 * and every pixel (x, y) of the same view with x0 <= x < x1 and y0 <= y < y1 inside the image receives
 *     fx = fabsf(((float)x - dx) * (1.f / rx) * 16.f)   (left to right);   ifx = min((int)floorf(fx), 15);      ify likewise
 *     w = table[ify*16 + ifx];   S.c = S.c + L.c * w   (the product rounded, then the sum);   Wt = Wt + w
 * A sample with an offset outside [0, 1], or NaN, adds nothing.  A destination pixel receives its contributions in the order
 * (j, qy, qx) ascending: that order is the definition, and because j is outermost it does not depend on how layers are batched.
 * Nothing crosses from one view into another.  The work is queued on hip_stream and the call does not wait for the GPU; the
 * device is the one that holds d_accum.  n_views == 0 and n_layers == 0 are no-ops.
 *
 * Resolving.  gnxr_film_resolve_device writes pixel lp of d_rgba_out as (c(Sr), c(Sg), c(Sb), 1): c(S) = 0 where Wt == 0, otherwise
 * t = S / Wt, replaced by 0 where t < 0 (a NaN stays).  A division, not pbrt's multiplication by the reciprocal, so that the box
 * case below meets gnxr_render_device.  d_rgba_out may be d_accum.  Queued on hip_stream, like the add.
 *
 * Rendering through the film.  gnxr_render_filtered_device is gnxr_render_views_device with this film in place of the unweighted
 * mean.  cameras == NULL with n_views == 1 means the scene's own camera and camera medium, as for gnxr_render_aov_device.  One layer is
 * added per sample s of [spp_begin, spp_end) in ascending order: for pixel (x, y) its L is the Li that gnxr_render_device adds for
 * that sample, and (ux, uy) are dimensions 0 and 1 of its Halton sample (gnxr_sample_halton; the film position camera_ray() shoots
 * through).  d_accum == NULL uses an internal accumulator, zeroed first; otherwise the call accumulates into the caller's
 * (npix, 4) buffer, which is zeroed first unless flags has GNXR_FILM_CONTINUE.  d_rgba_out (n_views images, resolved) may be NULL
 * when d_accum is given; at least one of the two is required.  samples_per_pass and passes_in_flight keep their meaning and the
 * result depends on neither.  shard_index must be 0, shard_count and shard_rows 0 or 1: a filter reads its neighbours' samples, so a
 * caller who shards splits the views.  All four integrators; the support matrix is gnxr_render_device's for the scene's own camera
 * and gnxr_render_views_device's with cameras.  Locking, stream ordering and the choice of the device are as for
 * gnxr_render_views_device; the call returns when the outputs are written.  n_views == 0 is a no-op.
 *
 * What follows from the definition:
 *   - a call over [0, a) followed by a call over [a, b) with GNXR_FILM_CONTINUE leaves the bits of one call over [0, b); the same
 *     holds for gnxr_film_add_device split by layers;
 *   - with BOX and radius 0.5 every weight is 1, and a pixel whose Wt == (float)spp carries gnxr_render_device's bits;
 *   - pbrt's window lets a sample with an offset of exactly 0 also reach the pixel below or left of it, and a sample whose qx + ux
 *     rounds to qx + 1 the pixel above or right of it: those receivers differ from gnxr_render_device.
 *
 * GNXR_ERR_INVALID, before anything is queued (the outputs stay untouched): a null or mis-sized filter record; an unknown kind; a
 * radius outside [0.5, 4] or NaN; a NULL table with TABLE; buffers that are null, not device memory, on different devices, on a
 * device without a copy of the scene, or not 16-byte aligned (8 for d_offsets); width or height < 1, negative n_views or n_layers;
 * unknown flag bits; the limits and parameter rules of gnxr_render_views_device.                                                 */
enum { GNXR_FILTER_BOX = 0, GNXR_FILTER_TRIANGLE = 1, GNXR_FILTER_GAUSSIAN = 2, GNXR_FILTER_MITCHELL = 3, GNXR_FILTER_TABLE = 4 };
#define GNXR_FILM_CONTINUE 1u   /* flags of gnxr_render_filtered_device: keep what d_accum holds */
typedef struct gnxr_film_filter { int32_t struct_size, kind; float radius_x, radius_y, a, b; const float *table; } gnxr_film_filter;
int gnxr_film_filter_table(const gnxr_film_filter *filter, float out[256]);
int gnxr_film_add_device(const gnxr_film_filter *filter, int32_t width, int32_t height, int32_t n_views, int32_t n_layers, const float *d_L,
                         const float *d_offsets, float *d_accum, void *hip_stream);
int gnxr_film_resolve_device(int32_t width, int32_t height, int32_t n_views, const float *d_accum, float *d_rgba_out, void *hip_stream);
int gnxr_render_filtered_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_film_filter *filter, const gnxr_camera *cameras,
                                const int32_t *camera_media, int32_t n_views, void *d_rgba_out, float *d_accum, uint32_t flags, void *hip_stream,
                                gnxr_stats *stats);

/* -- Lightmap baking: texture-space irradiance through Li, on device memory ----------------------------------------------------
 * A bake computes the light that arrives at the scene's triangles into a uv atlas (a lightmap) instead of a camera image.  It is
 * the texture-space front end of gnxr_li_device: gnxr_bake_texels_device rasterises the atlas, gnxr_surface_rays_device turns
 * (triangle, barycentrics, pixel, sample) into the rays and sample records gnxr_li_device takes, gnxr_bake_dilate_device fills the
 * gutters, and gnxr_bake_lightmap_device is the three of them around Li with an ordered reduction.  Everything is defined here
 * operation by operation in fp32 (single operations in the written order, no fused multiply-add, IEEE division and square root), so
 * that a restatement reproduces it bit for bit.  All arrays are device memory of one device that holds a copy of the scene (for
 * gnxr_bake_dilate_device: of one device); the work is queued on hip_stream after what the caller queued there, and scratch comes
 * from the stream-ordered allocator.  Triangles are named by their authoring index; spheres cannot be baked.
 *
 * Atlas rasterisation.  d_tri_lm_uv holds n_triangles * 6 floats, (u0 v0 u1 v1 u2 v2) per triangle in authoring order: a lightmap
 * uv set of the caller's (not the scene's tri_uv).  With E(a, b, c) = (b.u - a.u) * (c.v - a.v) - (b.v - a.v) * (c.u - a.u):
 *   area = E(p0, p1, p2);  a triangle with area == 0, a non-finite area or a non-finite uv covers nothing
 *   texel (x, y), row 0 at v near 0, has the centre P = (cu, cv) = (((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H)
 *   wa = E(p1, p2, P), wb = E(p2, p0, P), wc = E(p0, p1, P)
 *   P is covered when min(u) <= cu <= max(u) and min(v) <= cv <= max(v) over the three corners (fp32 comparisons; implied by the
 *   edge tests in exact arithmetic, stated so that the result never depends on which texels an implementation visits), and
 *   wa, wb, wc are all >= 0 (area > 0) or all <= 0 (area < 0): both windings bake, edges are inclusive
 * d_texel_tri[x + y*W] is the LOWEST index among the triangles that cover the centre, -1 where none does; d_texel_bary (may be
 * NULL) holds (b1, b2) = (wb / area, wc / area) of that triangle, (0, 0) where the texel is empty (b0 = wa / area = 1 - b1 - b2 up
 * to rounding is not stored).  uv outside [0, 1]^2 is simply outside the atlas.  The result does not depend on launch order.
 * d_tri_lm_uv and d_texel_tri 4-byte aligned, d_texel_bary 8-byte aligned; at most 2^30 texels.  Does not wait for the GPU.
 *
 * Surface rays.  For record i -- triangle d_tri[i], barycentrics (b1, b2) = d_bary[2i .. 2i+1], pixel (d_px[i], d_py[i]) and
 * sample d_s[i] of a HaltonSampler over [0, width) x [0, height) --
 *   p0, p1, p2 = the scene's CURRENT world-space vertices of the triangle (a bake after gnxr_scene_update_vertices or
 *   gnxr_scene_set_geometry sees the edit);  b0 = 1.f - b1 - b2
 *   p = b0*p0 + b1*p1 + b2*p2,  pError = gamma(7) * (|b0*p0| + |b1*p1| + |b2*p2|) per component,  n = Normalize(Cross(p0 - p2, p1 - p2)):
 *   the values Triangle::Intersect gives a hit with these barycentrics (gnxr_hit.n before any flip by shading normals); n is
 *   negated when flags has GNXR_BAKE_FLIP_NORMALS
 *   (u0, u1) = dimensions 3 and 4 of that Halton sample (gnxr_sample_halton): the pLens pair, which Li never draws and a pinhole
 *   camera skips, so the direction is decorrelated from everything Li draws from dimension 5 on
 *   w = CosineSampleHemisphere(u0, u1) (core/Sampling.h:140-145);  CoordinateSystem(n, &s, &t) (core/Geometry.h:988-995)
 *   d = (s * w.x + t * w.y) + n * w.z per component;  o = OffsetRayOrigin(p, pError, n, d) (core/Geometry.h:1408-1422)
 * d_rays[i] = (o, tmax = +inf, d, _pad = 0), d_samples[i] = {px, py, s, medium}: the two arrays gnxr_li_device takes; d_pn (may be
 * NULL) receives (p, 0, n, 0), 8 floats per record, n as flipped.  A degenerate triangle (zero world-space area) gets a zeroed ray,
 * sample and d_pn record and is no error.  A triangle outside [0, n_triangles), a pixel outside the image or s < 0 gets zeroed
 * records too; the other records are finished and the call returns GNXR_ERR_INVALID naming the first such record (the contract of
 * gnxr_camera_rays_device: the call waits for its own kernel).  d_rays, d_samples, d_pn 16-byte aligned, d_bary 8, the int arrays 4.
 * medium in [-1, n_media).  n == 0 is a no-op.  The call takes its turn with renders and edits on the copy of the scene it runs on.
 *
 * Dilation.  d_rgba is a width*height*4 fp32 image whose alpha is coverage; a texel starts out filled when alpha > 0.  Each of
 * `iterations` passes reads the previous pass's image and fill flags only: a texel that is not filled and has at least one filled
 * 8-neighbour inside the image takes rgb = (sum of the filled neighbours' rgb, added from 0 in (dy, dx) ascending order, dy
 * outermost) / (float)count and becomes filled.  Alpha is never changed, so a dilated texel stays distinguishable from a baked
 * one.  In place; d_rgba 16-byte aligned; iterations == 0 is a no-op.  Does not wait for the GPU.
 *
 * The bake.  params is the gnxr_render_params of Li: width, height = the atlas, spp = samples per texel; max_depth, rr_threshold,
 * the integrator and the strategies mean what they mean for gnxr_li_device; spp_begin, spp_end and shard_index must be 0,
 * shard_count and shard_rows 0 or 1.  For every covered texel (x, y) of the rasterisation and s in [0, spp), L_s is the Li of
 * gnxr_li_device along the surface ray of (tri, bary, px = x, py = y, s) with bake->flags and bake->medium; the texel is
 *   rgb = ((0 + L_0 + L_1 + ...) / (float)spp) * pi   (pi = 3.14159265358979323846f; sums in sample order, as Render sums),  alpha = 1
 * an empty texel is (0, 0, 0, 0), and bake->dilate dilation passes follow.  The result is the incident irradiance on the side n
 * points to; a triangle's own emission is not added.  A texel on a degenerate triangle receives L_s = 0.  The call runs in
 * sub-batches of samples through the front end of gnxr_li_device: samples_per_pass is the number of paths per sub-batch and per
 * sub-pass of Li (0 = auto), scratch for rays, sample records and L is bounded by a sub-batch, and the output depends on neither.
 * Locking, stream ordering, the choice of the device and stats (sums over the sub-batches; camera_samples = covered texels * spp)
 * follow gnxr_li_device, and the call returns when the lightmap is written.  GNXR_ERR_UNSUPPORTED: what gnxr_li_device refuses
 * (Whitted, DirectLighting or VolPath on a scene with image textures; spp beyond the 32-bit Halton indices).  GNXR_ERR_INVALID,
 * before anything is queued (the output stays untouched): null arguments, arrays that are not device memory, on a device without
 * a copy of the scene, on different devices or misaligned (d_rgba_out: 16 bytes), width or height < 1 or more than 2^30 texels,
 * invalid params, dilate < 0, unknown flag bits, medium outside [-1, n_media), struct_size != sizeof(gnxr_bake_params).
 * gnxr_bake_params carries struct_size, like gnxr_geometry; it is not part of gnxr_abi_sizeof's list.                            */
#define GNXR_BAKE_FLIP_NORMALS 1u   /* flags of gnxr_surface_rays_device and gnxr_bake_params: bake the back side */
typedef struct gnxr_bake_params { int32_t struct_size; uint32_t flags; int32_t dilate, medium; } gnxr_bake_params;
int gnxr_bake_texels_device(gnxr_scene *scene, const float *d_tri_lm_uv, int32_t width, int32_t height, int32_t *d_texel_tri, float *d_texel_bary,
                            void *hip_stream);
int gnxr_surface_rays_device(gnxr_scene *scene, int32_t width, int32_t height, const int32_t *d_tri, const float *d_bary, const int32_t *d_px,
                             const int32_t *d_py, const int32_t *d_s, int64_t n, uint32_t flags, int32_t medium, gnxr_ray *d_rays,
                             gnxr_li_sample *d_samples, float *d_pn, void *hip_stream);
int gnxr_bake_dilate_device(int32_t width, int32_t height, int32_t iterations, float *d_rgba, void *hip_stream);
int gnxr_bake_lightmap_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_bake_params *bake, const float *d_tri_lm_uv,
                              void *d_rgba_out, void *hip_stream, gnxr_stats *stats);

/* -- Light probes: L2 spherical-harmonic radiance at points in free space, on device memory ---------------------------------------
 * The other half of baked lighting: what a lightmap is for static, unwrapped surfaces a light probe is for everything that moves
 * through the scene.  A probe holds the incident radiance at a point, projected on the nine real spherical harmonics of bands 0
 * to 2, and gives the irradiance for any normal.  gnxr_lightprobe_rays_device turns (position, pixel, sample) into the rays and
 * sample records gnxr_li_device takes, gnxr_sh_project_device reduces (direction, L) pairs to coefficient sums in a defined order,
 * gnxr_sh_irradiance_device evaluates, and gnxr_bake_lightprobes_device is the first two around Li.  The conventions are those of
 * the lightmap section: single fp32 operations in the written order, no fused multiply-add, IEEE division and square root, sinf
 * and cosf the library's (gnxr_eval_libm); device memory of one device, work queued on hip_stream, scratch from the stream-ordered
 * allocator.
 *
 * The basis.  For a direction (x, y, z), slot j of a probe belongs to
 *   Y_0 = 0.282095f            Y_1 = 0.488603f*y           Y_2 = 0.488603f*z                          Y_3 = 0.488603f*x
 *   Y_4 = 1.092548f*(x*y)      Y_5 = 1.092548f*(y*z)       Y_6 = 0.315392f*((3.f*(z*z)) - 1.f)       Y_7 = 1.092548f*(x*z)
 *   Y_8 = 0.546274f*((x*x) - (y*y))
 * A probe is 9 float4, slot j = (r, g, b, 0).
 *
 * Probe rays.  For record i -- position d_pos[3i .. 3i+2], pixel (d_px[i], d_py[i]) and sample d_s[i] of a HaltonSampler over
 * [0, width) x [0, height) --
 *   (u0, u1) = dimensions 3 and 4 of that Halton sample (gnxr_sample_halton): the pLens pair, as for surface rays
 *   d = UniformSampleSphere(u0, u1) (core/Sampling.cpp:72-77):  z = 1.f - 2.f*u0,  r = sqrt(max(0.f, 1.f - z*z)),
 *   phi = (2.f*Pi)*u1 (Pi = 3.14159265358979323846f),  d = (r*cosf(phi), r*sinf(phi), z)
 * d_rays[i] = (o = the position, tmax = +inf, d, _pad = 0), d_samples[i] = {px, py, s, medium}.  A record with a non-finite
 * position, a pixel outside the image or s < 0 gets a zeroed ray and sample; the other records are finished and the call returns
 * GNXR_ERR_INVALID naming the first such record (the contract of gnxr_camera_rays_device: the call waits for its own kernel).
 * d_rays and d_samples 16-byte aligned, the others 4.  The scene gives the sampler tables and the range of medium, [-1, n_media).
 * n == 0 is a no-op.
 *
 * Projection.  d_rays (only d is read) and d_L (float4 per record, w ignored) hold n_probes * n_samples records in PROBE-MAJOR
 * order: record k*n_samples + s is sample s of probe k.  The term of sample s in slot j and channel c is L_s.c * Y_j(d_s).  The
 * sum is defined for a wave of 64 lanes:
 *   samples are cut into blocks of 64 consecutive samples; in block b, lane l holds the term of sample 64*b + l, or +0.0f when
 *   that sample is past n_samples
 *   for m = 32, 16, 8, 4, 2, 1 in this order every lane replaces its value by v[l] + v[l ^ m]; the block sum is lane 0's value
 *   (fp32 addition is commutative: every lane ends with the same bits)
 *   sum = (...((start + block_0) + block_1) + ...), in increasing block order; start = 0.0f, or what d_sh_sum holds when flags
 *   has GNXR_SH_CONTINUE
 * d_sh_sum[9k + j] = (sum_r, sum_g, sum_b, 0).  A caller who continues -- the samples of a probe spread over several calls --
 * passes whole blocks (n_samples a multiple of 64) in every call but the last: then the calls give the bits of one call over all
 * samples.  n_samples == 0 leaves start (0 without the flag).  All three arrays 16-byte aligned and on one device, which the
 * call runs on (no scene).  n_probes == 0 is a no-op.  Does not wait for the GPU.
 *
 * The bake.  params is the gnxr_render_params of Li: spp = samples per probe; width x height is a virtual grid of pixels whose
 * Halton sequences the probes use, and must hold n_probes pixels: probe k is pixel (k % width, k / width).  max_depth,
 * rr_threshold, the integrator and the strategies mean what they mean for gnxr_li_device; spp_begin, spp_end and shard_index must
 * be 0, shard_count and shard_rows 0 or 1.  For probe k at d_positions[3k .. 3k+2] and s in [0, spp), L_s is the Li of
 * gnxr_li_device along the probe ray of (position, px, py, s) with probe_params->medium, and
 *   d_sh_out[9k + j].rgb = (sum * 12.566370614359172f) / (float)spp,  w = 0,  sum = the projection's sum over all spp samples
 * (12.566370614359172f = 4 pi = 1 / the density of the directions).  A probe with a non-finite position gets zeros.  The call
 * runs in sub-batches -- ranges of probes, or ranges of whole blocks of one probe's samples -- through the front end of
 * gnxr_li_device: samples_per_pass is the number of paths per sub-batch (at least one block) and per sub-pass of Li (0 = auto),
 * scratch for rays, sample records and L is bounded by a sub-batch, and the output depends on neither: block sums are added one
 * after another however the samples are cut.  Locking, stream ordering, the choice of the device and stats (sums over the
 * sub-batches; camera_samples = n_probes * spp) follow gnxr_bake_lightmap_device, and the call returns when the coefficients are
 * written.  GNXR_ERR_UNSUPPORTED: what gnxr_li_device refuses.  GNXR_ERR_INVALID, before anything is queued (the output stays
 * untouched): null arguments, arrays that are not device memory, on a device without a copy of the scene, on different devices
 * or misaligned (d_positions: 4 bytes, d_sh_out: 16), n_probes < 0 or more than 2^27, a grid with fewer than n_probes pixels,
 * invalid params, flag bits (none is defined), medium outside [-1, n_media), struct_size != sizeof(gnxr_lightprobe_params).
 * n_probes == 0 is a no-op.  gnxr_lightprobe_params carries struct_size; it is not part of gnxr_abi_sizeof's list.
 *
 * Evaluation.  For record i with probe k = d_probe[i], coefficients c_j = d_sh[9k + j] and normal n = d_normals[3i .. 3i+2] (unit
 * length is the caller's business), per channel c
 *   E.c = ((((A0*(c_0.c*Y_0) + A1*(c_1.c*Y_1)) + A1*(c_2.c*Y_2)) + A1*(c_3.c*Y_3)) + A2*(c_4.c*Y_4)) + ... + A2*(c_8.c*Y_8)
 * left to right, Y_j = Y_j(n), A0 = 3.14159265f, A1 = 2.09439510f, A2 = 0.78539816f (the cosine lobe's band factors), and
 * d_E[i] = (E.r, E.g, E.b, 1).  A probe index outside [0, n_probes) gives a zeroed record; the others are finished and the call
 * returns GNXR_ERR_INVALID naming the first such record (it waits for its own kernel).  d_sh and d_E 16-byte aligned, d_probe and
 * d_normals 4; all on one device, which the call runs on (no scene).  n == 0 is a no-op.                                        */
#define GNXR_SH_CONTINUE 1u   /* flags of gnxr_sh_project_device: add to what d_sh_sum holds */
typedef struct gnxr_lightprobe_params { int32_t struct_size; uint32_t flags; int32_t medium; } gnxr_lightprobe_params;
int gnxr_lightprobe_rays_device(gnxr_scene *scene, int32_t width, int32_t height, const float *d_pos, const int32_t *d_px, const int32_t *d_py,
                                const int32_t *d_s, int64_t n, int32_t medium, gnxr_ray *d_rays, gnxr_li_sample *d_samples, void *hip_stream);
int gnxr_sh_project_device(const gnxr_ray *d_rays, const float *d_L, int32_t n_probes, int64_t n_samples, float *d_sh_sum, uint32_t flags,
                           void *hip_stream);
int gnxr_bake_lightprobes_device(gnxr_scene *scene, const gnxr_render_params *params, const gnxr_lightprobe_params *probe_params,
                                 const float *d_positions, int32_t n_probes, void *d_sh_out, void *hip_stream, gnxr_stats *stats);
int gnxr_sh_irradiance_device(const float *d_sh, int32_t n_probes, const int32_t *d_probe, const float *d_normals, int64_t n, float *d_E,
                              void *hip_stream);

/* -- Temporal accumulation: motion vectors and reprojected frame history, on device memory ------------------------------------------
 * What an interactive caller puts between its renderer and its spatial filter: where was this pixel's surface point on the previous
 * frame's film (gnxr_motion_device), is the history there still the same surface, and a blend of the new frame into the history that
 * survives the test (gnxr_temporal_accumulate_device).  Every operation is a single fp32 operation in the written order (no fused
 * multiply-add; division and sqrt are IEEE).  lum(x) = (0.212671f*x.r + 0.715160f*x.g) + 0.072169f*x.b, the denoiser's.  Raster
 * convention: the centre of pixel (x, y) is (x + 0.5, y + 0.5).  Image v of a buffer sits at v*width*height*stride, pixel (x, y) at
 * x + y*width.
 *
 * gnxr_camera_matrices (host, needs no device).  r2c (RasterToCamera) and c2w (CameraToWorld) are the matrices every kernel's camera
 * record holds for this camera over a width x height film; w2r is WorldToRaster = (ScreenToRaster * CameraToScreen) * WorldToCamera,
 * the product of the FORWARD fp32 matrices of the same three transforms r2c and c2w are made of (Transform::operator*: each entry
 * ((a0*b0 + a1*b1) + a2*b2) + a3*b3), not an inverse of r2c and c2w.  Row-major.  It is the single definition of w2r, as
 * gnxr_material_albedo is of the albedo: the kernels and the tests take the matrix from here.  Any output pointer may be NULL.
 * GNXR_ERR_INVALID: a null camera, width or height < 1.
 *
 * gnxr_motion_device: a pixel-centre G-buffer and where each pixel was one frame ago.  cameras: n_views records in host memory, or
 * NULL with n_views == 1 for the scene's own camera; prev_cameras (host memory, n_views records, required): the cameras of the
 * previous frame.  d_prev_vertices: NULL, or device memory of n_vertices*3 floats, the world-space vertex array the scene held one
 * frame ago in the layout of gnxr_scene_update_vertices.  For view v and pixel (x, y):
 *   Ray.  (o, d) by exactly the operations of the camera ray of a render for the film sample (fx, fy) = (0.5, 0.5), lens_radius
 *     taken as 0 whatever the camera says, tmax = +inf; no sampler table is read.
 *   Hit.  The bits of gnxr_trace_closest_device on that ray (the same front end, the same 4-wide walk; spheres included).
 *     d_guide = (hit.n, hit.t), (0, 0, 0, 0) on a miss; d_prim = hit.prim.
 *   Position one frame ago.  P = o + t*d per component (one multiply, one add).
 *     triangle hit with d_prev_vertices:  P' = (b0*q0 + b1*q1) + b2*q2 per component, qi the previous position of corner i of the
 *                                         hit triangle
 *     sphere hit, or no d_prev_vertices:  P' = P
 *     miss, perspective camera:           P' = E' + d, E' = (c2w'[3], c2w'[7], c2w'[11]) the previous camera's position (a direction
 *                                         keeps its place on the film under translation)
 *     miss, orthographic camera:          P' = o
 *     (the kind of the miss is that of the view's camera, the kind of the expected depth below that of prev_cameras[v])
 *   Projection.  With m = w2r of prev_cameras[v]:  xr = (m[0]*X + m[1]*Y) + (m[2]*Z + m[3]), and yr, zr, w the same from rows 1, 2
 *     and 3.  If w == 1, (x', y') = (xr, yr); otherwise (x', y') = (xr / w, yr / w).
 *   Expected previous depth.  Miss: t' = 0.  Perspective: e = P' - E', t' = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z).  Orthographic:
 *     t' = zr * 10.f (this undoes Orthographic(0, 10)).
 *   d_motion = (x', y', t', 1.0f) when w > 0 and x', y', t' are all finite; otherwise (0, 0, 0, 0).
 * Locking, stream ordering and the choice of the scene copy under gnxr_init_devices are those of gnxr_render_aov_device; scratch is
 * one ray per pixel from the stream-ordered allocator, which also holds the hit's leaf code (and the corner -> vertex table of the
 * refit, uploaded once per scene, when d_prev_vertices is given); the call returns when the buffers are written.  n_views == 0 is a no-op.
 * GNXR_ERR_INVALID, before anything is queued: a null scene, params, prev_cameras or out; a struct_size other than sizeof of its
 * record; width or height < 1, n_views < 0; all channels NULL; null cameras with n_views > 1; a channel or d_prev_vertices that is
 * not device memory or is on a device without a copy of the scene; d_motion or d_guide not 16-byte aligned, d_prim or
 * d_prev_vertices not 4-byte aligned; n_views*width*height beyond the limit of gnxr_render_views_device.
 *
 * gnxr_temporal_accumulate_device: validate, gather and blend; a pure image operation, no scene.  A stat record is (m1, m2, N, var):
 * first and second moment of the luminance, the history length as a float, the variance.  The history of the next frame is
 * (d_out_color, d_out_stat, this frame's d_guide, this frame's d_prim): the caller swaps.  Per pixel p = (x, y) of view v:
 *   c = d_color[p].rgb;  out.w = d_color[p].w;  l = lum(c);  cur_ok: the three channels of c are finite.
 *   Gather (skipped without history or when d_motion[p].w == 0).  (x', y', t') = d_motion[p].xyz.
 *     fx = x' - 0.5f, fy = y' - 0.5f.  Snap: if |fx - rintf(fx)| <= 1/256 then fx = rintf(fx), the same for fy (a static camera and
 *     scene are a single-tap copy, stable on bits).  Range, in float, before any conversion to int: no taps unless fx >= -1 &&
 *     fx < (float)W && fy >= -1 && fy < (float)H (NaN, inf and 1e30 give no taps).  x0 = floorf(fx), ax = fx - x0, the same in y.
 *     Taps in the order (i, j) = (0,0), (1,0), (0,1), (1,1), q = (x0 + i, y0 + j) inside view v (no tap crosses into another view),
 *     b = (i ? ax : 1 - ax) * (j ? ay : 1 - ay).  A tap counts iff b > 0, q is inside the image, hist_stat[q].z > 0,
 *     hist_prim[q] == prim[p], hist_color[q].rgb and hist_stat[q].xy are finite and, when prim[p] >= 0,
 *     |hist_guide[q].w - t'| <= depth_tol * t' and ((n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z) >= normal_cos (n_p = d_guide[p].xyz,
 *     n_q = hist_guide[q].xyz; a NaN fails either comparison).  From +0, over the taps that count: sw += b; sc += b * hc per
 *     channel; s1 += b * m1_q; s2 += b * m2_q; sN += b * N_q.  History exists iff sw > 0; then H = sc / sw, M1 = s1 / sw,
 *     M2 = s2 / sw, N = sN / sw.
 *   Blend.  var(m1, m2) = m2 - m1*m1, taken as 0 unless it is > 0.
 *     history and cur_ok:   N' = min(N + 1, (float)max_history); alpha = 1 / N'; out_c = H_c + alpha * (c_c - H_c);
 *                           m1' = M1 + alpha * (l - M1); m2' = M2 + alpha * (l*l - M2); stat (m1', m2', N', var(m1', m2'))
 *     no history, cur_ok:   out = c, stat (l, l*l, 1, 0)
 *     history, not cur_ok:  out = H, stat (M1, M2, N, var(M1, M2))
 *     neither:              out.rgb = 0, stat (0, 0, 0, 0)
 * The device is the one that holds d_color; the work is queued on hip_stream and the call returns without waiting for the GPU, as
 * gnxr_denoise_device; no scratch.  n_views == 0 is a no-op.  GNXR_ERR_INVALID, before anything is queued: a null params, io or
 * required pointer; a struct_size other than sizeof of its record; some but not all history pointers; width or height < 1,
 * n_views < 0; max_history < 1; a negative or NaN depth_tol, a NaN normal_cos; a pointer that is not device memory or is on another
 * device than d_color; a four-float buffer not 16-byte aligned, d_prim or d_hist_prim not 4-byte aligned; an output that overlaps
 * an input or the other output (the gather reads neighbours); n_views*width*height beyond the limit of gnxr_render_views_device.
 * A caller resets its history (passes NULL history once) after an edit that changes what a primitive id means or how surfaces
 * shade: new geometry, new lights, new materials.  The records carry struct_size; they are not part of gnxr_abi_sizeof's list.  */
int gnxr_camera_matrices(const gnxr_camera *camera, int32_t width, int32_t height, float r2c[16], float c2w[16], float w2r[16]);
typedef struct gnxr_motion_params  { int32_t struct_size, width, height, n_views; } gnxr_motion_params;
typedef struct gnxr_motion_buffers { int32_t struct_size, pad;
    float   *d_motion;  /* V*H*W*4: (x', y', t', flag)                       */
    float   *d_guide;   /* V*H*W*4: (n.x, n.y, n.z, t) of the centre hit     */
    int32_t *d_prim;    /* V*H*W  : gnxr_hit.prim of the centre hit, -1 miss */
} gnxr_motion_buffers;  /* NULL = channel not wanted; not all three NULL     */
int gnxr_motion_device(gnxr_scene *scene, const gnxr_motion_params *params, const gnxr_camera *cameras, const gnxr_camera *prev_cameras,
                       const float *d_prev_vertices, const gnxr_motion_buffers *out, void *hip_stream);
typedef struct gnxr_temporal_params { int32_t struct_size, width, height, n_views, max_history;
                                      float depth_tol, normal_cos; } gnxr_temporal_params;
typedef struct gnxr_temporal_buffers { int32_t struct_size, pad;
    const float *d_color;                                     /* V*H*W*4, required: this frame's image                       */
    const float *d_motion, *d_guide; const int32_t *d_prim;   /* required: this frame's, from gnxr_motion_device             */
    const float *d_hist_color, *d_hist_stat, *d_hist_guide; const int32_t *d_hist_prim;   /* all four, or all NULL (first frame) */
    float *d_out_color, *d_out_stat;                          /* V*H*W*4 each, required                                      */
} gnxr_temporal_buffers;
int gnxr_temporal_accumulate_device(const gnxr_temporal_params *params, const gnxr_temporal_buffers *io, void *hip_stream);

/* -- Display stage: auto-exposure, tone map and sRGB RGBA8, on device memory -----------------------------------------------------
 * The last link of a frame pipeline (render -> motion -> accumulate -> denoise -> display): from a linear float RGBA image in device
 * memory to bytes a window or a PNG takes, with an exposure that follows the scene and never leaves the device.  Three pure image
 * operations, no scene.  Every operation is a single fp32 operation in the written order (no fused multiply-add; division is IEEE);
 * expf and powf are the library's (gnxr_eval_libm: glibc's bits).  lum(x) = (0.212671f*x.r + 0.715160f*x.g) + 0.072169f*x.b, the
 * denoiser's.  Image v of a buffer sits at v*width*height*stride.  gnxr_framebuffer_update (host memory, one view, the reference
 * UI's constants) stays what it is.
 *
 * Common to the three calls.  The device is the one that holds the image (gnxr_exposure_device: the histogram); the work is queued
 * on hip_stream and the call returns without waiting for the GPU; no scratch.  n_views == 0 is a no-op.  GNXR_ERR_INVALID, before
 * anything is queued: a null params or required pointer; a struct_size other than sizeof of the record; width or height < 1,
 * n_views < 0; a parameter outside the range given below; a pointer that is not device memory, is on another device than the first
 * array, or whose extent runs past the end of its allocation; a four-float buffer, a histogram or an exposure record not 16-byte
 * aligned, an RGBA8 plane not 4-byte aligned; an output that overlaps an input (one exception: in-place exposure);
 * n_views*width*height beyond the limit of gnxr_render_views_device.  The records carry struct_size; they are not part of
 * gnxr_abi_sizeof's list.
 *
 * gnxr_luminance_histogram_device: a log-luminance histogram from the bit pattern of the luminance.  Integers only: the result is
 * exact and does not depend on the order in which pixels are counted.  min_log2 in [-126, 111].  d_hist: GNXR_HISTOGRAM_WORDS = 260
 * uint32 per view, overwritten (zeroed on the stream first).  Per pixel, l = lum(d_rgba[p].rgb), bits = the word of l:
 *   exponent field all ones (NaN, +-inf)                         hist[258]++
 *   otherwise !(l > 0) (0, -0, negatives)                        hist[256]++
 *   otherwise k = (int)(bits >> 19) - ((min_log2 + 127) << 4):   k < 0: hist[256]++ (subnormals too);  k > 255: hist[257]++;
 *                                                                else hist[k]++
 *   hist[259] stays 0.
 * Sixteen bins per octave over [2^min_log2, 2^(min_log2 + 16)): bin k covers a sixteenth of an octave's mantissa range, and its
 * coordinate min_log2 + (k + 0.5)/16 is a piecewise-linear log2, within -0.12 / +0.03 stop of the true one (the price of a histogram
 * without libm).  With min_log2 = -12: 2^-12 -> bin 0, 0.18 -> 151, 1.0 -> 192, the float below 16 -> 255, 16.0 -> above.
 *
 * gnxr_exposure_device: the exposure the histogram meters, adapted over time.  d_exposure: one float4 per view, (exposure, target,
 * L, kept weight).  d_prev_exposure: NULL, or the same layout; it may BE d_exposure (in place) but may not overlap it at an offset.
 * Refused unless 0 <= low < high <= 1, key > 0, 0 < rate <= 1, 0 < min_exposure <= max_exposure, every float finite, min_log2 in
 * [-126, 111].  Per view, sequentially -- the order is the definition:
 *   total = (float)(hist[0] + ... + hist[255], as integers);  skip = total*low;  keep = total*high - skip;  sw = sx = +0
 *   for k = 0 .. 255:  c = (float)hist[k];  s = fminf(c, skip);  c -= s;  skip -= s;
 *                      t = fminf(c, keep);  keep -= t;  sw += t;  sx += t * ((float)k + 0.5f)
 *   prev = d_prev_exposure ? d_prev_exposure[4v] : 0;  prev_ok: prev > 0 and finite
 *   sw > 0:  m = sx / sw;  L = (float)min_log2 + m * 0.0625f;
 *            target = fminf(fmaxf(key * powf(2.0f, -L), min_exposure), max_exposure)
 *   else:    L = 0;  target = prev_ok ? prev : 1.0f            (black, or everything out of range: hold)
 *   exposure = prev_ok ? prev + (target - prev) * rate : target
 *   d_exposure[4v ..] = (exposure, target, L, sw)
 * (the pixels between the quantiles low and high of the in-range luminances are averaged in log2; key / 2^L puts that average on
 * key.)
 *
 * gnxr_tonemap_device: exposure, curve, sRGB encoding, bytes.  curve: one of GNXR_TONEMAP_*; flags: GNXR_TONEMAP_SRGB |
 * GNXR_TONEMAP_ROUND, no other bit; exposure finite and >= 0; white in [1e-3, 65504] (read by REINHARD only, validated always).
 * d_exposure: NULL -- E = params.exposure -- or the float4-per-view record of gnxr_exposure_device -- E = d_exposure[4v], read on
 * the device.  d_rgba8_out: 4 bytes per pixel; it overlaps neither d_rgba nor d_exposure.  Per pixel and colour channel:
 *   x = in * E;  if !(x > 0) x = 0;  x = fminf(x, 65504.f)                        (NaN, negatives -> 0; +inf -> 65504)
 *   LINEAR     y = x
 *   REFERENCE  y = 1.0f - expf(-x / 0.25f)                                         (FrameBuffer::update_f_u_c's curve)
 *   REINHARD   y = (x * (1.0f + x / (white*white))) / (1.0f + x)
 *   ACES       y = (x * (2.51f*x + 0.03f)) / (x * (2.43f*x + 0.59f) + 0.14f)
 *   y = fminf(fmaxf(y, 0.f), 1.f)
 *   SRGB set   z = y <= 0.0031308f ? 12.92f*y : 1.055f * powf(y, 1.f/2.4f) - 0.055f   (GammaCorrect, core/GNXRayTracer.h:360)
 *      unset   z = y
 *   ROUND set  byte = (uint8)(z*255.f + 0.5f);  unset  byte = (uint8)(z*255.f)          (truncation is FrameBuffer's)
 * Alpha is 255; a pixel is the 32-bit word R | G<<8 | B<<16 | A<<24.  With REFERENCE, no flag and E = 1 the bytes are those of
 * gnxr_framebuffer_update(zeros, frame, 1) on a finite non-negative frame.                                                       */
#define GNXR_HISTOGRAM_WORDS 260
enum { GNXR_TONEMAP_LINEAR = 0, GNXR_TONEMAP_REFERENCE = 1, GNXR_TONEMAP_REINHARD = 2, GNXR_TONEMAP_ACES = 3 };   /* curve */
#define GNXR_TONEMAP_SRGB  1u   /* flags of gnxr_tonemap_device: encode with the sRGB transfer function */
#define GNXR_TONEMAP_ROUND 2u   /*                               round to the nearest byte instead of truncating */
typedef struct gnxr_histogram_params { int32_t struct_size, width, height, n_views, min_log2; } gnxr_histogram_params;
typedef struct gnxr_exposure_params { int32_t struct_size, n_views, min_log2, pad;
                                      float key, low, high, rate, min_exposure, max_exposure; } gnxr_exposure_params;
typedef struct gnxr_tonemap_params { int32_t struct_size, width, height, n_views, curve; uint32_t flags;
                                     float exposure, white; } gnxr_tonemap_params;
int gnxr_luminance_histogram_device(const gnxr_histogram_params *params, const float *d_rgba, uint32_t *d_hist, void *hip_stream);
int gnxr_exposure_device(const gnxr_exposure_params *params, const uint32_t *d_hist, const float *d_prev_exposure, float *d_exposure,
                         void *hip_stream);
int gnxr_tonemap_device(const gnxr_tonemap_params *params, const float *d_rgba, const float *d_exposure, uint8_t *d_rgba8_out,
                        void *hip_stream);

/* -- Deforming smooth meshes in place: pose -> moved vertices -> refit -> shading normals ---------------------------------
 * gnxr_skin_vertices_device makes the moved vertices, gnxr_scene_update_vertices[_ex] takes them (it accepts device memory) and
 * refits the tree, gnxr_scene_recompute_normals gives the smooth triangles the normals of the new shape, and
 * gnxr_scene_update_attributes replaces per-corner rows with the caller's own.  Every arithmetic step below is ONE rounded fp32
 * operation: nothing is contracted into a fused multiply-add, divisions and square roots are correctly rounded, and sums run in the
 * stated order, so a restatement in fp32 that follows the text reproduces the results bit for bit (tests/deform_reference.py).
 *
 * gnxr_scene_update_attributes: rows [first_triangle, first_triangle + n_triangles) of the scene's per-corner tables become the
 * caller's.  Triangles are in authoring numbering (gnxr_scene_desc.indices); tri_uv has 6 floats per triangle, tri_n and tri_s 9,
 * in the layout of gnxr_scene_desc; a NULL array leaves that table as it is.  The arrays are all host memory or all device memory of
 * the scene's first device (the rule of gnxr_scene_set_geometry); reads are ordered after work already queued on hip_stream, and the
 * call returns when every device of the scene holds the new rows.  Afterwards every result is, bit for bit, that of a scene created
 * with these attributes (the tree is the one the handle has); re-sending the rows a scene holds changes nothing.  Refusals are all
 * detected before anything is written and leave the scene untouched.  GNXR_ERR_INVALID: a null scene, a range outside the scene's
 * triangles, all three arrays NULL with n_triangles > 0, arrays on mixed sides or on another device.  GNXR_ERR_UNSUPPORTED: an array
 * whose table the scene was created without; a triangle whose own-attribute status would change -- it has attributes of its own when
 * its uvs differ in any bit from the defaults (0,0) (1,0) (1,1) or its normal or tangent row has any bit set, which selects its
 * material copy and shade class and is therefore topology (gnxr_scene_set_geometry changes it); a normal or tangent row with a bit
 * set on an emissive triangle (refused at creation as well).
 *
 * gnxr_scene_triangle_attributes (test hook): the rows the first device holds, in authoring order and unpadded; which = 0 uvs
 * (6 floats per triangle), 1 normals, 2 tangents (9).  *n_floats receives the size of the table (0: the scene has none); the rows
 * are written when out is not NULL and capacity_floats >= *n_floats.
 *
 * gnxr_scene_recompute_normals: shading normals from the vertices the scene holds now.  S = the triangles whose tri_n row has any
 * bit set when the call starts (the smooth triangles); the others take no part and are not written.  For t in S with corners p0, p1,
 * p2 (the positions the scene holds): a = p1 - p0, b = p2 - p0, F_t = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), each
 * product rounded, then the difference; F_t is not normalised, so faces weigh in by their area.  With GNXR_NORMALS_FLIP every
 * component of F_t is negated.  For a vertex index v, N_v = the sum of F_t over the corners of triangles in S that name v, starting
 * from +0, in ascending authoring triangle number and, within a triangle, ascending corner (a triangle that names v twice adds twice).
 * Triangles share a normal where they share a vertex INDEX; duplicated vertices make a crease.  For each corner of t in S, with N the
 * sum of its vertex: l2 = (N.x N.x + N.y N.y) + N.z N.z; if l2 is finite and > 0 the corner's normal becomes N / sqrt(l2) (three
 * divisions by the one rounded root), otherwise the corner keeps the normal it had.  So no row becomes zero and no triangle's
 * own-attribute status changes.  tri_s and tri_uv are not touched (the shading frame is orthogonalised against the normal at every
 * hit).  The vertex -> corner table behind N_v is built on the device at the first call and kept until gnxr_scene_set_geometry
 * replaces the mesh; gnxr_scene_rebuild_bvh leaves it valid.  Every device of the scene computes the same bits; the call returns when
 * all hold them.  GNXR_ERR_INVALID for a null scene or unknown flag bits; a scene without tri_n is a successful no-op.
 *
 * gnxr_skin_vertices_device: linear-blend skinning with blend shapes on device memory, no scene involved.  Per vertex v:
 * q = d_rest[v]; for m = 0 .. n_morphs - 1 in order, q = q + w_m * d_morph_delta[m][v] per component (w_m = d_morph_weight[m]; one
 * multiply, one add).  P = (0, 0, 0); for slot k = 0 .. 3 in order, with w = d_bone_weight[v][k]: a slot with w == 0 is skipped and its
 * index is not looked at; otherwise, with the row-major 3x4 matrix m of bone d_bone_index[v][k], T.x = ((m00 q.x + m01 q.y) + m02 q.z)
 * + m03 and likewise T.y, T.z, and P = P + w * T per component.  d_out[v] = P.  Weights are used as given (never normalised).  All
 * arrays are device memory of one device, validated as gnxr_temporal_accumulate_device validates its buffers; d_bone_index,
 * d_bone_weight and d_bones are 16-byte aligned (their rows are read whole), the others 4-byte; d_out overlaps no input;
 * d_morph_delta and d_morph_weight may be NULL when n_morphs == 0.  An index outside [0, n_bones) in a slot with a non-zero weight
 * is never dereferenced: the call returns GNXR_ERR_INVALID with the contents of d_out unspecified.  The work is queued on hip_stream;
 * the call waits for its status word only.  d_out can go straight into gnxr_scene_update_vertices. */
#define GNXR_NORMALS_FLIP 1u   /* flags of gnxr_scene_recompute_normals */
typedef struct gnxr_skin_params { int32_t struct_size, n_vertices, n_bones, n_morphs; } gnxr_skin_params;
int gnxr_scene_update_attributes(gnxr_scene *scene, int32_t first_triangle, int32_t n_triangles, const float *tri_uv, const float *tri_n,
                                 const float *tri_s, void *hip_stream);
int gnxr_scene_triangle_attributes(gnxr_scene *scene, int32_t which, float *out, int64_t capacity_floats, int64_t *n_floats);
int gnxr_scene_recompute_normals(gnxr_scene *scene, uint32_t flags, void *hip_stream);
int gnxr_skin_vertices_device(const gnxr_skin_params *params, const float *d_rest, const int32_t *d_bone_index, const float *d_bone_weight,
                              const float *d_bones, const float *d_morph_delta, const float *d_morph_weight, float *d_out, void *hip_stream);

/* -- Closest-point queries: which triangle is nearest to a point, where on it, and how far -------------------------------
 * The proximity counterpart of the ray queries: contact against a mesh gnxr_scene_update_vertices has just refitted, snapping probes
 * or texels off walls, projecting particles onto a surface.  The walk goes through the scene's live 4-wide tree (the binary tree
 * for scenes that are off it; same results), so after gnxr_scene_update_vertices[_ex], gnxr_scene_rebuild_bvh and
 * gnxr_scene_set_geometry the answer is for the geometry the scene holds now.  Spheres of the scene are NOT considered: triangles only.
 * The result is defined triangle by triangle, so it does not depend on the tree; every arithmetic step below is ONE rounded fp32
 * operation (nothing is contracted, divisions are correctly rounded), dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, min(x, y) =
 * (y < x ? y : x), max(x, y) = (y > x ? y : x), and a restatement in fp32 that follows the text reproduces the records bit for bit
 * (tests/closest_reference.py).
 *
 * Per triangle (a, b, c) -- its first, second and third vertex -- and query point q: the region walk of Ericson, Real-Time Collision
 * Detection 5.1.5 (ClosestPtPointTriangle), in its order.  ab = b - a, ac = c - a, ap = q - a, d1 = dot(ab, ap), d2 = dot(ac, ap).
 *   1. d1 <= 0 and d2 <= 0: p = a, (b1, b2) = (0, 0), feature 4.
 *   2. bp = q - b, d3 = dot(ab, bp), d4 = dot(ac, bp); d3 >= 0 and d4 <= d3: p = b, (1, 0), feature 5.
 *   3. vc = d1 d4 - d3 d2; vc <= 0, d1 >= 0 and d3 <= 0: v = d1 / (d1 - d3), p = a + v ab, (v, 0), feature 1.
 *   4. cp = q - c, d5 = dot(ab, cp), d6 = dot(ac, cp); d6 >= 0 and d5 <= d6: p = c, (0, 1), feature 6.
 *   5. vb = d5 d2 - d1 d6; vb <= 0, d2 >= 0 and d6 <= 0: w = d2 / (d2 - d6), p = a + w ac, (0, w), feature 2.
 *   6. va = d3 d6 - d5 d4; va <= 0, d4 - d3 >= 0 and d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), p = b + w (c - b),
 *      (1 - w, w), feature 3.
 *   7. otherwise denom = 1 / ((va + vb) + vc), v = vb denom, w = vc denom, p = (a + v ab) + w ac, (v, w), feature 0.
 * Every product of a scalar and a vector is rounded per component before the sum.  Then p is clamped componentwise into the triangle's
 * own bounding box: per axis lo = min(min(a, b), c), hi = max(max(a, b), c), p = (p < lo ? lo : (p > hi ? hi : p)) -- a NaN stays a NaN;
 * the clamp moves p by rounding error at most and makes every enclosing box's distance a lower bound of dist2 in fp32.
 * d = q - p, dist2 = dot(d, d).
 *
 * The winner.  r2 = max_distance * max_distance.  A triangle counts only if dist2 <= r2 (a NaN dist2 -- a zero-area triangle that reaches
 * step 7 -- never does).  The winner is the triangle of least dist2 and, among bit-equal dist2, of smallest authoring index (ties are the
 * normal case at shared vertices and edges).  A query with a NaN coordinate, a NaN max_distance or max_distance < 0 has no winner.
 * max_distance = +inf: unbounded.
 *
 * gnxr_closest_point: prim = the winner's authoring index (the numbering of gnxr_hit.prim), dist2, p, the barycentrics b1, b2 of p with
 * respect to the second and third vertex (b0 = 1 - b1 - b2 is the caller's to form), feature = 0 face, 1 / 2 / 3 edge ab / ac / bc,
 * 4 / 5 / 6 vertex a / b / c.  Without a winner prim = -1 and every other field is 0.
 *
 * gnxr_closest_point_device: the conventions of gnxr_trace_closest_device -- d_queries and d_out are device memory of one device that
 * holds a copy of the scene, both 16-byte aligned; the work is queued on hip_stream (NULL: the null stream) after what the caller queued
 * there, nothing is copied back and nothing waits for the GPU; scratch comes from the stream-ordered allocator on that stream -- the walk's stack
 * beyond its LDS levels (sized by the scene and the grid, never by n) and, from 65536 queries on, the arrays of a radix sort that bins
 * the queries by a coarse Morton key of p before the walk (at most 96 MB whatever n is; the order of the work changes, no result does)
 * --, so calls on several streams and a render in flight share no state; n == 0 is a no-op; GNXR_ERR_INVALID before anything is queued for a null scene, a null pointer with n > 0, n < 0, host
 * pointers, pointers on a device without a copy of the scene or on different devices, an array that runs past its allocation, or a
 * misaligned pointer.  The queries run on the device that holds the arrays.  gnxr_closest_point_counted_device is the same call through
 * the counting instantiation of the kernel (measurements only: slower): it ADDS the nodes visited and the triangles tested by the call
 * to d_counts[0], d_counts[1] (device memory, 8-byte aligned, the caller's to clear).  gnxr_closest_point takes host arrays: copy in,
 * the same walk, copy out; it returns when `out` is written.
 * The two records carry no struct_size and are not part of gnxr_abi_sizeof's list. */
typedef struct gnxr_point_query { float p[3]; float max_distance; } gnxr_point_query;   /* 16 bytes, 16-byte aligned on the device */
/* (the record shares its name with the host entry point, so it is a struct tag without a typedef: write `struct gnxr_closest_point`) */
struct gnxr_closest_point { int32_t prim; float dist2; float p[3]; float b1, b2; int32_t feature; };   /* 32 bytes */
int gnxr_closest_point_device(gnxr_scene *scene, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out,
                              void *hip_stream);
int gnxr_closest_point_counted_device(gnxr_scene *scene, const gnxr_point_query *d_queries, int64_t n, struct gnxr_closest_point *d_out,
                                      uint64_t *d_counts, void *hip_stream);
int gnxr_closest_point(gnxr_scene *scene, const gnxr_point_query *queries, int64_t n, struct gnxr_closest_point *out);

/* -- All-hits ray queries: EVERYTHING a ray passes through, counted and listed in order -----------------------------------
 * gnxr_trace_closest_device answers with the nearest hit of a ray, gnxr_trace_any_device with whether there is one.  This call answers
 * with all of them: thickness, transmission through stacked sheets, multi-return range scans, CSG classification -- and, through the
 * parity of the crossing count, whether a point lies inside a closed mesh, which with gnxr_closest_point is a signed distance.  The walk
 * goes through the scene's live 4-wide tree (the binary tree for scenes that are off it; same results), so after
 * gnxr_scene_update_vertices[_ex], gnxr_scene_rebuild_bvh and gnxr_scene_set_geometry the answer is for the geometry the scene holds
 * now.  Spheres of the scene are NOT considered: triangles only.
 *
 * The result is defined triangle by triangle, so it does not depend on the tree.  For a ray (o, d, tmax) and a triangle with vertices
 * p0, p1, p2 and authoring index prim, the triangle is a HIT iff both of these accept, each with the ray's own tmax (never a shrunk one):
 *   1. The own-box test.  Per axis lo = min(min(p0, p1), p2), hi = max(max(p0, p1), p2) with min(x, y) = (y < x ? y : x), max(x, y) =
 *      (y > x ? y : x) -- selection, no arithmetic.  Then Bounds3::IntersectP(ray, invDir, dirIsNeg) of the reference on [lo, hi] in its
 *      comparison sequence: invDir = 1 / d per component, dirIsNeg = invDir < 0; per axis tNear = (near - o) * invDir, tFar = (far - o)
 *      * invDir with near / far the bound dirIsNeg selects; tFar *= k, k = 1 + 2 * gamma(3), gamma(n) = (n * 2^-24) / (1 - n * 2^-24)
 *      in fp32; reject if tMin > tyMax or tyMin > tMax; if (tyMin > tMin) tMin = tyMin; if (tyMax < tMax) tMax = tyMax; the same with z;
 *      accept iff tMin < tmax and tMax > 0.  Every step is one rounded fp32 operation.
 *   2. The triangle test: the ray-space part of the reference's watertight Triangle::Intersect (translate by o, permute so that |d| is
 *      largest in z, shear, the three edge functions -- recomputed in fp64 when one of them is exactly 0 --, the sign test, det,
 *      tScaled against 0 and tmax * det, then t = tScaled / det against the error bound deltaT).  t, b1 = e1 / det, b2 = e2 / det are
 *      that function's outputs: b1 and b2 weight the second and the third vertex, the convention of gnxr_closest_point.
 * The own-box test is part of the definition, not of the implementation: the slab arithmetic is monotone in the box, so a triangle
 * whose own box accepts has every enclosing box accepting, the tests inside the tree only choose the subtrees that are walked, and a
 * brute force over all triangles (tests/allhits_reference.py) reproduces the output byte for byte whatever tree the scene has
 * (DESIGN.md).  A one-triangle leaf of the reference's tree tests exactly this box; a leaf of several triangles tests a wider one, so a
 * hit that grazes the own box by an ulp and that gnxr_trace_closest_device reports through its leaf's wider box can in principle be
 * absent here.
 *
 * Invalid rays have no hits: a non-finite component of o or d, a NaN tmax, or d == (0, 0, 0).  tmax = +inf is valid; tmax <= 0 falls
 * out of the arithmetic as no hits.  Results for triangles with non-finite vertices are not defined (the call neither faults nor loops).
 * (A direction ALL of whose components are so small that 1 / d overflows -- |d| below 3e-39 -- is a valid ray for which the triangle test
 * can accept with a NaN t; the order of such hits is not defined.  Scale d.)
 *
 * There is NO pruning by distance: every triangle along the ray within tmax is visited, whatever max_hits is.  (A walk that stops at
 * the K nearest would need an fp32 bound between a box's slab entry and the watertight test's t; nobody has one.  K-nearest pruning is
 * out of scope.)  A caller who wants fewer hits bounds tmax.
 *
 * Output, per ray: d_counts[i] = the number of hits, all of them, never clamped to max_hits.  The first min(count, max_hits) hits in
 * ascending order of (t, prim) -- t compared as a float (it is always > 0), bit-equal t ordered by the smaller authoring index, so
 * coincident triangles are both kept -- as records d_hits[i * max_hits + j] = (t, prim, b1, b2); the slots from min(count, max_hits)
 * up to max_hits - 1 are written as (+inf, -1, 0, 0), so the whole output is defined and comparable on bytes.  max_hits == 0 is the
 * count-only form (d_hits must be NULL); max_hits is at most GNXR_ALL_HITS_MAX.  A scene without triangles gives counts of 0 and empty
 * slots.
 *
 * Containment.  For a CLOSED mesh a point p is inside iff the count along (p, dir, +inf) is odd, for any direction that crosses no
 * edge or vertex exactly; GNXR_CONTAINS_DIRECTION_X / _Y / _Z are (3, 2, 1) / sqrt(14) to within an ulp of fp32, a direction that is
 * parallel to no axis or diagonal plane (Scene.contains and Scene.signed_distance of the Python module use it).  A ray through a shared
 * edge EXACTLY can count one crossing twice; a caller who cannot accept that votes over several directions.
 *
 * gnxr_trace_all_device: the conventions of gnxr_trace_closest_device and gnxr_closest_point_device -- every array is device memory of
 * one device that holds a copy of the scene, d_rays and d_hits 16-byte aligned, d_counts 4-byte aligned; the work is queued on
 * hip_stream (NULL: the null stream) after what the caller queued there, nothing is copied back and nothing waits for the GPU; scratch
 * (the walk's stack beyond its LDS levels, sized by the scene and the grid, never by n) comes from the stream-ordered allocator on that
 * stream; n == 0 is a no-op; GNXR_ERR_INVALID before anything is queued for a null scene, a null pointer with n > 0, n < 0, max_hits
 * outside [0, GNXR_ALL_HITS_MAX], d_hits set with max_hits == 0 or missing with max_hits > 0, a misaligned pointer, host pointers,
 * pointers on a device without a copy of the scene or on different devices, or an array that runs past its allocation.
 * gnxr_trace_all_counted_device is the same call through the counting instantiation of the kernel (measurements only: slower): it ADDS
 * the nodes visited, the own-box tests and the triangle tests of the call to d_work[0 .. 3) (device memory, 8-byte aligned, the
 * caller's to clear).  gnxr_trace_all takes host arrays: copy in, the same walk, copy out; it returns when the arrays are written.
 * The record carries no struct_size and is not part of gnxr_abi_sizeof's list. */
#define GNXR_ALL_HITS_MAX 32
#define GNXR_CONTAINS_DIRECTION_X 0.8017837f
#define GNXR_CONTAINS_DIRECTION_Y 0.5345225f
#define GNXR_CONTAINS_DIRECTION_Z 0.26726124f
typedef struct gnxr_ray_hit { float t; int32_t prim; float b1, b2; } gnxr_ray_hit;   /* 16 bytes, 16-byte aligned on the device */
int gnxr_trace_all_device(gnxr_scene *scene, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits, int32_t *d_counts,
                          void *hip_stream);
int gnxr_trace_all_counted_device(gnxr_scene *scene, const gnxr_ray *d_rays, int64_t n, int32_t max_hits, gnxr_ray_hit *d_hits,
                                  int32_t *d_counts, uint64_t *d_work, void *hip_stream);
int gnxr_trace_all(gnxr_scene *scene, const gnxr_ray *rays, int64_t n, int32_t max_hits, gnxr_ray_hit *hits, int32_t *counts);

/* -- Neighbour queries: the triangles within a radius of a point, and the K nearest ------------------------------------------
 * gnxr_closest_point_device answers with the one nearest triangle.  This call answers with everything near a point: the contact
 * manifold against a mesh that has just been refitted, the k nearest faces for attribute transfer or a blended distance field, the
 * candidate set of a particle within its own radius.  The walk goes through the scene's live 4-wide tree (the binary tree for scenes
 * that are off it; same results), so after gnxr_scene_update_vertices[_ex], gnxr_scene_rebuild_bvh and gnxr_scene_set_geometry the
 * answer is for the geometry the scene holds now.  Spheres of the scene are NOT considered: triangles only.
 *
 * The result is defined triangle by triangle, so it does not depend on the tree, the split method, the binning of the queries, or on
 * K beyond the cut.  For a query (p, max_distance) and every triangle in authoring order:
 *   1. dist2 and the record (prim, dist2, p, b1, b2, feature) are exactly those of "Closest-point queries" above: the same region walk,
 *      the same clamp into the triangle's own bounds, the same single rounded fp32 operations, the same 32-byte gnxr_closest_point.
 *   2. r2 = max_distance * max_distance, one fp32 product.  The triangle is NEAR iff dist2 <= r2; a NaN dist2 (a zero-area triangle
 *      that reaches step 7) fails.
 *   3. The query is valid under the closest-point rule: a NaN coordinate, a NaN max_distance or max_distance < 0 gives no neighbours.
 *      max_distance = +inf is allowed; in the GNXR_NEAR_ALL mode every triangle with a dist2 that is not NaN is then near.
 *   4. The list of the query is its near triangles in ascending (dist2, prim): dist2 compared as a float, bit-equal dist2 ordered by
 *      the smaller authoring index, so coincident triangles are both kept.  The list is cut to its first max_near = K entries.
 *   5. Output: the records d_out[i * K + j], j < min(near triangles, K), in that order; the slots behind them are EMPTY: prim = -1,
 *      dist2 = +inf and every other field 0, so the whole output is defined and comparable on bytes.  (gnxr_closest_point's record
 *      without a winner has dist2 = 0; an empty slot here has +inf, so that a row of dist2 is ascending through its empty slots.)
 * A brute force over all triangles that follows this text (tests/near_reference.py) reproduces records and counts byte for byte.
 *
 * Two modes share the flag word; any other bit is refused.
 *   GNXR_NEAR_ALL (0)      d_counts[i] = the number of ALL near triangles, never clamped to K.  K in [0, GNXR_NEAR_MAX]; K == 0 is the
 *                          count-only form (d_out must be NULL).  The walk drops a box iff its distance bd2 > r2, a fixed bound, so its
 *                          cost follows the radius, not K.
 *   GNXR_NEAR_NEAREST (1)  the list is the same, byte for byte, as GNXR_NEAR_ALL gives for the same query and K; d_counts[i] = the
 *                          number of slots filled, min(count of GNXR_NEAR_ALL, K).  K in [1, GNXR_NEAR_MAX].  Once the list is full the
 *                          bound becomes the K-th key: a box is dropped iff bd2 > the K-th dist2, and a box with bd2 == the K-th dist2
 *                          is entered, because a smaller authoring index may tie.  bd2 is a lower bound in fp32 of the dist2 of every
 *                          triangle under the box and the K-th key only shrinks, so nothing that belongs to the first K is dropped
 *                          (DESIGN.md); no epsilon anywhere.  With K == 1 the one record equals gnxr_closest_point's wherever that has
 *                          a winner.
 * A scene without triangles gives counts of 0 and empty slots.
 *
 * gnxr_near_device: the conventions of gnxr_closest_point_device and gnxr_trace_all_device -- every array is device memory of one
 * device that holds a copy of the scene, d_queries and d_out 16-byte aligned, d_counts 4-byte aligned; the work is queued on hip_stream
 * (NULL: the null stream) after what the caller queued there, nothing is copied back and nothing waits for the GPU; scratch comes from
 * the stream-ordered allocator on that stream -- the walk's stack beyond its LDS levels (sized by the scene and the grid, never by n)
 * and, from 65536 queries on, the arrays of the radix sort that bins the queries by a coarse Morton key of p before the walk, the one
 * of gnxr_closest_point_device (at most 96 MB whatever n is; the order of the work changes, no result does); n == 0 is a no-op;
 * GNXR_ERR_INVALID with a message, before anything is queued and with the scene untouched, for a null scene, a null pointer with
 * n > 0, n < 0, max_near out of range for the mode, d_out set with max_near == 0 or missing with max_near > 0, unknown flag bits, a
 * misaligned pointer, host pointers, pointers on a device without a copy of the scene or on different devices, or an array that runs
 * past its allocation.  While a query is walked its row of d_out is the walk's own working list; it holds the result when the call's
 * work on the stream is done.  gnxr_near_counted_device is the same call through the counting instantiation of the kernel
 * (measurements only: slower): it ADDS the nodes visited and the triangles tested by the call to d_work[0], d_work[1] (device memory,
 * 8-byte aligned, the caller's to clear).  gnxr_near takes host arrays: copy in, the same walk, copy out; it returns when the arrays
 * are written.  The calls add no struct: the records are gnxr_point_query and gnxr_closest_point. */
#define GNXR_NEAR_MAX 32
#define GNXR_NEAR_ALL 0u
#define GNXR_NEAR_NEAREST 1u
int gnxr_near_device(gnxr_scene *scene, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags,
                     struct gnxr_closest_point *d_out, int32_t *d_counts, void *hip_stream);
int gnxr_near_counted_device(gnxr_scene *scene, const gnxr_point_query *d_queries, int64_t n, int32_t max_near, uint32_t flags,
                             struct gnxr_closest_point *d_out, int32_t *d_counts, uint64_t *d_work, void *hip_stream);
int gnxr_near(gnxr_scene *scene, const gnxr_point_query *queries, int64_t n, int32_t max_near, uint32_t flags,
              struct gnxr_closest_point *out, int32_t *counts);

/* -- Sphere casts: the first impact of a moving ball ---------------------------------------------------------------------
 * The swept query beside the ray, overlap and closest-point calls: a ball of radius r whose centre is o + t d for t in [0, tmax]; when
 * does it first touch the mesh, and on which triangle.  A particle with a radius, the end caps of a character capsule, a camera boom, a
 * probe that must keep clearance.  (A ray along the centre line misses what the ball's rim touches first; stepping
 * gnxr_closest_point_device along the path tunnels through thin geometry and costs a launch per step.)  The walk goes through the
 * scene's live 4-wide tree (the binary tree for scenes that are off it; same results), so after gnxr_scene_update_vertices[_ex],
 * gnxr_scene_rebuild_bvh and gnxr_scene_set_geometry the answer is for the geometry the scene holds now.  Spheres of the scene are NOT
 * considered: triangles only.  d is not normalised and t is in units of d; tmax = +inf: unbounded; radius = 0 is allowed (nothing
 * promises that it equals gnxr_trace_closest_device).
 *
 * The result is defined triangle by triangle, so it does not depend on the tree.  The conventions are those of "Closest-point queries":
 * every arithmetic step is ONE rounded fp32 operation (nothing is contracted, divisions and square roots are correctly rounded),
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, min(x, y) = (y < x ? y : x), max(x, y) = (y > x ? y : x), a product of a scalar and a
 * vector is rounded per component before a sum, closest(q) is that section's steps 1-7 with the clamp, giving (dist2, p, b1, b2,
 * feature).  A restatement in fp32 that follows the text reproduces the records bit for bit (tests/spherecast_reference.py).
 *
 * Per cast (o, r, d, tmax):
 *   0. The cast is INVALID -- no triangle hits -- if o, d, r or tmax holds a NaN, r < 0 or tmax < 0; a cast with an infinite component
 *      of o or d hits nothing either.  r = +inf and tmax = +inf are allowed.  r2 = r r, dd = dot(d, d), inv = 1 / d per axis.  An axis
 *      whose inv is not finite (d is zero or so small that 1 / d overflows) is STATIC, the others MOVE.
 * Per triangle (a, b, c), in authoring order:
 *   1. The grown-box test.  lo = min(min(a, b), c), hi = max(max(a, b), c) per axis; glo = lo - r, ghi = hi + r.  A static axis k
 *      passes iff glo_k <= o_k <= ghi_k, and gives no time.  A moving axis k has near_k = (inv_k < 0 ? ghi_k : glo_k), far_k the
 *      other one, entry_k = (near_k - o_k) inv_k, exit_k = (far_k - o_k) inv_k.  tb = max over {0, entry_k of the moving axes},
 *      tx = min over {+inf, exit_k of the moving axes}.  The test passes iff every static axis passes, tb <= tx and tb <= tmax.
 *      (tx is not widened: step 3 makes that unnecessary.  With o and d finite no operand is a NaN and inv is never 0, so
 *      0 * inf does not occur; a static axis is never multiplied.)
 *   2. The analytic time ta, the smallest of the following; a candidate t counts iff 0 <= t < +inf (a NaN fails).
 *      start     closest(o).dist2 <= r2: ta = 0 (the ball starts in contact), and nothing else is looked at.
 *      face      ab = b - a, ac = c - a, n = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z, ab.x ac.y - ab.y ac.x), nn = dot(n, n).
 *                Only if nn > 0 (a degenerate triangle has no face term): len = sqrt(nn), sd = dot(n, o - a), dn = dot(n, d),
 *                h = r len, tf = ((sd < 0 ? -h : h) - sd) / dn -- the plane offset by r towards o.  tf counts iff
 *                closest(o + tf d).feature == 0.
 *      edges     (p0, p1) = (a, b), (a, c), (b, c): e = p1 - p0, m = o - p0, me = dot(m, e), de = dot(d, e), ee = dot(e, e),
 *                md = dot(m, d), mm = dot(m, m); A = ee dd - de de, C = ee (mm - r2) - me me, B = ee md - de me, disc = B B - A C.
 *                Only if A > 0 and disc >= 0: t = (-B - sqrt(disc)) / A, w = me + t de; t counts iff 0 <= w <= ee (the axial
 *                parameter w / ee within [0, 1]).
 *      vertices  v = a, b, c: m = o - v, bq = dot(m, d), cq = dot(m, m) - r2, disc = bq bq - dd cq.  Only if dd > 0 and disc >= 0:
 *                t = (-bq - sqrt(disc)) / dd.
 *      Only entering roots are taken: a ball that starts inside a cylinder or a sphere and is not in contact at t = 0 meets the
 *      triangle through another term first.  Ties between the terms need no rule (the record comes from closest()).
 *   3. t = max(tb, ta) = (ta > tb ? ta : tb).  The triangle HITS iff step 1 passed, ta exists (ta < +inf) and t <= tmax.
 * The winner is the triangle of least t and, among bit-equal t, of smallest authoring index.  Step 3 is what lets a walk through any
 * tree prune with no epsilon: tb of every box that encloses the triangle's own box is <= tb of the own box <= t in fp32.
 *
 * The answer is a gnxr_closest_point record with the dist2 slot holding t: prim = the winner's authoring index, dist2 = t, and
 * (p, b1, b2, feature) = closest(o + t d) of the winner -- the contact point; the contact normal is (o + t d - p) / r.  Without a hit,
 * and for an invalid cast: prim = -1, t = +inf, every other field 0.
 *
 * gnxr_sphere_cast_device: the conventions of gnxr_closest_point_device -- d_casts and d_out are device memory of one device that
 * holds a copy of the scene, both 16-byte aligned; the work is queued on hip_stream (NULL: the null stream) after what the caller
 * queued there, nothing is copied back and nothing waits for the GPU; scratch (the walk's stack beyond its LDS levels, sized by the
 * scene and the grid, never by n) comes from the stream-ordered allocator on that stream; casts are walked in caller order (no
 * binning); n == 0 is a no-op; GNXR_ERR_INVALID before anything is queued for a null scene, a null pointer with n > 0, n < 0, host
 * pointers, pointers on a device without a copy of the scene or on different devices, an array that runs past its allocation, or a
 * misaligned pointer.  gnxr_sphere_cast_counted_device is the same call through the counting instantiation of the kernel
 * (measurements only: slower): it ADDS the nodes visited and the triangles taken to step 2 by the call to d_work[0], d_work[1]
 * (device memory, 8-byte aligned, the caller's to clear).  gnxr_sphere_cast takes host arrays: copy in, the same walk, copy out; it
 * returns when `out` is written.  The record carries no struct_size and is not part of gnxr_abi_sizeof's list. */
/* (the record shares its name with the host entry point, so it is a struct tag without a typedef: write `struct gnxr_sphere_cast`) */
struct gnxr_sphere_cast { float o[3]; float radius; float d[3]; float tmax; };   /* 32 bytes, 16-byte aligned on the device */
int gnxr_sphere_cast_device(gnxr_scene *scene, const struct gnxr_sphere_cast *d_casts, int64_t n, struct gnxr_closest_point *d_out,
                            void *hip_stream);
int gnxr_sphere_cast_counted_device(gnxr_scene *scene, const struct gnxr_sphere_cast *d_casts, int64_t n,
                                    struct gnxr_closest_point *d_out, uint64_t *d_work, void *hip_stream);
int gnxr_sphere_cast(gnxr_scene *scene, const struct gnxr_sphere_cast *casts, int64_t n, struct gnxr_closest_point *out);

/* -- Overlap queries: the triangles an axis-aligned box touches ------------------------------------------------------------
 * The volume query beside the ray, point and swept-sphere calls: which triangles touch this box.  Broad-phase collision against a mesh
 * that has just been refitted, region selection, trigger volumes, an occupancy or navigation grid (a voxel grid is many boxes), the
 * triangles to re-bake after an edit.  (gnxr_near_device with the box's half diagonal answers with a superset that grows with the
 * box's aspect ratio.)  The walk goes through the scene's live 4-wide tree (the binary tree for scenes that are off it; same results),
 * so after gnxr_scene_update_vertices[_ex], gnxr_scene_rebuild_bvh and gnxr_scene_set_geometry the answer is for the geometry the
 * scene holds now.  Spheres of the scene are NOT considered: triangles only.
 *
 * A query is a gnxr_box_query (lo, hi); the two pad words are ignored.  The result is defined triangle by triangle, so it does not
 * depend on the tree.  Every arithmetic step is ONE rounded fp32 operation (nothing is contracted), min(x, y) = (y < x ? y : x),
 * max(x, y) = (y > x ? y : x), dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z.  Per box:
 *   1. Box validity.  If any lo[k] <= hi[k] is false (a NaN bound fails the comparison) or any of the six bounds is not finite, NOTHING
 *      overlaps: the count is 0 and the list is empty.  lo == hi, a point, is a valid box.  (A caller who wants "everything" passes
 *      the scene's bounds.)
 *      Of a valid box: ctr[k] = 0.5 lo[k] + 0.5 hi[k] and h[k] = 0.5 hi[k] - 0.5 lo[k]: two products, then one sum / one difference.
 * Per triangle (a, b, c), the vertices the scene holds, in authoring order:
 *   2. Bounds test.  tlo = min(min(a, b), c), thi = max(max(a, b), c) per axis: selections, no arithmetic.  The triangle passes iff
 *      tlo[k] <= hi[k] && thi[k] >= lo[k] on every axis k -- closed: touching counts.  This is also the ONLY test a tree applies to a
 *      node's box: a node's box is the min / max of the vertices under it, so a triangle that passes has every enclosing node passing,
 *      and a walk prunes on plain comparisons with no epsilon.
 *   3. ua = a - ctr, ub = b - ctr, uc = c - ctr per component; e0 = ub - ua, e1 = uc - ub, e2 = ua - uc (of the rounded u).
 *   4. Nine edge axes (Akenine-Moller's triangle-box test).  For the edges in the order e0, e1, e2, each with its pair of vertices of
 *      distinct projections (p, q) = (ua, uc), (ub, ua), (uc, ub) -- the edge's first vertex and the vertex off the edge --, and for the
 *      box axes in the order x, y, z with (i, j) = (y, z), (z, x), (x, y):
 *          p0 = e[i] p[j] - e[j] p[i],   p1 = e[i] q[j] - e[j] q[i]      (two products and a difference each)
 *          r  = h[i] |e[j]| + h[j] |e[i]|                                  (two products and a sum)
 *      the axis SEPARATES iff min(p0, p1) > r || max(p0, p1) < -r.
 *   5. Plane test.  n = (e0.y e1.z - e0.z e1.y, e0.z e1.x - e0.x e1.z, e0.x e1.y - e0.y e1.x).  Per axis k: below = (-h[k]) - ua[k],
 *      above = h[k] - ua[k]; vmin[k] = (n[k] > 0 ? below : above), vmax[k] = (n[k] > 0 ? above : below).  The plane SEPARATES iff
 *      dot(n, vmin) > 0 || !(dot(n, vmax) >= 0).
 * The triangle OVERLAPS iff step 2 passes and neither step 4 nor step 5 separates.  Step 2 stands in for the original's three box-axis
 * tests, which would round.  Steps 4 and 5 round: a triangle and a box that only just touch, or only just miss, may fall on either
 * side, within a few ulps of the scene's size (DESIGN.md has the measured float64 margin); the answer is the same on every tree,
 * every device and in the restatement.  A zero-area triangle has n = 0 and is decided by steps 2 and 4.  A brute force over all
 * triangles in numpy float32 that follows this text (tests/overlap_reference.py) reproduces lists and counts byte for byte.
 *
 * The list of a box is the authoring indices (gnxr_hit.prim) of its overlapping triangles, ASCENDING, cut to the capacity of its row:
 * a row shorter than the count holds the smallest indices; the slots behind the list hold -1; d_counts[i] is the number of ALL
 * overlapping triangles, never clamped.  Two row layouts:
 *   rows mode (d_offsets == NULL)  row i is d_prims[i K .. (i + 1) K), K = max_prims in [0, GNXR_OVERLAP_MAX].  K == 0 is the
 *                                  count-only form and requires d_prims == NULL.
 *   CSR mode (d_offsets given)     n + 1 ascending int64 values on the device, 8-byte aligned; row i is
 *                                  d_prims[d_offsets[i] .. d_offsets[i + 1]) and its capacity is that difference (not limited by
 *                                  GNXR_OVERLAP_MAX; 0 when the two are out of order).  max_prims must be -1 and d_prims must be
 *                                  given.  The usual sequence is a count-only call, an exclusive prefix sum of the counts, one
 *                                  allocation, and this call.  Nothing outside a row is ever written, so offsets that are stale
 *                                  for the geometry cut or pad rows and corrupt nothing; the offsets themselves are the caller's
 *                                  word for where d_prims may be written.
 * While a box is walked its row is the walk's own working list (insertion: a row of length L costs up to L^2 / 2 dword moves); it
 * holds the result when the call's work on the stream is done.
 *
 * gnxr_overlap_box_device: the conventions of gnxr_trace_all_device -- every array is device memory of one device that holds a copy
 * of the scene, d_boxes 16-byte aligned, d_offsets 8-byte, d_prims and d_counts 4-byte aligned; the work is queued on hip_stream
 * (NULL: the null stream) after what the caller queued there, nothing is copied back and nothing waits for the GPU; scratch (the
 * walk's stack beyond its LDS levels, sized by the scene and the grid, never by n) comes from the stream-ordered allocator on that
 * stream; boxes are walked in caller order (no binning); n == 0 is a no-op; GNXR_ERR_INVALID with a message, before anything is queued
 * and with the scene untouched, for a null scene, a null pointer with n > 0, n < 0, max_prims outside [0, GNXR_OVERLAP_MAX] in rows
 * mode, d_prims set with max_prims == 0 or missing with max_prims > 0, max_prims != -1 together with d_offsets or -1 without them, a
 * misaligned pointer, host pointers, pointers on a device without a copy of the scene or on different devices, or an array that runs
 * past its allocation (the extent of CSR rows lives on the device and is not looked at).  gnxr_overlap_box_counted_device is the same
 * call through the counting instantiation of the kernel (measurements only: slower): it ADDS the nodes visited and the triangles
 * taken to step 2 by the call to d_work[0], d_work[1] (device memory, 8-byte aligned, the caller's to clear).  gnxr_overlap_box
 * takes host arrays: copy in, the same walk, copy out; it returns when the arrays are written, and, since it can read them, refuses
 * offsets that are negative or do not ascend.  The record carries no struct_size and is not part of gnxr_abi_sizeof's list. */
#define GNXR_OVERLAP_MAX 32
typedef struct gnxr_box_query { float lo[3]; float pad0; float hi[3]; float pad1; } gnxr_box_query;   /* 32 bytes, 16-byte aligned on the device */
int gnxr_overlap_box_device(gnxr_scene *scene, const gnxr_box_query *d_boxes, int64_t n, int32_t max_prims, const int64_t *d_offsets,
                            int32_t *d_prims, int32_t *d_counts, void *hip_stream);
int gnxr_overlap_box_counted_device(gnxr_scene *scene, const gnxr_box_query *d_boxes, int64_t n, int32_t max_prims,
                                    const int64_t *d_offsets, int32_t *d_prims, int32_t *d_counts, uint64_t *d_work, void *hip_stream);
int gnxr_overlap_box(gnxr_scene *scene, const gnxr_box_query *boxes, int64_t n, int32_t max_prims, const int64_t *offsets,
                     int32_t *prims, int32_t *counts);

/* -- Triangle overlap queries: the triangles another triangle touches, and a mesh against itself ----------------------------
 * The exact test beside the box query: which triangles of the scene touch this triangle.  Mesh against mesh -- a tool, a garment, a
 * second character, a prop: one query per foreign triangle -- and, with the scene's own triangles as the queries, self-intersection:
 * did this pose fold the mesh through itself?  (gnxr_overlap_box_device on a foreign triangle's bounds answers with a superset, which
 * for a thin or diagonal triangle is most of what it returns.)  The walk, the live tree and the spheres are as for the box queries.
 *
 * A query is a gnxr_tri_query (a, b, c); the three pad words are ignored.  The result is defined triangle by triangle, so it does not
 * depend on the tree.  The conventions are the box section's: every arithmetic step is ONE rounded fp32 operation (nothing is
 * contracted), min(x, y) = (y < x ? y : x), max(x, y) = (y > x ? y : x), of three values min(min(x, y), z) and max(max(x, y), z) in the
 * order they are written below, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, u - v per component, and
 * cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x): two products and a difference per component.
 * Per query (qa, qb, qc):
 *   1. Validity.  If any of the nine coordinates is not finite, NOTHING overlaps: the count is 0 and the list is empty.  Every finite
 *      triangle is valid, zero-area ones included: a segment or a point is a legitimate query.
 *      Of a valid query: qlo = min(min(qa, qb), qc), qhi = max(max(qa, qb), qc) per axis (selections); ub = qb - qa, uc = qc - qa;
 *      f0 = ub, f1 = uc - ub, f2 = uc; nq = cross(ub, uc).
 * Per triangle (a, b, c), the vertices the scene holds, in authoring order:
 *   2. Bounds test.  Step 2 of the box queries against the box [qlo, qhi]: tlo = min(min(a, b), c), thi = max(max(a, b), c) per axis,
 *      and the triangle passes iff tlo[k] <= qhi[k] && thi[k] >= qlo[k] on every axis k -- closed, comparisons only.  This is the ONLY
 *      test a tree applies to a node's box, so a walk visits exactly the nodes gnxr_overlap_box_device visits for the box [qlo, qhi]
 *      and prunes with no epsilon.
 *   3. Shared vertices (only with GNXR_OVERLAP_TRI_SKIP_SHARED).  If any of the nine pairs (query vertex, triangle vertex) compares
 *      equal with == on all three coordinates (-0 == +0; a NaN equals nothing), the triangle is SKIPPED: neither counted nor listed.
 *      With the scene's own triangles as the queries this leaves out the triangle itself and its edge and vertex neighbours, which
 *      touch by construction: what remains is self-intersection.  The rule looks at positions only, so the duplicated vertices of a
 *      crease or a texture seam count as shared.
 *   4. Translate.  ta = a - qa, tb = b - qa, tc = c - qa; e0 = tb - ta, e1 = tc - tb, e2 = ta - tc (of the rounded t);
 *      nt = cross(e0, e1).
 *   5. Seventeen separating axes L: nq; nt; cross(f_i, e_j) for i, j in 0..2; cross(nq, f_i) for i in 0..2; cross(nt, e_j) for j in
 *      0..2 -- the last two groups are the in-plane axes that decide coplanar pairs.  On an axis, with the query's vertices at 0, ub,
 *      uc after the translation:
 *          qmin = min(min(0, dot(L, ub)), dot(L, uc)),          qmax = max(max(0, dot(L, ub)), dot(L, uc))
 *          tmin = min(min(dot(L, ta), dot(L, tb)), dot(L, tc)),  tmax = max(max(dot(L, ta), dot(L, tb)), dot(L, tc))
 *      and the axis SEPARATES iff tmin > qmax || tmax < qmin -- closed: touching counts.  A zero axis (a zero-area triangle, parallel
 *      edges) gives two intervals [0, 0] and never separates.  Where an axis overflows to NaN (inf - inf) the comparisons are false
 *      and it does not separate: the answer is then conservative, and still the same bits everywhere.
 * The triangle OVERLAPS iff step 2 passes, step 3 does not skip it and no axis of step 5 separates.  The axes are independent of each
 * other: an implementation may evaluate them in any order, stop at the first that separates, and compute what depends on the query
 * alone (nq, the three cross(nq, f_i), the query's intervals on those four) once per query; the bits do not change.
 * Limits.  (i) The translation is by the QUERY's first vertex, so at the rounding margin overlaps(Q, T) and overlaps(T, Q) may differ;
 * a caller who needs a symmetric relation ORs the two directions (as the pairs of a self-intersection call do).  (ii) Steps 4 and 5
 * round: a touching answer means "within a few ulps of the coordinates' size", as for boxes (DESIGN.md has the measured float64
 * margin).  (iii) A zero-area triangle has no normal and so no in-plane axes of its own: a segment lying in the plane of a triangle
 * it passes beside can be reported (conservative).  A brute force over all triangles in numpy float32 that follows this text
 * (tests/overlap_tri_reference.py) reproduces lists and counts byte for byte.
 *
 * Lists, counts and row layouts are exactly gnxr_overlap_box_device's: authoring indices ASCENDING, cut to the capacity of the row, -1
 * behind the list, d_counts[i] never clamped; rows mode with max_prims in [0, GNXR_OVERLAP_MAX] (0: count only, d_prims NULL) or CSR
 * mode through d_offsets with max_prims == -1; nothing outside a row is written.
 *
 * flags: GNXR_OVERLAP_TRI_SKIP_SHARED applies step 3.  GNXR_OVERLAP_TRI_SELF: the queries are the scene's own triangles -- d_tris must
 * be NULL, n must equal the scene's triangle count, SKIP_SHARED is implied, query i is the triangle with authoring index i, and rows,
 * offsets and counts are indexed by authoring index.  (The kernel takes the triangles in the tree's leaf order, where neighbouring
 * lanes walk nearly the same path; other queries are walked in caller order.)
 *
 * gnxr_overlap_tri_device: the conventions, alignments and refusals of gnxr_overlap_box_device, with d_tris 16-byte aligned (three
 * 16-byte loads per record); in addition GNXR_ERR_INVALID with a message for an unknown flag bit, for SELF with a non-NULL d_tris and
 * for SELF with n other than the scene's triangle count.  gnxr_overlap_tri_counted_device ADDS nodes visited and triangles taken to
 * step 2 to d_work[0], d_work[1] (measurements only: slower).  gnxr_overlap_tri takes host arrays, as gnxr_overlap_box does.  The
 * record carries no struct_size and is not part of gnxr_abi_sizeof's list. */
#define GNXR_OVERLAP_TRI_SKIP_SHARED 1u
#define GNXR_OVERLAP_TRI_SELF        2u
typedef struct gnxr_tri_query { float a[3]; float pad0; float b[3]; float pad1; float c[3]; float pad2; } gnxr_tri_query;   /* 48 bytes, 16-byte aligned on the device */
int gnxr_overlap_tri_device(gnxr_scene *scene, const gnxr_tri_query *d_tris, int64_t n, uint32_t flags, int32_t max_prims,
                            const int64_t *d_offsets, int32_t *d_prims, int32_t *d_counts, void *hip_stream);
int gnxr_overlap_tri_counted_device(gnxr_scene *scene, const gnxr_tri_query *d_tris, int64_t n, uint32_t flags, int32_t max_prims,
                                    const int64_t *d_offsets, int32_t *d_prims, int32_t *d_counts, uint64_t *d_work, void *hip_stream);
int gnxr_overlap_tri(gnxr_scene *scene, const gnxr_tri_query *tris, int64_t n, uint32_t flags, int32_t max_prims, const int64_t *offsets,
                     int32_t *prims, int32_t *counts);

/* -- Shading queries on device memory: the pieces an integrator is made of, batched -------------------------------------
 * Same conventions as the device calls of the Aggregate seam: every array is device memory of one device that holds a copy of the
 * scene, the work is queued on hip_stream (NULL: the null stream) after what the caller queued there, scratch comes from the
 * stream-ordered allocator (bounded whatever n is: at most 128 MB), n == 0 is a no-op, and GNXR_ERR_INVALID comes back before anything is
 * queued for a null scene, a null pointer with n > 0, n < 0, host pointers, pointers on a device without a copy of the scene or
 * on different devices, or a misaligned pointer.
 *
 * gnxr_bsdf_device: per ray Scene::Intersect (d_rays[i]: o, d, tmax), ComputeScatteringFunctions(TransportMode::Radiance,
 * allowMultipleLobes = true) at the hit and, with wo = Normalize(-d) as SurfaceInteraction sets it: BSDF::f(wo, wi) and
 * BSDF::Pdf(wo, wi) for the world-space d_wi[3i..] and BSDF::Sample_f(wo, u) for d_u[2i..], all under the BxDFType mask `flags`
 * (BSDF_ALL = 31).  d_differentials: NULL (hasDifferentials == false: the unfiltered texture lookup PathIntegrator makes) or per
 * ray 12 floats rxOrigin, rxDirection, ryOrigin, ryDirection (they reach ImageTexture lookups of Kd / Ks and the dudx / dvdy of
 * the record).  d_rays and d_out 16-byte aligned, the float arrays 4-byte aligned.  The traversal is the one of
 * gnxr_trace_closest_device; the hit point, shading frame and BSDF are built by the functions the render's shade kernels use.
 * Returns without waiting for the GPU; may run beside a render of the same handle and beside other queries.
 *
 * gnxr_light_sample_device: d_queries holds 12 dwords per query (48 bytes, read as three 16-byte loads): p[3], the light (int32:
 * an index into the scene's lights), n[3], u[2], wi_query[3].  With ref = the Interaction at p with normal n and zero pError:
 * Light::Sample_Li(ref, u) of that light, Light::Pdf_Li(ref, wi_query) and the probability with which the LightDistribution of
 * `strategy` (gnxr_light_strategy) picks that light at p.  d_queries and d_out 16-byte aligned.  The selection table is the
 * render's (built on first use, shared with gnxr_render, gnxr_li_device and gnxr_light_grid_table), so the call holds the render
 * lock of the handle and of the copy it runs on: it takes its turn with renders and Li calls there.  A light index outside
 * [0, n_lights) gives a zero record, the other queries are finished and the call returns GNXR_ERR_INVALID naming the first such
 * query; that status has to come back, so every call waits for its own kernel (hip_stream is synchronised) before it returns.
 *
 * gnxr_light_le_device: Light::Le(ray) of light `light` for escaped rays (d_rays 16-byte aligned; d_le: 3 floats per ray, 4-byte
 * aligned); zero for lights without Le (everything but the infinite and the sky-box light).  GNXR_ERR_INVALID for a light index
 * outside [0, n_lights).                                                                                                        */
int gnxr_bsdf_device(gnxr_scene *scene, const gnxr_ray *d_rays, const float *d_wi, const float *d_u, const float *d_differentials, int64_t n,
                     int32_t flags, gnxr_bsdf_result *d_out, void *hip_stream);
int gnxr_light_sample_device(gnxr_scene *scene, const float *d_queries, int64_t n, int32_t strategy, gnxr_light_result *d_out, void *hip_stream);
int gnxr_light_le_device(gnxr_scene *scene, int32_t light, const gnxr_ray *d_rays, int64_t n, float *d_le, void *hip_stream);

/* -- sampler / camera probes (bit-exactness test hooks) --------------------------------- */
/* HaltonSampler(spp, [0,width)x[0,height)) value of dimension dim[i] for sample s[i] of pixel
 * (px[i],py[i]) -- GetIndexForSample + SampleDimension, HaltonSampler.cpp:63-94.            */
int gnxr_sample_halton(int32_t width, int32_t height, const int32_t *px, const int32_t *py,
                       const int64_t *s, const int32_t *dim, int64_t n, float *out);
/* Camera rays (Perspective.cpp:62-112 + Integrator.cpp:277-283): for sample s of pixel (px,py)
 * writes origin[3], direction[3] per ray.                                                    */
int gnxr_camera_rays(const gnxr_camera *cam, int32_t width, int32_t height, const int32_t *px,
                     const int32_t *py, const int64_t *s, int64_t n, float *o_out, float *d_out);

/* FrameBuffer::saveToFile (ui/FrameBuffer.cpp:6-9: stbi_write_png of the RGBA8 plane): writes `rgba8` (width * height * 4
 * bytes, row-major, as gnxr_framebuffer_update produces it) as an 8-bit RGBA PNG.  Host-only; the file decodes to the same
 * pixels as the reference's (the zlib stream itself is not stb's). */
int gnxr_framebuffer_save_png(const char *path, const uint8_t *rgba8, int32_t width, int32_t height);

/* Unit-test hook: the light-selection table of `strategy` (core/LightDistribution.cpp; per voxel cdf[1..n], func[0..n-1],
 * funcInt), built on the device (on_host == 0) or by the host restatement (on_host != 0).  *n_floats receives the table
 * size; the table is copied when `out` has room for it. */
int gnxr_light_grid_table(gnxr_scene *s, int32_t strategy, int32_t on_host, float *out, int64_t capacity, int64_t *n_floats);

/* Unit-test hook: the device's float libm on caller-supplied arguments.  fn: 0 logf, 1 expf, 2 sinf, 3 cosf, 4 / 5 sinf / cosf
 * through the shared-reduction pair evaluation, 6 acosf, 7 atan2f(x, x2), 8 powf(x, x2) (x2 may be NULL otherwise).  The
 * reference reaches these through std::log / std::exp / std::sin / std::cos on floats (core/Sampling.cpp:87-105,
 * media/GridDensityMedium.cpp:41,67, media/HomogeneousMedium.cpp:13,24, core/Medium.cpp:187, core/Geometry.h:1436-1443);
 * the device restates glibc 2.35's algorithms so the results carry glibc's bits. */
int gnxr_eval_libm(int32_t fn, const float *x, const float *x2, int64_t n, float *out);
/* The double-precision libm calls of the path, on float arguments widened to double, results as doubles.  fn: 0 sin, 1 cos (the pair
 * the device evaluates for `r * cos(phi)`, `r * sin(phi)` at core/MicroFacet.cpp:220-223, where the unqualified calls bind to the
 * double versions), 2 sqrt (MicroFacet.cpp:220, DisneyMaterial.cpp:236), 3 tan (MicroFacet.cpp:190-191, 297). */
int gnxr_eval_libm_f64(int32_t fn, const float *x, int64_t n, double *out);

/* -- output stage (FrameBuffer::update_f_u_c, ui/FrameBuffer.h:127-149) ------------------ */
/* Folds one Render() result into the running mean of `frame_count` previous frames and
 * tone-maps 1-exp(-x/0.25) to RGBA8 (A=255).  Device-side; host pointers in and out.        */
int gnxr_framebuffer_update(float *running_mean_rgba, const float *frame_rgba, int32_t width,
                            int32_t height, int32_t frame_count, uint8_t *rgba8_out);

/* -- host-side scene authoring (mirror of ui/ModelList.cpp, ui/MaterialList.cpp) -------- */
typedef struct gnxr_builder gnxr_builder;
int gnxr_builder_create(gnxr_builder **out);
void gnxr_builder_destroy(gnxr_builder *b);
/* material factories return a material index */
int gnxr_builder_add_material(gnxr_builder *b, const gnxr_material *m);
int gnxr_builder_matte(gnxr_builder *b, const float kd[3], float sigma_deg);          /* RenderThread.cpp:79-99 */
int gnxr_builder_mirror(gnxr_builder *b, const float kr[3]);                          /* RenderThread.cpp:102   */
int gnxr_builder_purple_plastic(gnxr_builder *b);                                     /* MaterialList.cpp:48-56 */
int gnxr_builder_yellow_metal(gnxr_builder *b);                                       /* MaterialList.cpp:58-69 */
int gnxr_builder_white_glass(gnxr_builder *b);                                        /* MaterialList.cpp:71-83 */
/* geometry: each returns the index of the first triangle added, or <0 */
int gnxr_builder_add_mesh(gnxr_builder *b, const float *vertices, int32_t n_vertices,
                          const int32_t *indices, int32_t n_triangles, const float *object_to_world16,
                          int32_t material, int32_t medium_inside, int32_t medium_outside);
int gnxr_builder_add_model_3d(gnxr_builder *b, const char *path, int32_t material);   /* ModelList.cpp:47-69, plyRead.h:19-48 */
int gnxr_builder_add_cornell(gnxr_builder *b, int32_t material1, int32_t material2,
                             int32_t material3);                                      /* ModelList.cpp:71-118 */
int gnxr_builder_add_floor(gnxr_builder *b, int32_t material);                        /* ModelList.cpp:20-45  */
int gnxr_builder_add_area_light(gnxr_builder *b, int32_t material);                   /* ModelList.cpp:120-147 */
/* AddAreaLight's pattern for any mesh: one DiffuseAreaLight(Lemit, nSamples, triangle, twoSided = false) per triangle
 * (ModelList.cpp:137-146); returns the first triangle index */
int gnxr_builder_add_emissive_mesh(gnxr_builder *b, const float *vertices, int32_t n_vertices, const int32_t *indices, int32_t n_triangles,
                                   const float *object_to_world16, int32_t material, const float lemit[3], int32_t n_samples);
int gnxr_builder_add_sky_light(gnxr_builder *b);                                      /* ModelList.cpp:163-170 */
int gnxr_builder_add_spot_light(gnxr_builder *b);                                     /* AddSpotLight, ModelList.cpp:149-154 */
int gnxr_builder_add_dist_light(gnxr_builder *b);                                     /* AddDistLight, ModelList.cpp:156-161 */
int gnxr_builder_add_light(gnxr_builder *b, const gnxr_light *l);                     /* POINT / SPOT / DISTANT with caller-chosen parameters */
int gnxr_builder_add_inf_light(gnxr_builder *b, const char *hdr_path);                /* ModelList.cpp:172-179 */
int gnxr_builder_add_inf_light_data(gnxr_builder *b, const float *rgb, int32_t w, int32_t h,
                                    const float *light_to_world16, const float power[3]);
int gnxr_builder_add_medium(gnxr_builder *b, const gnxr_medium *m, const float *density);
/* GridDensityMedium from a `.volume` text file (the format of the reference's Resources/density_render.70.volume: `nx N ny N nz N`,
 * `p0 x y z`, `p1 x y z`, `sigma_a r g b`, `sigma_s r g b`, then nx*ny*nz densities): sigma_a / sigma_s of the header times
 * sigma_scale, Henyey-Greenstein g, MediumToWorld = medium_to_world16 or, when NULL, Translate(p0) * Scale(p1 - p0) of the header.
 * The reference ships the file but no reader for it, so the file semantics (x fastest, the p0 / p1 placement) are THIS project's
 * definition -- parity unpinned for the loader, pinned for the medium it builds.  Each dimension <= 4096, at most 2^31 - 1 values;
 * GNXR_ERR_IO for a malformed file, GNXR_ERR_OOM when the values do not fit in memory.  Returns the medium index.                  */
int gnxr_builder_add_volume_file(gnxr_builder *b, const char *path, float g, float sigma_scale, const float *medium_to_world16);
/* ImageTexture: `t` carries the mapping / filter parameters (width, height, texel_offset are filled in); returns the texture
 * index.  _file decodes a Radiance .hdr like stbi_loadf; other formats (the reference's awesomeface.jpg) must be decoded by the
 * caller and passed as texels. */
int gnxr_builder_add_texture_data(gnxr_builder *b, const gnxr_texture *t, const float *rgb, int32_t w, int32_t h);
int gnxr_builder_add_texture_file(gnxr_builder *b, const gnxr_texture *t, const char *hdr_path);
int gnxr_builder_set_material_texture(gnxr_builder *b, int32_t material, int32_t slot /* 0 Kd, 1 Ks */, int32_t texture);
/* per-corner (u,v) of triangles [first_triangle, first_triangle + n_triangles): tri_uv holds n_triangles * 6 floats */
int gnxr_builder_set_triangle_uv(gnxr_builder *b, int32_t first_triangle, int32_t n_triangles, const float *tri_uv);
/* per-corner WORLD-space shading normals (n_triangles * 9 floats); a caller with object-space normals applies the mesh's
 * ObjectToWorld as TriangleMesh's constructor does (Transform::operator()(Normal3f): the inverse transpose) */
int gnxr_builder_set_triangle_normals(gnxr_builder *b, int32_t first_triangle, int32_t n_triangles, const float *tri_n);
int gnxr_builder_set_triangle_tangents(gnxr_builder *b, int32_t first_triangle, int32_t n_triangles, const float *tri_s);   /* TriangleMesh::s, world space */
int gnxr_builder_add_sphere(gnxr_builder *b, const float center[3], float radius, int32_t material, int32_t medium_inside,
                            int32_t medium_outside);                                      /* returns the sphere index */
int gnxr_builder_set_camera(gnxr_builder *b, const gnxr_camera *cam);
int gnxr_builder_set_bvh_split_method(gnxr_builder *b, int32_t method);               /* gnxr_bvh_split_method */
int gnxr_builder_set_camera_medium(gnxr_builder *b, int32_t medium);                  /* Camera::medium, core/Camera.h; -1 == none */                 /* RenderThread.cpp:60-68 */
/* The returned description points into builder-owned memory, valid until the next builder
 * call or gnxr_builder_destroy.                                                            */
int gnxr_builder_desc(gnxr_builder *b, gnxr_scene_desc *out);

/* Deterministic synthetic stand-in for the absent Resources/dragon.3d (.MISSING_LARGE_BLOBS:1):
 * writes a `.3d` text file in the format plyRead.h:19-48 parses.                           */
int gnxr_write_synthetic_3d(const char *path, int32_t target_triangles, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* GNXR_H */
