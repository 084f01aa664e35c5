// host_scene.h -- host side of libgnxr: scene authoring (mirror of ui/ModelList.cpp and
// ui/MaterialList.cpp) and the scene compiler that flattens a gnxr_scene_desc into a CompiledScene: the tables a device takes once
// (SceneUploadTables) and the facts a live scene's host side keeps (SceneFacts).
#pragma once
#include <string>
#include <vector>

#include "../../include/gnxr.h"
#include "gnxr_device_types.h"
#include "host_math.h"

namespace gnxr {

void set_error(const char *fmt, ...);
const char *get_error();

// ---------------- authoring ----------------
struct Builder {
    std::vector<float> vertices;   // world space
    std::vector<int32_t> indices, tri_material, tri_light, tri_med_in, tri_med_out;
    std::vector<gnxr_material> materials;
    std::vector<gnxr_light> lights;
    std::vector<gnxr_medium> media;
    std::vector<gnxr_sphere> spheres;
    std::vector<float> grid_density;
    std::vector<gnxr_texture> textures;
    std::vector<float> texels;
    std::vector<float> tri_uv;     // empty, or 6 floats per triangle (defaults for triangles never given uvs)
    std::vector<float> tri_n;      // empty, or 9 floats per triangle (zeros for triangles without normals)
    std::vector<float> tri_s;      // empty, or 9 floats per triangle (zeros for triangles without tangents)
    std::vector<float> env_rgb;
    int env_w = 0, env_h = 0;
    gnxr_camera camera;
    int camera_medium = -1;
    int bvh_split_method = 0;
    Builder();
    int add_mesh(const float *verts, int nv, const int32_t *idx, int nt, const Xf &o2w, int material, int med_in, int med_out);
    void fill_desc(gnxr_scene_desc *d) const;
};

bool read_model_3d(const char *path, std::vector<float> *verts, std::vector<int32_t> *idx);  // shape/plyRead.h:19-48
bool write_synthetic_3d(const char *path, int target_tris, uint32_t seed);
bool read_rgbe(const char *path, std::vector<float> *rgb, int *w, int *h);  // what stbi_loadf returns for a .hdr

// ---------------- compiled scene ----------------
// What compile_scene produces comes in two parts.  The UPLOAD TABLES are bulk data that exists to be copied to a device once: after
// gnxr_scene_create the devices hold the only copy, and every edit of a live scene (refit, rebuild, set_geometry, material, attribute, media
// and texture edits) changes it there.  The SCENE FACTS are what the host authored or keeps reading; a handle keeps exactly these
// (SceneHost, api_scene.hip.h).  Nothing in leaf or node order is a fact, except the refit's seeds until they are uploaded (RefitSeeds).
struct SceneUploadTables {
    std::vector<DNode> nodes;
    std::vector<DNode4> nodes4;          // 4-wide collapse of `nodes`, cuts of least surface area (wide_collapse.h; same leaf visiting order)
    std::vector<DTri> tris;              // leaf order
    std::vector<float> leaf_boxes;       // 8 floats per leaf-order triangle, valid at the first triangle of each leaf: the leaf's LinearBVHNode bounds (lo.xyz hi.x | hi.yz 0 0)
    std::vector<uint8_t> tri_class;      // per leaf-order triangle: the key the binning pass gives a path that hit it: DMaterial::shade_class of its material (0 for null materials) | material_kind() << kClassKeyKindShift
    std::vector<int32_t> leaf_of_prim;   // authoring index -> leaf index
    std::vector<int32_t> tri_media;      // leaf order, (inside, outside) per triangle; empty when no triangle is a medium boundary
    std::vector<float> tri_uv;           // empty, or 8 floats per leaf-order triangle: (u,v) x 3 corners + pad
    std::vector<float> tri_n;            // empty, or 12 floats per leaf-order triangle: 3 shading normals + pad (zeros == none)
    std::vector<float> tri_s;            // the same for TriangleMesh::s (shading tangents)
    std::vector<float> tex_texels;       // float4 (rgb_) per texel, all levels of all textures (SceneFacts::textures holds their offsets)
    std::vector<float> grid_density;     // the media's density grids (SceneFacts::dmedia holds their offsets)
    std::vector<float> ewa_lut;          // MIPMap::weightLut
};

// The refit's seed tables (gnxr_scene_update_vertices): the one set that goes to a device lazily, at the first edit of the scene, so that a
// scene that is never edited takes no device memory for them.  compile_scene fills them in the CompiledScene; gnxr_scene_create moves them
// into SceneFacts::refit_seeds, which releases them once every copy of the scene holds its own (refit_tables, api_edit.hip.h).  After
// gnxr_scene_rebuild_bvh or gnxr_scene_set_geometry the devices' tables are the only ones.
struct RefitSeeds {
    std::vector<int32_t> corner_vertex;  // 3 per leaf-order triangle: the authored vertex of each corner
    std::vector<int32_t> node_parent;    // per DNode: its parent (-1 at the root)
    std::vector<int32_t> node4_src;      // 4 per DNode4: the DNode behind each child slot (-1: kNode4Empty)
};

struct SceneFacts {
    // geometry: the counts and flags of the upload tables (compile_scene fills them; rebuild and set_geometry keep them current)
    size_t n_triangles = 0, n_nodes = 0, n_nodes4 = 0;   // tris / nodes / nodes4
    bool has_tri_media = false, has_tri_uv = false, has_tri_n = false, has_tri_s = false;   // the table exists (is not empty)
    int32_t root4 = 0;                   // root reference (a leaf ref when the scene has a single leaf)
    int stack4_need = 1;                 // worst-case traversal stack entries for nodes4
    int leaf1_from_verts = 0;            // every one-triangle leaf's bounds == min / max of its triangle's vertices (checked in compile_scene)
    int bvh_max_depth = 0;
    Box3 world_bound;
    int n_vertices = 0;                  // gnxr_scene_desc::n_vertices
    RefitSeeds refit_seeds;              // a live scene's, until every copy holds them (empty in a CompiledScene, which carries them itself)
    // shading
    std::vector<DMaterial> materials;
    std::vector<DMaterial> materials_single;   // allowMultipleLobes == false (Whitted)
    std::vector<DTexture> textures;            // image textures: parameters + level offsets into the texel table
    std::vector<gnxr_texture> desc_textures;   // gnxr_scene_desc::textures with texel_offset zeroed (the raw texels are not retained): what a parameters-only texture edit compares against
    std::vector<float> aov_albedo;             // feature buffers: float4 per AUTHORED material, gnxr_material_albedo's rgb + the bits of kd_texture
    std::vector<int32_t> material_authored;    // per entry of `materials` (the attribute copies included): the authored material index
    // material edits (gnxr_scene_update_materials / gnxr_scene_set_triangle_materials): what compile_materials reads, in AUTHORING order and
    // therefore valid whatever leaf order the tree has; the two per-triangle tables go to the device at the first edit
    std::vector<gnxr_material> desc_materials;   // gnxr_scene_desc::materials
    std::vector<int32_t> tri_material;           // gnxr_scene_desc::tri_material
    std::vector<uint8_t> tri_own_attr;           // per authored triangle: 1 = uvs other than the defaults, normals or tangents of its own
    std::vector<int32_t> sphere_material;        // gnxr_sphere::material (DSphere::material is -1 for a GNXR_MAT_NONE material)
    std::vector<int32_t> mat_map;                // 4 per authored material: internal index (-1: no BSDF), its attribute copy (-1: none), shade class, kind (material_kind)
    std::vector<DLight> lights;
    std::vector<int32_t> infinite_lights;
    // sampler
    std::vector<uint16_t> perms;
    std::vector<int32_t> primes, prime_sums;
    std::vector<uint32_t> prime_magic;   // 8 words per prime: multiplier, shift (exact u32 division), base, permutation offset, 1 / base, perm[0] tail, ceil(2^32 / base), 0
    // env light
    bool has_env = false;
    DEnv env;
    std::vector<float> env_texels;       // Lmap level 0, rgb
    std::vector<float> env_texels4;      // the same as float4 (rgb_) per texel: one dwordx4 per texel of the bilinear lookup on the device
    float env_power_lookup[3] = {0, 0, 0};   // Lmap->Lookup((.5,.5), .5), for InfiniteAreaLight::Power
    std::vector<float> env_cond_func, env_cond_cdf, env_cond_int;   // Distribution2D conditional rows
    std::vector<float> env_marg_func, env_marg_cdf;
    std::vector<uint16_t> env_marg_guide, env_cond_guide;   // FindInterval guide tables (kEnvGuideMarg + 1 entries; per row kEnvGuideCond + 1)
    // media
    std::vector<gnxr_medium> media;
    std::vector<DMedium> dmedia;
    std::vector<DSphere> spheres;
    int n_spheres = 0;
    // camera description (matrices depend on the render resolution)
    gnxr_camera camera;
    int camera_medium = -1;
    // copy of the description for the light grid builder
    std::vector<gnxr_light> desc_lights;
};

// the whole of what compile_scene produces (the stand-alone host checks and gnxr_scene_create's local)
struct CompiledScene : SceneUploadTables, RefitSeeds, SceneFacts {};

// HLBVH (GNXR_BVH_HLBVH, BVHAccel.cpp:369-626) is built by the caller's device stage (api_hlbvh.hip.h + hlbvh_build.hip.h): Morton codes, radix
// sort, one LBVH per treelet and the SAH over the treelet roots.  It returns the build tree -- leaves index the sorted primitive array
// (`first`, `n`), interior nodes carry their two children and the split axis -- its root, and the sorted primitive order.
struct HlbvhNode { float b[6]; int32_t child[2]; int32_t axis, first, n; };   // bounds lo.xyz hi.xyz
typedef bool (*HlbvhBuildFn)(const float *prim_bounds6, const float *centroids3, int n, const float lo[3], const float hi[3],
                             std::vector<HlbvhNode> *nodes, int *root, uint32_t *prims_sorted);
bool compile_scene(const gnxr_scene_desc *d, CompiledScene *out, HlbvhBuildFn hlbvh_build = nullptr);
// The materials section of compile_scene, which gnxr_scene_create and the material edits share: the internal material tables (one record per
// authored material, then one attribute copy per material that a triangle with uvs, normals or tangents of its own uses, numbered in the
// order `visit` -- n_triangles authored indices, null = authoring order -- meets them), the feature buffers' albedo table, the way back
// to the authored index and mat_map.  Validates as compile_scene does (texture references, textured materials on spheres, unknown types);
// false (error set) leaves *mt half-written and nothing else touched.
struct MaterialTables {
    std::vector<DMaterial> materials, materials_single;
    std::vector<float> aov_albedo;
    std::vector<int32_t> material_authored, mat_map;
    void move_to(SceneFacts *cs);
};
bool compile_materials(const gnxr_material *mats, int n_materials, int n_textures, const std::vector<int32_t> &sphere_material, const int32_t *tri_material,
                       const uint8_t *tri_own_attr, int n_triangles, const int32_t *visit, MaterialTables *mt);
// one triangle's DTri::material and tri_class byte from mat_map (k_material_tris, material_kernel.hip.h, is the device's form)
void triangle_material(const int32_t *mat_map, int32_t authored, uint8_t own_attr, int32_t *material, uint8_t *class_key);
// MATERIAL_KIND_* of a compiled material: non-zero for the class-1 materials that a narrow glossy kernel covers (conductor, rough dielectric)
int material_kind(const DMaterial &m);
// after a refit: the root box of the binary BVH (lo.xyz hi.xyz) -> world_bound (grown by the spheres), the environment light's bounding
// sphere and the distant lights' radius, computed as compile_scene computes them
void refit_world_bound(SceneFacts *cs, const float root6[6]);
// one DLight from its description, as compile_scene makes it (gnxr_scene_update_lights): for AREA_TRI from the corners of its triangle and
// its leaf index; for INFINITE the record without the environment tables; false (error set) for an unknown type
bool compile_light(const gnxr_light &l, int index, const Vec3 corners[3], int tri_leaf, const Box3 &world_bound, DLight *out);
// A whole new light list for a live scene (gnxr_scene_set_lights), checked and compiled before anything of the scene is touched: recs gets
// max(1, n) records as compile_scene makes them, except that an AREA_TRI record carries its AUTHORED triangle in tri_leaf and blank corners
// (the device binds it to its leaf-order triangle and computes the rest: lights_kernel.hip.h, k_refit_lights); infinite the indices of the
// INFINITE and SKYBOX records; light_of_prim per authored triangle the light that names it or -1.  Returns GNXR_OK, GNXR_ERR_INVALID (a
// triangle out of range or named twice, an unknown type) or GNXR_ERR_UNSUPPORTED (an INFINITE record added, dropped, changed in any byte or
// moved across a SKYBOX record: its tables are gnxr_scene_update_environment's), with the error set.
int compile_light_list(const SceneFacts &cs, const gnxr_light *in, int n, std::vector<DLight> *recs, std::vector<int32_t> *infinite, std::vector<int32_t> *light_of_prim);
// one DMedium from its description and, for a GRID medium, the maximum of its grid (GridDensityMedium.h:28-31: the fold from +0 over
// std::max), as compile_scene makes it (gnxr_scene_update_media): sigma_t, w2m = Inverse(medium_to_world), inv_max_density = 1 / max_density.
// density_offset is left 0: where the grid sits is the caller's.  false (error set) for an unknown type or an empty grid
bool compile_medium(const gnxr_medium &m, int index, float max_density, DMedium *out);
// the host's share of gnxr_scene_update_environment, whose tables the device builds (env_build_kernel.hip.h): MIPMap's power-of-two size,
// the Lanczos weights of its resample (they depend on the two sizes only), the sizes of the pyramid's levels, and InfiniteAreaLight::Power's
// lookup over the pyramid's top levels -- top_rgba[k] holds level first_level + k as float4 texels, first_level = max(0, levels - 3) --
// all computed by the code build_env runs for gnxr_scene_create
struct EnvResampleWeight { int32_t first; float w[4]; };
int env_round_up_pow2(int v);
std::vector<EnvResampleWeight> env_resample_weights(int old_res, int new_res);
void env_pyramid_sizes(int rx, int ry, std::vector<int> *lw, std::vector<int> *lh);
void env_power_from_top_levels(int rx, int ry, int first_level, const std::vector<std::vector<float>> &top_rgba, float out[3]);
// one DTexture from its description, as build_textures makes it (gnxr_scene_update_textures, whose pyramid the device builds): the
// power-of-two size, the number of levels and the mapping; level_offset counts from `first_texel`, the levels following each other
// without padding.  *n_texels receives the texels of all levels.  false (error set) for a size <= 0, an unknown wrap or more than 16 levels
bool compile_texture(const gnxr_texture &t, int index, int64_t first_texel, DTexture *out, int64_t *n_texels);
DCamera make_camera(const gnxr_camera &c, int W, int H, int medium);      // camera/Perspective.cpp:114-135, core/Camera.h:54-75
void camera_world_to_raster(const gnxr_camera &c, int W, int H, float w2r[16]);   // (s2r * c2s) * lookat of make_camera's factors
DHalton make_halton(int W, int H);                                          // samplers/HaltonSampler.cpp:33-60
// light-selection table: dense restatement of core/LightDistribution.cpp (uniform / power / spatial)
void build_light_grid(const SceneFacts &cs, int strategy, DLightGrid *grid, std::vector<float> *table, bool layout_only = false);
void light_grid_probes(const SceneFacts &cs, float *ri /* [5][128] */);

// host restatements used by probes and the light grid
float host_radical_inverse(const SceneFacts &cs, int baseIndex, uint64_t a);

}  // namespace gnxr
