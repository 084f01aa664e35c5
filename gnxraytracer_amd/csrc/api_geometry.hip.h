// api_geometry.hip.h -- gnxr_scene_set_geometry: host driver of the mesh replacement (geometry_kernel.hip.h in front of the rebuild of
// api_rebuild.hip.h).  Part of api.hip's translation unit (after api_rebuild.hip.h).
//
// Every device of the handle makes the authoring-order tables from the caller's arrays (geometry_on_device: k_geom_build, then
// k_material_tris once the host has compiled the material tables) and builds tree and leaf-order tables from them into FRESH buffers
// (rebuild_on_device with these tables as its source).  Only when all devices have reported clean flags and the same tree does anything of
// the scene change: the writes that can still fail first (the material tables with the DTexTables record, the spheres' primitive ids;
// a failure puts the old ones back), then the host scene once, then pointer swaps on every copy.  What crosses to the host: the flags and
// per-light counters, tri_material and the own-attribute bytes (compile_materials reads them; both are kept for the material edits), the
// root box, and what the rebuild fetches (counts, result scalars, the light records).  Vertex and index data reach the host only on
// their way to further devices of gnxr_init_devices.
#pragma once

namespace {

// the caller's arrays as one device sees them: the caller's own pointers, or copies the call owns
struct GeomArrays {
    gnxr_geometry g;
    DevBuf<float> vertices, tri_uv, tri_n, tri_s;
    DevBuf<int32_t> indices, tri_material, tri_light, med_in, med_out;
    // host arrays -> the (bound) device, queued on st
    int stage(const gnxr_geometry &h, hipStream_t st) {
        g = h;
        const size_t nt = (size_t)h.n_triangles;
        int rc;
#define GX_STAGE(field, buf, count)                                                                                         \
    if (h.field) {                                                                                                          \
        if ((rc = buf.alloc(count)) != GNXR_OK) return rc;                                                                  \
        HIP_TRY(hipMemcpyAsync(buf.p, h.field, (count) * sizeof(*h.field), hipMemcpyHostToDevice, st));                     \
        g.field = buf.p;                                                                                                    \
    }
        GX_STAGE(vertices, vertices, 3 * (size_t)h.n_vertices) GX_STAGE(indices, indices, 3 * nt) GX_STAGE(tri_material, tri_material, nt) GX_STAGE(tri_light, tri_light, nt)
        GX_STAGE(tri_medium_inside, med_in, nt) GX_STAGE(tri_medium_outside, med_out, nt) GX_STAGE(tri_uv, tri_uv, 6 * nt) GX_STAGE(tri_n, tri_n, 9 * nt) GX_STAGE(tri_s, tri_s, 9 * nt)
#undef GX_STAGE
        return GNXR_OK;
    }
};

// device arrays of the primary -> host copies (for the other devices of the handle); *h points into `keep`
struct GeomHostCopy {
    std::vector<float> vertices, tri_uv, tri_n, tri_s;
    std::vector<int32_t> indices, tri_material, tri_light, med_in, med_out;
    int fetch(const gnxr_geometry &d, gnxr_geometry *h) {
        *h = d;
        const size_t nt = (size_t)d.n_triangles;
#define GX_FETCH(field, vec, count)                                                                                         \
    if (d.field) {                                                                                                          \
        vec.resize(count);                                                                                                  \
        HIP_TRY(hipMemcpy(vec.data(), d.field, (count) * sizeof(*d.field), hipMemcpyDeviceToHost));                         \
        h->field = vec.data();                                                                                              \
    }
        GX_FETCH(vertices, vertices, 3 * (size_t)d.n_vertices) GX_FETCH(indices, indices, 3 * nt) GX_FETCH(tri_material, tri_material, nt) GX_FETCH(tri_light, tri_light, nt)
        GX_FETCH(tri_medium_inside, med_in, nt) GX_FETCH(tri_medium_outside, med_out, nt) GX_FETCH(tri_uv, tri_uv, 6 * nt) GX_FETCH(tri_n, tri_n, 9 * nt) GX_FETCH(tri_s, tri_s, 9 * nt)
#undef GX_FETCH
        return GNXR_OK;
    }
};

// what the host learns from the primary's pass and shares with the other devices
struct GeomHost {
    std::vector<int32_t> tri_material, light_tri;   // light_tri: per light the triangle that names it (-1: none)
    std::vector<uint8_t> own_attr;
    MaterialTables mt;
    std::vector<DSphere> spheres;
    float root6[6] = {0, 0, 0, 0, 0, 0};
};

// 0: host memory, 1: device memory of `device`, -1: device memory of another device
int geometry_side(const void *p, int device) {
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();   // memory the runtime has never seen (malloc, numpy) makes the call fail: that is the answer
    if (e != hipSuccess || at.type != hipMemoryTypeDevice) return 0;
    return at.device == device ? 1 : -1;
}

int geometry_refusal(int flags) {
    using namespace geom;
    if (flags & G_BAD_INDEX) set_error("set_geometry: triangle index out of range");
    else if (flags & G_BAD_MATERIAL) set_error("set_geometry: material index out of range");
    else if (flags & G_BAD_MEDIUM) set_error("set_geometry: medium index out of range");
    else if (flags & G_BAD_LIGHT) set_error("set_geometry: light index out of range");
    else if (flags & G_NOT_FINITE) set_error("set_geometry: a triangle has a corner or a centroid that is not finite");
    else if (flags & G_EMISSIVE_NORMALS) set_error("set_geometry: per-vertex normals on an emissive triangle are not supported");
    else set_error("set_geometry: per-vertex tangents on an emissive triangle are not supported");
    return GNXR_ERR_INVALID;
}

// One copy's build on its (bound) device from the arrays `d` (device memory there).  `first`: the primary, which validates for all and
// fills *hh (the material tables included); the other copies read *hh.  Nothing of `s` changes.
int geometry_on_device(gnxr_scene *s, const gnxr_geometry &d, hipStream_t st, bool first, GeomHost *hh, Rebuilt *out) {
    const SceneFacts &cs = s->cs;
    const int nt = d.n_triangles, n_lights = (int)cs.desc_lights.size(), n_chk = 1 + 2 * n_lights;
    const size_t n = (size_t)nt;
    const bool has_media = d.tri_medium_inside != nullptr, has_uv = d.tri_uv != nullptr, has_n = d.tri_n != nullptr, has_s = d.tri_s != nullptr;
    // ---- the authoring-order tables
    DevBuf<DTri> tris;
    DevBuf<uint8_t> tri_class, own;
    DevBuf<int32_t> corner, tri_media, chk, mat_map;
    DevBuf<float> tri_uv, tri_n, tri_s;
    DevBuf<DLight> lights;
    int rc;
    if ((rc = tris.alloc(n)) || (rc = tri_class.alloc(n)) || (rc = own.alloc(n)) || (rc = corner.alloc(3 * n)) || (rc = chk.alloc(n_chk)) || (has_media && (rc = tri_media.alloc(2 * n))) ||
        (has_uv && (rc = tri_uv.alloc(8 * n))) || (has_n && (rc = tri_n.alloc(12 * n))) || (has_s && (rc = tri_s.alloc(12 * n))) || (rc = lights.alloc(cs.lights.size())))
        return rc;
    std::vector<int> h_chk(n_chk, 0);
    for (int l = 0; l < n_lights; ++l) h_chk[1 + n_lights + l] = -1;
    HIP_TRY(hipMemcpyAsync(chk.p, h_chk.data(), n_chk * sizeof(int), hipMemcpyHostToDevice, st));
    geom::GeomIn in;
    in.vertices = d.vertices; in.indices = d.indices; in.tri_material = d.tri_material; in.tri_light = d.tri_light;
    in.med_in = d.tri_medium_inside; in.med_out = d.tri_medium_outside; in.tri_uv = d.tri_uv; in.tri_n = d.tri_n; in.tri_s = d.tri_s;
    in.n_vertices = d.n_vertices; in.n_triangles = nt; in.n_materials = (int)cs.desc_materials.size(); in.n_media = (int)cs.media.size(); in.n_lights = n_lights;
    geom::GeomOut o;
    o.tris = tris.p; o.own_attr = own.p; o.corner = corner.p; o.chk = chk.p;
    o.tri_media = has_media ? reinterpret_cast<int2 *>(tri_media.p) : nullptr;
    o.tri_uv = has_uv ? reinterpret_cast<float4 *>(tri_uv.p) : nullptr;
    o.tri_n = has_n ? reinterpret_cast<float4 *>(tri_n.p) : nullptr;
    o.tri_s = has_s ? reinterpret_cast<float4 *>(tri_s.p) : nullptr;
    hipLaunchKernelGGL(geom::k_geom_build, dim3(grid_for(nt)), dim3(refit::kB), 0, st, in, o);
    HIP_TRY(hipGetLastError());
    // ---- flags and per-light counters: one small copy
    HIP_TRY(hipMemcpyAsync(h_chk.data(), chk.p, n_chk * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_chk[0]) return geometry_refusal(h_chk[0]);
    for (int l = 0; l < n_lights; ++l) {
        const bool area = cs.desc_lights[l].type == GNXR_LIGHT_AREA_TRI;
        const int named = h_chk[1 + l];
        if (!area && named > 0) { set_error("set_geometry: tri_light names light %d, which is not an AREA_TRI light", l); return GNXR_ERR_INVALID; }
        if (area && named != 1) { set_error("set_geometry: AREA_TRI light %d is named by %d triangles (exactly one must name it)", l, named); return GNXR_ERR_INVALID; }
    }
    if (first) {
        // ---- the two small per-triangle tables compile_materials reads, and the material tables (attribute copies in authoring order:
        // their numbering shows in no result)
        hh->light_tri.assign(h_chk.begin() + 1 + n_lights, h_chk.end());
        hh->tri_material.resize(n); hh->own_attr.resize(n);
        HIP_TRY(hipMemcpyAsync(hh->tri_material.data(), d.tri_material, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hh->own_attr.data(), own.p, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!compile_materials(cs.desc_materials.data(), (int)cs.desc_materials.size(), (int)cs.textures.size(), cs.sphere_material, hh->tri_material.data(), hh->own_attr.data(), nt, nullptr,
                               &hh->mt))
            return GNXR_ERR_INVALID;
        hh->spheres = cs.spheres;
        for (int i = 0; i < cs.n_spheres; ++i) hh->spheres[i].prim = nt + i;
    }
    // ---- DTri::material and the class byte through mat_map
    if ((rc = mat_map.alloc(hh->mt.mat_map.size())) != GNXR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(mat_map.p, hh->mt.mat_map.data(), hh->mt.mat_map.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(matedit::k_material_tris, dim3(grid_for(nt)), dim3(refit::kB), 0, st, tris.p, tri_class.p, nt, (const int *)d.tri_material, (const unsigned char *)own.p,
                       reinterpret_cast<const int4 *>(mat_map.p));
    HIP_TRY(hipGetLastError());
    // ---- the light records: the scene's, each area light on the row of the triangle that names it; the rebuild recomputes the rest
    std::vector<DLight> h_lights = cs.lights;
    for (int l = 0; l < n_lights; ++l) if (cs.desc_lights[l].type == GNXR_LIGHT_AREA_TRI) h_lights[l].tri_leaf = hh->light_tri[l];
    HIP_TRY(hipMemcpyAsync(lights.p, h_lights.data(), h_lights.size() * sizeof(DLight), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (h_lights and hh->mt.mat_map are pageable: the copies have left them)
    // ---- tree and leaf-order tables: the rebuild, from these tables instead of the scene's
    RebuildSource src;
    src.n = nt; src.tris = tris.p; src.tri_class = tri_class.p; src.corner = corner.p;
    src.tri_media = has_media ? tri_media.p : nullptr;
    src.tri_uv = has_uv ? tri_uv.p : nullptr; src.tri_n = has_n ? tri_n.p : nullptr; src.tri_s = has_s ? tri_s.p : nullptr;
    src.lights = lights.p; src.refit_lights = true;
    if ((rc = rebuild_on_device(s, src, st, out)) != GNXR_OK) return rc;   // (it allocates exactly the per-corner and media tables the source has)
    if (first) {
        DNode root;
        HIP_TRY(hipMemcpyAsync(&root, out->nodes.p, sizeof(DNode), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        hh->root6[0] = root.lo[0]; hh->root6[1] = root.lo[1]; hh->root6[2] = root.lo[2]; hh->root6[3] = root.hi0; hh->root6[4] = root.hi1; hh->root6[5] = root.hi2;
    }
    return GNXR_OK;
}

// The writes of the commit that can fail, on one copy's (bound) device: the material tables behind the record that points at the
// per-corner tables (at the addresses given), the feature buffers' tables and the spheres.  All in place: the buffers were sized for the
// worst case by upload_scene.  Used with the new state and, after a failure, with the old one.
int geometry_write_tables(gnxr_scene *s, const std::vector<DMaterial> &materials, const std::vector<DMaterial> &materials_single, const std::vector<float> &aov_albedo,
                          const std::vector<int32_t> &material_authored, const std::vector<DSphere> &spheres, const float *uv, const float *n, const float *sv) {
    const size_t ni = materials.size();
    if (ni + 1 > s->materials.n || ni + 1 > s->materials_single.n || ni > s->material_authored.n || aov_albedo.size() > s->aov_albedo.n || spheres.size() > s->spheres.n) {
        set_error("set_geometry: %zu internal materials do not fit the scene's tables", ni);
        return GNXR_ERR_RUNTIME;
    }
    if (int rc = s->write_material_tables(materials, materials_single, uv, n, sv)) return rc;
    HIP_TRY(hipMemcpy(s->aov_albedo.p, aov_albedo.data(), aov_albedo.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->material_authored.p, material_authored.data(), ni * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->spheres.p, spheres.data(), spheres.size() * sizeof(DSphere), hipMemcpyHostToDevice));
    return GNXR_OK;
}

// the host scene, once: the counts and flags of the new mesh's tables (which exist on the devices only), the authoring-order tables of the
// material edits, and what follows the mesh, recomputed as compile_scene computes it
void geometry_commit_host(gnxr_scene *s, const gnxr_geometry &g, GeomHost &hh, Rebuilt &r) {
    SceneFacts &cs = s->cs;
    rebuild_commit_host(s, r);   // node counts, result scalars, the light records
    cs.n_triangles = (size_t)g.n_triangles;
    cs.has_tri_media = r.tri_media.p != nullptr; cs.has_tri_uv = r.tri_uv.p != nullptr; cs.has_tri_n = r.tri_n.p != nullptr; cs.has_tri_s = r.tri_s.p != nullptr;
    cs.n_vertices = g.n_vertices;
    cs.tri_material = std::move(hh.tri_material);
    cs.tri_own_attr = std::move(hh.own_attr);
    hh.mt.move_to(&cs);
    cs.spheres = std::move(hh.spheres);
    for (size_t l = 0; l < cs.desc_lights.size(); ++l) if (cs.desc_lights[l].type == GNXR_LIGHT_AREA_TRI) cs.desc_lights[l].tri = hh.light_tri[l];
    refit_world_bound(&cs, hh.root6);   // Scene::WorldBound, the environment light's bounding sphere, the delta lights' radius (in cs.lights: refit_world uploads them)
}
// ... then every copy: pointer swaps; the tables of the old mesh that the new one lacks go, as do the material edits' authoring-order
// tables (material_tables uploads the new ones at the next edit) and the vertex -> corner table of gnxr_scene_recompute_normals
void geometry_commit_copy(gnxr_scene *s, Rebuilt &r) {
    const bool has_media = r.tri_media.p, has_uv = r.tri_uv.p, has_n = r.tri_n.p, has_s = r.tri_s.p;   // (asked before the swaps)
    rebuild_commit_copy(s, r);
    if (!has_media) s->tri_media.release();
    if (!has_uv) s->tri_uv.release();
    if (!has_n) s->tri_n.release();
    if (!has_s) s->tri_s.release();
    s->mat_map.release(); s->mat_tri.release(); s->mat_own.release();
    s->adj_offsets.release(); s->adj_corners.release();   // the normals' adjacency follows the index array (api_deform.hip.h builds the new one at the next call)
}

}  // namespace

extern "C" int gnxr_scene_set_geometry(gnxr_scene *s, const gnxr_geometry *g, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (!g) { set_error("null geometry record"); return GNXR_ERR_INVALID; }
    if (g->struct_size != (int32_t)sizeof(gnxr_geometry)) { set_error("gnxr_geometry::struct_size is %d, this library's record has %zu bytes", g->struct_size, sizeof(gnxr_geometry)); return GNXR_ERR_INVALID; }
    if (g->n_vertices < 1 || g->n_triangles < 1) { set_error("set_geometry: %d vertices, %d triangles", g->n_vertices, g->n_triangles); return GNXR_ERR_INVALID; }
    if (!g->vertices || !g->indices || !g->tri_material) { set_error("set_geometry: null vertices, indices or tri_material"); return GNXR_ERR_INVALID; }
    if ((g->tri_medium_inside != nullptr) != (g->tri_medium_outside != nullptr)) { set_error("set_geometry: only one of the two medium arrays"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    if (!g->tri_light)
        for (const gnxr_light &l : cs.desc_lights)
            if (l.type == GNXR_LIGHT_AREA_TRI) { set_error("set_geometry: null tri_light in a scene with AREA_TRI lights"); return GNXR_ERR_INVALID; }
    int rc = s->bind();
    if (rc) return rc;
    // all arrays on one side
    const void *arrays[] = {g->vertices, g->indices, g->tri_material, g->tri_light, g->tri_medium_inside, g->tri_medium_outside, g->tri_uv, g->tri_n, g->tri_s};
    int side = -2;
    for (const void *p : arrays) {
        if (!p) continue;
        const int sd = geometry_side(p, s->device);
        if (sd < 0) { set_error("set_geometry: an array lives on another device than the scene's first device %d", s->device); return GNXR_ERR_INVALID; }
        if (side != -2 && sd != side) { set_error("set_geometry: the arrays are partly host memory, partly device memory"); return GNXR_ERR_INVALID; }
        side = sd;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // 1. every device builds into fresh buffers (the primary on the caller's stream, validating for all), and all must have built the same tree
    std::vector<Rebuilt> built(s->n_copies());
    GeomHost hh;
    {
        GeomArrays prim;
        prim.g = *g;
        if (side == 0 && (rc = prim.stage(*g, st)) != GNXR_OK) return rc;
        if ((rc = geometry_on_device(s, prim.g, st, /*first=*/true, &hh, &built[0])) != GNXR_OK) { (void)hipGetLastError(); return rc; }
        if (s->n_copies() > 1) {   // gnxr_init_devices: the same build on every replica, from host memory
            GeomHostCopy keep;
            gnxr_geometry h = *g;
            if (side == 1 && (rc = keep.fetch(*g, &h)) != GNXR_OK) return rc;
            rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int {
                if (i == 0) return GNXR_OK;
                GeomArrays arr;
                if (int rc_ = arr.stage(h, nullptr)) return rc_;
                return geometry_on_device(c, arr.g, nullptr, /*first=*/false, &hh, &built[i]);
            });
            if (rc) return rc;
        }
    }
    for (size_t i = 1; i < built.size(); ++i)
        if (!built[i].same_tree(built[0])) { set_error("set_geometry: the devices disagree (internal error)"); return GNXR_ERR_RUNTIME; }
    // 2. the only writes that can still fail; a failure puts the tables the host scene still describes back on every copy
    rc = s->apply_or_put_back([&](gnxr_scene *c, size_t i) -> int {
        const Rebuilt &r = built[i];
        if (int rc_ = refit_tables(c)) return rc_;   // the swaps below exchange the refit's tables: the set must exist (its flag marks it complete)
        return geometry_write_tables(c, hh.mt.materials, hh.mt.materials_single, hh.mt.aov_albedo, hh.mt.material_authored, hh.spheres, r.tri_uv.p, r.tri_n.p, r.tri_s.p);
    }, [&](gnxr_scene *c, size_t) -> int {
        const DTexTables old = c->tex_tables(c->tri_uv.p, c->tri_n.p, c->tri_s.p);
        return geometry_write_tables(c, cs.materials, cs.materials_single, cs.aov_albedo, cs.material_authored, cs.spheres, old.tri_uv, old.tri_n, old.tri_s);
    });
    if (rc) return rc;
    // 3. the host scene, then the swaps, then what depends on the world bound and the light records
    geometry_commit_host(s, *g, hh, built[0]);
    for (size_t i = 0; i < s->n_copies(); ++i) geometry_commit_copy(s->copy(i), built[i]);
    return s->each_copy(refit_world);
    // the old tables are released with `built` (hipFree waits for what still reads them)
}
