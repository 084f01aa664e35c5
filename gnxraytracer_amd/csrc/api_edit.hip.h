// api_edit.hip.h -- editing a scene in place: gnxr_scene_update_vertices[_ex] (the BVH refit, refit_kernel.hip.h), gnxr_scene_update_lights,
// gnxr_scene_update_materials / gnxr_scene_set_triangle_materials (material_kernel.hip.h) and gnxr_scene_set_camera.  Part of api.hip's
// translation unit (before api_rebuild.hip.h, which uses refit_tables).  An edit changes the handle's one host scene (SceneHost) once and
// the device tables of every copy in turn (each_copy), under the primary's render_mutex.
#pragma once

// the refit's tables go to a device at the first update of the scene, from the host's seeds (the flag is allocated last: it marks the set
// complete).  The seeds are released when the last copy has taken them; a copy whose upload failed finds them at the next edit.
static int refit_tables(gnxr_scene *s) {
    if (s->upd_flag.p) return GNXR_OK;
    SceneFacts &cs = s->cs;
    const RefitSeeds &seeds = cs.refit_seeds;
    int rc;
    if ((rc = s->upd_corner.upload(seeds.corner_vertex)) || (rc = s->upd_parent.upload(seeds.node_parent)) || (rc = s->upd_node4_src.upload(seeds.node4_src)) ||
        (rc = s->upd_arrived.alloc(cs.n_nodes)) || (rc = s->upd_flag.alloc(1)))
        return rc;
    if (--s->host->copies_awaiting_seeds == 0) cs.refit_seeds = RefitSeeds();
    return GNXR_OK;
}

// positions of vertices [first, first + n) staged in s->upd_xyz -> triangles, binary tree, 4-wide tree on the scene's (bound) device;
// returns the refitted root box.  Topology, primitive order and every id stay as they are, so the one-triangle leaves still have the
// min / max of their triangle's corners as their box (k_refit_fit computes it so) and SceneFacts::leaf1_from_verts keeps its value.
// move_lights (GNXR_UPDATE_MOVE_LIGHTS): the AREA_TRI light records are recomputed from the moved triangles (k_refit_lights); with h_lights
// every record comes back with the root box, behind the same synchronisation: refit_world uploads the host copy over the device's afterwards.
static int refit_apply(gnxr_scene *s, int first, int n, hipStream_t st, float root6[6], bool move_lights = false, std::vector<DLight> *h_lights = nullptr) {
    const SceneFacts &cs = s->cs;
    const int nt = (int)cs.n_triangles, nn = (int)cs.n_nodes, nslots = (int)(4 * cs.n_nodes4);
    hipLaunchKernelGGL(refit::k_refit_tris, dim3(grid_for(nt)), dim3(refit::kB), 0, st, s->tris.p, (const int *)s->upd_corner.p, nt, first, n, (const float *)s->upd_xyz.p);
    HIP_TRY(hipMemsetAsync(s->upd_arrived.p, 0, (size_t)nn * sizeof(unsigned int), st));
    hipLaunchKernelGGL(refit::k_refit_fit, dim3(grid_for(nn)), dim3(refit::kB), 0, st, nn, s->nodes.p, (const int *)s->upd_parent.p, s->upd_arrived.p, (const DTri *)s->tris.p,
                       s->leaf_boxes.p);
    // (the 4-wide slots copy finished boxes: the launch boundary orders them after the fit; k_trace4's top-of-tree LDS copy is
    // loaded from nodes4 at the start of every launch)
    hipLaunchKernelGGL(refit::k_refit_wide, dim3(grid_for(nslots)), dim3(refit::kB), 0, st, nslots, s->nodes4.p, (const int *)s->upd_node4_src.p, (const DNode *)s->nodes.p);
    const int n_lights = (int)cs.desc_lights.size();   // (a scene without lights still holds one blank record)
    if (move_lights && n_lights > 0) hipLaunchKernelGGL(refit::k_refit_lights, dim3(grid_for(n_lights)), dim3(refit::kB), 0, st, s->lights.p, n_lights, (const DTri *)s->tris.p, nt);
    HIP_TRY(hipGetLastError());
    DNode root;
    HIP_TRY(hipMemcpyAsync(&root, s->nodes.p, sizeof(DNode), hipMemcpyDeviceToHost, st));
    if (h_lights) {
        h_lights->resize(cs.lights.size());
        HIP_TRY(hipMemcpyAsync(h_lights->data(), s->lights.p, cs.lights.size() * sizeof(DLight), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    root6[0] = root.lo[0]; root6[1] = root.lo[1]; root6[2] = root.lo[2]; root6[3] = root.hi0; root6[4] = root.hi1; root6[5] = root.hi2;
    return GNXR_OK;
}

// One copy's share of what depends on the world bound or the light records (an each_copy callable): cs.lights over the (bound) device's
// records -- the delta lights' radius, moved or edited lights -- and a new light-selection table at the next render (ensure_grid).  The host's
// share (Scene::WorldBound, the environment light's bounding sphere in DEnv, read at every render) is refit_world_bound's, once per edit.
static int refit_world(gnxr_scene *s, size_t) {
    HIP_TRY(hipMemcpy(s->lights.p, s->cs.lights.data(), s->cs.lights.size() * sizeof(DLight), hipMemcpyHostToDevice));
    s->grid_strategy = -1;
    return GNXR_OK;
}

extern "C" int gnxr_scene_update_vertices_ex(gnxr_scene *s, int32_t first_vertex, int32_t n_vertices, const float *xyz, uint32_t flags, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (flags & ~(uint32_t)GNXR_UPDATE_MOVE_LIGHTS) { set_error("unknown update flags 0x%x", flags); return GNXR_ERR_INVALID; }
    if (n_vertices > 0 && !xyz) { set_error("null vertex array"); return GNXR_ERR_INVALID; }
    if (first_vertex < 0 || n_vertices < 0 || (int64_t)first_vertex + n_vertices > (int64_t)s->cs.n_vertices) {
        set_error("vertex range [%d, %lld) outside the scene's %d vertices", first_vertex, (long long)first_vertex + n_vertices, s->cs.n_vertices);
        return GNXR_ERR_INVALID;
    }
    if (n_vertices == 0) return GNXR_OK;
    const bool move_lights = (flags & GNXR_UPDATE_MOVE_LIGHTS) != 0;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    int rc = s->bind();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t nf = 3 * (size_t)n_vertices;
    if ((rc = refit_tables(s)) || (rc = s->upd_xyz.alloc(nf))) return rc;
    // one copy path for host and device memory; ordered after what the caller queued on its stream
    HIP_TRY(hipMemcpyAsync(s->upd_xyz.p, xyz, nf * sizeof(float), hipMemcpyDefault, st));
    if (!move_lights) {
        // emissive triangles keep their vertices (their DLight records hold them): refuse before anything is written
        int h_flag = 0;
        const int nt = (int)s->cs.n_triangles;
        HIP_TRY(hipMemsetAsync(s->upd_flag.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(refit::k_refit_check, dim3(grid_for(nt)), dim3(refit::kB), 0, st, (const DTri *)s->tris.p, (const int *)s->upd_corner.p, nt, first_vertex, n_vertices,
                           (const float *)s->upd_xyz.p, s->upd_flag.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h_flag, s->upd_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_flag) {
            set_error("a vertex of an emissive (AREA_TRI) triangle would move: pass GNXR_UPDATE_MOVE_LIGHTS to gnxr_scene_update_vertices_ex to move area lights");
            return GNXR_ERR_UNSUPPORTED;
        }
    }
    float root6[6];
    // the moved light records, held back until all devices have refitted (a failure before that leaves the host scene alone).  Every device
    // holds the same tree and the same records, so the primary's are fetched for all.
    std::vector<DLight> moved;
    if ((rc = refit_apply(s, first_vertex, n_vertices, st, root6, move_lights, move_lights ? &moved : nullptr)) != GNXR_OK) return rc;
    if (s->n_copies() > 1) {   // gnxr_init_devices: the same refit on every replica, from a host copy of the staged positions
        std::vector<float> staged(nf);
        HIP_TRY(hipMemcpy(staged.data(), s->upd_xyz.p, nf * sizeof(float), hipMemcpyDeviceToHost));
        rc = s->each_copy([&](gnxr_scene *r, size_t i) -> int {
            if (i == 0) return GNXR_OK;   // the primary has refitted above, on the caller's stream
            float rroot[6];
            int rc_;
            if ((rc_ = refit_tables(r)) || (rc_ = r->upd_xyz.upload(staged.data(), nf))) return rc_;
            return refit_apply(r, first_vertex, n_vertices, nullptr, rroot, move_lights);
        });
        if (rc) return rc;
    }
    // the fetched records become the host's BEFORE refit_world_bound refreshes the delta lights' radius in them and refit_world
    // uploads them: the power table (build_light_grid) reads cs.lights[i].area, and a stale copy would undo the kernel's work
    if (move_lights) s->cs.lights = std::move(moved);
    refit_world_bound(&s->cs, root6);
    return s->each_copy(refit_world);
}

extern "C" int gnxr_scene_update_vertices(gnxr_scene *s, int32_t first_vertex, int32_t n_vertices, const float *xyz, void *hip_stream) {
    return gnxr_scene_update_vertices_ex(s, first_vertex, n_vertices, xyz, 0, hip_stream);
}

// The new records of lights [first, first + n): nothing of the scene is touched before every one of them has passed.  What a record may
// change: AREA_TRI le / two_sided / n_samples (its triangle stays; corners, area and normal come from the vertices the scene holds NOW,
// which cs.lights carries: gnxr_scene_update_vertices_ex and gnxr_scene_rebuild_bvh keep that copy current); POINT / SPOT / DISTANT
// everything; SKYBOX centre and radius; INFINITE nothing (its importance tables and texels are rebuilt by gnxr_scene_update_environment).
static int build_light_update(const SceneFacts &cs, int first, int n, const gnxr_light *in, std::vector<DLight> *lights, std::vector<gnxr_light> *desc) {
    *lights = cs.lights;
    *desc = cs.desc_lights;
    for (int k = 0; k < n; ++k) {
        const int i = first + k;
        const gnxr_light &was = cs.desc_lights[i], &l = in[k];
        if (l.type != was.type) { set_error("light %d: the type of a light cannot change in place (%d -> %d); gnxr_scene_set_lights replaces the list", i, was.type, l.type); return GNXR_ERR_UNSUPPORTED; }
        if (l.type == GNXR_LIGHT_INFINITE) {
            if (memcmp(&l, &was, sizeof(gnxr_light)) != 0) { set_error("light %d: an INFINITE light does not change through gnxr_scene_update_lights (gnxr_scene_update_environment rebuilds its tables)", i); return GNXR_ERR_UNSUPPORTED; }
            continue;
        }
        Vec3 corners[3];
        int tri_leaf = -1;
        if (l.type == GNXR_LIGHT_AREA_TRI) {
            if (l.tri != was.tri) { set_error("light %d: the triangle of an area light cannot change in place (%d -> %d); gnxr_scene_set_lights replaces the list", i, was.tri, l.tri); return GNXR_ERR_UNSUPPORTED; }
            const DLight &cur = cs.lights[i];
            tri_leaf = cur.tri_leaf;
            corners[0] = Vec3(cur.p0[0], cur.p0[1], cur.p0[2]); corners[1] = Vec3(cur.p1[0], cur.p1[1], cur.p1[2]); corners[2] = Vec3(cur.p2[0], cur.p2[1], cur.p2[2]);
        }
        if (!compile_light(l, i, corners, tri_leaf, cs.world_bound, &(*lights)[i])) return GNXR_ERR_INVALID;
        (*desc)[i] = l;
    }
    return GNXR_OK;
}

extern "C" int gnxr_scene_update_lights(gnxr_scene *s, int32_t first_light, int32_t n_lights, const gnxr_light *lights) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_lights > 0 && !lights) { set_error("null light array"); return GNXR_ERR_INVALID; }
    const int64_t have = (int64_t)s->cs.desc_lights.size();   // (the live count: gnxr_scene_set_lights changes it)
    if (first_light < 0 || n_lights < 0 || (int64_t)first_light + n_lights > have) {
        set_error("light range [%d, %lld) outside the scene's %lld lights", first_light, (long long)first_light + n_lights, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_lights == 0) return GNXR_OK;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    // 1. the records into a copy (one set: every device holds the same tree and the same records)
    std::vector<DLight> recs;
    std::vector<gnxr_light> descs;
    if (int rc = build_light_update(s->cs, first_light, n_lights, lights, &recs, &descs)) return rc;
    // 2. the uploads; one that fails puts the host's records, still the old ones, back on the devices already written
    const int rc = s->apply_or_put_back([&](gnxr_scene *d, size_t) -> int {
        const hipError_t e = hipMemcpy(d->lights.p, recs.data(), recs.size() * sizeof(DLight), hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("HIP error: %s", hipGetErrorString(e)); return GNXR_ERR_RUNTIME; }
        return GNXR_OK;
    }, refit_world);
    if (rc) return rc;
    // 3. the host scene (the render plan reads desc_lights' n_samples) and a new light-selection table at the next render
    s->cs.lights = std::move(recs);
    s->cs.desc_lights = std::move(descs);
    for (size_t i = 0; i < s->n_copies(); ++i) s->copy(i)->grid_strategy = -1;
    return GNXR_OK;
}

// ---- materials.  Both edits build the tables compile_materials gives the edited description into a copy (MaterialEdit), write every copy of
// the scene with material_apply and only then make them the host scene's.

// the authoring-order tables of k_material_tris go to a (bound) device at the first material edit of the scene
static int material_tables(gnxr_scene *s) {
    if (s->mat_map.p) return GNXR_OK;
    const SceneFacts &cs = s->cs;
    int rc;
    if ((rc = s->mat_tri.upload(cs.tri_material)) || (rc = s->mat_own.upload(cs.tri_own_attr)) || (rc = s->mat_map.alloc(cs.mat_map.size()))) return rc;
    return GNXR_OK;
}

struct MaterialEdit {
    MaterialTables mt;
    std::vector<DSphere> spheres;         // DSphere::material follows its material's type (-1 for GNXR_MAT_NONE)
    const int32_t *ids = nullptr;         // gnxr_scene_set_triangle_materials: host copy of tri_material[first, first + n)
    int first = 0, n = 0;
};

// the state the host scene holds, in the form of an edit (what a failed upload puts back)
static MaterialEdit material_current(const SceneFacts &cs, int first, int n) {
    MaterialEdit e;
    e.mt.materials = cs.materials; e.mt.materials_single = cs.materials_single; e.mt.aov_albedo = cs.aov_albedo;
    e.mt.material_authored = cs.material_authored; e.mt.mat_map = cs.mat_map;
    e.spheres = cs.spheres;
    e.ids = n > 0 ? cs.tri_material.data() + first : nullptr; e.first = first; e.n = n;
    return e;
}

static std::vector<DSphere> material_spheres(const SceneFacts &cs, const std::vector<gnxr_material> &mats) {
    std::vector<DSphere> sp = cs.spheres;
    for (size_t i = 0; i < cs.sphere_material.size(); ++i) {
        const int m = cs.sphere_material[i];
        sp[i].material = (m >= 0 && mats[m].type == GNXR_MAT_NONE) ? -1 : m;
    }
    return sp;
}

// One copy's share of a material edit, on its (bound) device: the small tables over the device's (their buffers were sized for the worst
// case by upload_scene), the edited range of the authored ids, then one pass over the leaf-order triangles.  Everything is queued on st and
// waited for.  The device holds the only leaf-order tables, and DTri::prim is all the kernel needs of them.
static int material_apply(gnxr_scene *s, const MaterialEdit &e, hipStream_t st) {
    const SceneFacts &cs = s->cs;
    const size_t ni = e.mt.materials.size();
    if (int rc = material_tables(s)) return rc;
    if (ni + 1 > s->materials.n || ni + 1 > s->materials_single.n || ni > s->material_authored.n || e.mt.mat_map.size() > s->mat_map.n || e.mt.aov_albedo.size() > s->aov_albedo.n ||
        e.spheres.size() > s->spheres.n || (size_t)e.first + e.n > s->mat_tri.n) {
        set_error("material edit: %zu internal materials do not fit the scene's tables", ni);
        return GNXR_ERR_RUNTIME;
    }
    HIP_TRY(hipMemcpyAsync(s->materials.p + 1, e.mt.materials.data(), ni * sizeof(DMaterial), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->materials_single.p + 1, e.mt.materials_single.data(), ni * sizeof(DMaterial), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->aov_albedo.p, e.mt.aov_albedo.data(), e.mt.aov_albedo.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->material_authored.p, e.mt.material_authored.data(), ni * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->mat_map.p, e.mt.mat_map.data(), e.mt.mat_map.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->spheres.p, e.spheres.data(), e.spheres.size() * sizeof(DSphere), hipMemcpyHostToDevice, st));
    if (e.n > 0) HIP_TRY(hipMemcpyAsync(s->mat_tri.p + e.first, e.ids, (size_t)e.n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int nt = (int)cs.n_triangles;
    hipLaunchKernelGGL(matedit::k_material_tris, dim3(grid_for(nt)), dim3(refit::kB), 0, st, s->tris.p, s->tri_class.p, nt, (const int *)s->mat_tri.p,
                       (const unsigned char *)s->mat_own.p, reinterpret_cast<const int4 *>(s->mat_map.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return GNXR_OK;
}

// every copy takes the edit (the primary on the caller's stream); a copy that fails puts the host's state, still the old one, back on all
static int material_apply_all(gnxr_scene *s, const MaterialEdit &e, hipStream_t st) {
    return s->apply_or_put_back([&](gnxr_scene *d, size_t i) -> int { return material_apply(d, e, i == 0 ? st : nullptr); },
                                [&](gnxr_scene *d, size_t) -> int { return d->mat_map.p ? material_apply(d, material_current(s->cs, e.first, e.n), nullptr) : GNXR_OK; });
}

extern "C" int gnxr_scene_update_materials(gnxr_scene *s, int32_t first_material, int32_t n_materials, const gnxr_material *materials) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_materials > 0 && !materials) { set_error("null material array"); return GNXR_ERR_INVALID; }
    const int64_t have = (int64_t)s->cs.desc_materials.size();   // (the number of materials never changes)
    if (first_material < 0 || n_materials < 0 || (int64_t)first_material + n_materials > have) {
        set_error("material range [%d, %lld) outside the scene's %lld materials", first_material, (long long)first_material + n_materials, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_materials == 0) return GNXR_OK;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    SceneFacts &cs = s->cs;
    // 1. all records into a copy: a refusal leaves the scene as it was
    std::vector<gnxr_material> descs = cs.desc_materials;
    std::copy(materials, materials + n_materials, descs.begin() + first_material);
    MaterialEdit e;
    if (!compile_materials(descs.data(), (int)descs.size(), (int)cs.textures.size(), cs.sphere_material, cs.tri_material.data(), cs.tri_own_attr.data(), (int)cs.tri_material.size(),
                           nullptr, &e.mt))
        return GNXR_ERR_INVALID;
    e.spheres = material_spheres(cs, descs);
    // 2. every copy of the scene, 3. the host scene (the render plan derives the kernel set from cs.materials at every call)
    if (int rc = material_apply_all(s, e, nullptr)) return rc;
    e.mt.move_to(&cs);
    cs.desc_materials = std::move(descs);
    cs.spheres = std::move(e.spheres);
    return GNXR_OK;
}

extern "C" int gnxr_scene_set_triangle_materials(gnxr_scene *s, int32_t first_triangle, int32_t n_triangles, const int32_t *material, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (n_triangles > 0 && !material) { set_error("null material id array"); return GNXR_ERR_INVALID; }
    const int64_t have = (int64_t)s->cs.tri_material.size();
    if (first_triangle < 0 || n_triangles < 0 || (int64_t)first_triangle + n_triangles > have) {
        set_error("triangle range [%d, %lld) outside the scene's %lld triangles", first_triangle, (long long)first_triangle + n_triangles, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_triangles == 0) return GNXR_OK;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    int rc = s->bind();
    if (rc) return rc;
    SceneFacts &cs = s->cs;
    hipStream_t st = (hipStream_t)hip_stream;
    // the ids come to the host (one copy path for host and device memory, ordered after what the caller queued on its stream): which
    // authored materials triangles with attributes of their own use decides the attribute copies.  Validated before anything is written.
    std::vector<int32_t> ids((size_t)n_triangles);
    HIP_TRY(hipMemcpyAsync(ids.data(), material, ids.size() * sizeof(int32_t), hipMemcpyDefault, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int nm = (int)cs.desc_materials.size();
    for (int i = 0; i < n_triangles; ++i)
        if (ids[i] < -1 || ids[i] >= nm) { set_error("triangle %d: material %d outside [-1, %d)", first_triangle + i, ids[i], nm); return GNXR_ERR_INVALID; }
    std::vector<int32_t> tri_material = cs.tri_material;
    std::copy(ids.begin(), ids.end(), tri_material.begin() + first_triangle);
    MaterialEdit e;
    if (!compile_materials(cs.desc_materials.data(), nm, (int)cs.textures.size(), cs.sphere_material, tri_material.data(), cs.tri_own_attr.data(), (int)tri_material.size(), nullptr, &e.mt))
        return GNXR_ERR_INVALID;
    e.spheres = cs.spheres;
    e.ids = ids.data(); e.first = first_triangle; e.n = n_triangles;
    if ((rc = material_apply_all(s, e, st)) != GNXR_OK) return rc;
    e.mt.move_to(&cs);
    cs.tri_material = std::move(tri_material);
    return GNXR_OK;
}

// test hook: what the primary's device holds per triangle, back in authoring order
extern "C" int gnxr_scene_triangle_materials(gnxr_scene *s, int32_t *material_out, uint8_t *shade_class_out, int64_t capacity) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    const int nt = (int)s->cs.tri_material.size();
    if (!material_out || !shade_class_out || capacity < nt) return nt;
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    int rc = s->bind();
    if (rc) return rc;
    DevBuf<int32_t> d_mat;
    DevBuf<uint8_t> d_cls;
    if ((rc = d_mat.alloc(nt)) || (rc = d_cls.alloc(nt))) return rc;
    hipLaunchKernelGGL(matedit::k_material_gather, dim3(grid_for(nt)), dim3(refit::kB), 0, 0, (const DTri *)s->tris.p, (const unsigned char *)s->tri_class.p, nt,
                       (const int *)s->material_authored.p, d_mat.p, d_cls.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(material_out, d_mat.p, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(shade_class_out, d_cls.p, (size_t)nt, hipMemcpyDeviceToHost));
    return nt;
}

extern "C" int gnxr_scene_set_camera(gnxr_scene *s, const gnxr_camera *camera, int32_t camera_medium) {
    if (!s || !camera) { set_error("null argument"); return GNXR_ERR_INVALID; }
    const int n_media = (int)s->cs.media.size();
    // as gnxr_scene_create: -1 == none; without media any value means none
    if (n_media > 0 && (camera_medium < -1 || camera_medium >= n_media)) { set_error("camera_medium %d out of range (%d media)", camera_medium, n_media); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    s->cs.camera = *camera;
    s->cs.camera_medium = n_media > 0 ? camera_medium : -1;
    return GNXR_OK;
}
