// api_rebuild.hip.h -- gnxr_scene_rebuild_bvh: host driver of the in-place rebuild (rebuild_kernel.hip.h).  Part of api.hip's translation
// unit (after api_edit.hip.h: the rebuild keeps the refit's tables, refit_tables, current).
//
// Every device of the handle builds into FRESH buffers (rebuild_on_device); only when all of them have reported clean flags and the same
// tree are the buffers swapped into the copies (rebuild_commit_copy, pointer swaps only; the one device write that could still fail, the
// DTexTables record, is made before them: rebuild_point_tables) and the host scene told its facts once (rebuild_commit_host), so a refused or failed
// call leaves the scene as it was.  What crosses to the host:
// the six floats of the centroid bounds, the run / treelet / level counts of the HLBVH stage, the node counts, and the result scalars
// (rebuild::R_*); and the DLight records, whose host copy refit_world uploads again after the next gnxr_scene_update_vertices (and from
// which gnxr_scene_update_lights takes an area light's corners and tri_leaf).
#pragma once

namespace {

template <typename T>
void swap_buf(DevBuf<T> &a, DevBuf<T> &b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }

struct Rebuilt {
    DevBuf<DNode> nodes;
    DevBuf<DNode4> nodes4;
    DevBuf<DTri> tris;
    DevBuf<float> leaf_boxes, tri_uv, tri_n, tri_s;
    DevBuf<uint8_t> tri_class;
    DevBuf<int32_t> tri_media, corner, parent, node4_src;
    DevBuf<unsigned int> arrived;
    DevBuf<DLight> lights;
    std::vector<DLight> h_lights;
    int n_nodes = 0, n_nodes4 = 0, root4 = 0, stack4_need = 1, max_depth = 0, leaf1_from_verts = 1;
    bool leaf_over_127 = false;
    // the result scalars: what the host scene records of a tree.  Every device builds the same one.
    bool same_tree(const Rebuilt &o) const {
        return n_nodes == o.n_nodes && n_nodes4 == o.n_nodes4 && root4 == o.root4 && stack4_need == o.stack4_need && max_depth == o.max_depth &&
               leaf1_from_verts == o.leaf1_from_verts && leaf_over_127 == o.leaf_over_127;
    }
};

// What a rebuild reads: the per-triangle tables of n triangles on the (bound) device, in any order that DTri::prim numbers 0 .. n - 1 --
// the scene's own in leaf order (rebuild_source_of), or gnxr_scene_set_geometry's in authoring order (api_geometry.hip.h).  Absent tables
// are null.  lights: the scene's DLight records with tri_leaf counting rows of `tris`; refit_lights: the AREA_TRI records take corners, area
// and normal from their triangles (k_refit_lights) instead of keeping them.
struct RebuildSource {
    int n = 0;
    const DTri *tris = nullptr;
    const uint8_t *tri_class = nullptr;
    const int32_t *corner = nullptr, *tri_media = nullptr;
    const float *tri_uv = nullptr, *tri_n = nullptr, *tri_s = nullptr;
    const DLight *lights = nullptr;
    bool refit_lights = false;
};
// the tables `s` holds (the refit's corner table goes to the device first; after a rebuild the device's is the only one)
int rebuild_source_of(gnxr_scene *s, RebuildSource *src) {
    const SceneFacts &cs = s->cs;
    if (int rc = refit_tables(s)) return rc;
    src->n = (int)cs.n_triangles;
    src->tris = s->tris.p; src->tri_class = s->tri_class.p; src->corner = s->upd_corner.p;
    src->tri_media = cs.has_tri_media ? s->tri_media.p : nullptr;
    src->tri_uv = cs.has_tri_uv ? s->tri_uv.p : nullptr;
    src->tri_n = cs.has_tri_n ? s->tri_n.p : nullptr;
    src->tri_s = cs.has_tri_s ? s->tri_s.p : nullptr;
    src->lights = s->lights.p;
    return GNXR_OK;
}

// the tree over the triangles of `src` on the (bound) device of `s`, into `r`; nothing of `s` changes
int rebuild_on_device(gnxr_scene *s, const RebuildSource &src, hipStream_t st, Rebuilt *r) {
    using namespace rebuild;
    const SceneFacts &cs = s->cs;
    const int n = src.n;
    const int n_lights = (int)cs.desc_lights.size();
    int rc;
    const auto fetch = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };
    // ---- primitive bounds, centroids and their bounds
    DevBuf<float> pb, cen;
    DevBuf<int> old_of_prim, new_of_old, res;
    DevBuf<uint32_t> cb;
    if ((rc = pb.alloc(6 * (size_t)n)) || (rc = cen.alloc(3 * (size_t)n)) || (rc = old_of_prim.alloc(n)) || (rc = new_of_old.alloc(n)) || (rc = cb.alloc(6)) || (rc = res.alloc(R_COUNT)))
        return rc;
    const float FMAX = 3.402823466e+38f;
    uint32_t h_cb[6];
    for (int k = 0; k < 3; ++k) { h_cb[k] = float_to_ordered(FMAX); h_cb[3 + k] = float_to_ordered(-FMAX); }
    int h_res[R_COUNT] = {0};
    h_res[R_STACK4_NEED] = 1;
    HIP_TRY(hipMemcpyAsync(cb.p, h_cb, sizeof(h_cb), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(res.p, h_res, sizeof(h_res), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(old_of_prim.p, 0xff, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL(k_rb_prims, dim3(grid_for(n)), dim3(kB), 0, st, src.tris, n, pb.p, cen.p, old_of_prim.p, cb.p, res.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fetch(h_cb, cb.p, sizeof(h_cb)));
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = ordered_to_float(h_cb[k]); hi[k] = ordered_to_float(h_cb[3 + k]); }
    // ---- the HLBVH stage
    HlbvhDevice hb;
    if ((rc = device_hlbvh_core(pb.p, cen.p, n, lo, hi, st, &hb)) != GNXR_OK) return rc;
    const int U = hb.U, cap = (int)hb.cap, N = 2 * U - 1;
    // ---- flatten
    DevBuf<int> par, size;
    DevBuf<unsigned int> arrived;
    DevBuf<unsigned char> choice, is_root4;
    DevBuf<WideCost> cost;
    DevBuf<uint32_t> id4, sums, total;
    if ((rc = par.alloc(cap)) || (rc = size.alloc(cap)) || (rc = arrived.alloc(cap)) || (rc = choice.alloc(N)) || (rc = is_root4.alloc(N)) || (rc = cost.alloc(N)) || (rc = id4.alloc(N)) ||
        (rc = sums.alloc((size_t)(N + hlbvh::kTile - 1) / hlbvh::kTile + 2)) || (rc = total.alloc(1)) || (rc = r->nodes.alloc(N)) || (rc = r->parent.alloc(N)) ||
        (rc = r->arrived.alloc(N)) || (rc = r->leaf_boxes.alloc(8 * (size_t)n)))
        return rc;
    HIP_TRY(hipMemsetAsync(par.p, 0xff, (size_t)cap * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(size.p, 0, (size_t)cap * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(arrived.p, 0, (size_t)cap * sizeof(unsigned int), st));
    HIP_TRY(hipMemsetAsync(id4.p, 0, (size_t)N * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(choice.p, 0, (size_t)N, st));
    HIP_TRY(hipMemsetAsync(is_root4.p, 0, (size_t)N, st));
    HIP_TRY(hipMemsetAsync(cost.p, 0, (size_t)N * sizeof(WideCost), st));
    HIP_TRY(hipMemsetAsync(r->arrived.p, 0, (size_t)N * sizeof(unsigned int), st));
    HIP_TRY(hipMemsetAsync(r->nodes.p, 0, (size_t)N * sizeof(DNode), st));
    HIP_TRY(hipMemsetAsync(r->parent.p, 0xff, (size_t)N * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(r->leaf_boxes.p, 0, 8 * (size_t)n * sizeof(float), st));
    hipLaunchKernelGGL(k_rb_parents, dim3(grid_for(cap)), dim3(kB), 0, st, (const HlbvhNode *)hb.d_nodes.p, U, cap, par.p, res.p);
    hipLaunchKernelGGL(k_rb_sizes, dim3(grid_for(U)), dim3(kB), 0, st, U, cap, (const HlbvhNode *)hb.d_nodes.p, (const int *)par.p, arrived.p, size.p, res.p);
    hipLaunchKernelGGL(k_rb_flatten, dim3(grid_for(cap)), dim3(kB), 0, st, U, cap, hb.root, N, n, (const HlbvhNode *)hb.d_nodes.p, (const int *)par.p, (const int *)size.p, r->nodes.p,
                       r->parent.p, r->leaf_boxes.p, res.p);
    // the cuts of the 4-wide tree (wide_collapse.h): costs bottom-up, then which nodes are DNode4s; r->arrived serves as the counters (the
    // refit clears it before every use)
    hipLaunchKernelGGL(k_rb_cost, dim3(grid_for(N)), dim3(kB), 0, st, N, (const DNode *)r->nodes.p, (const int *)r->parent.p, r->arrived.p, cost.p, choice.p);
    hipLaunchKernelGGL(k_rb_cuts, dim3(grid_for(N)), dim3(kB), 0, st, N, (const DNode *)r->nodes.p, (const int *)r->parent.p, (const unsigned char *)choice.p, id4.p, is_root4.p, res.p);
    hl_scan(id4.p, N, sums.p, total.p, st);
    HIP_TRY(hipGetLastError());
    uint32_t n4 = 0;
    HIP_TRY(hipMemcpyAsync(&n4, total.p, sizeof(n4), hipMemcpyDeviceToHost, st));
    HIP_TRY(fetch(h_res, res.p, sizeof(h_res)));
    if (h_res[R_ERROR] || n4 > (uint32_t)N) { set_error("BVH rebuild: the build tree is not a tree (internal error)"); return GNXR_ERR_RUNTIME; }
    if (h_res[R_MAX_DEPTH] + 1 > 64) { set_error("BVH depth %d exceeds the 64-entry traversal stack (BVHAccel.cpp:661)", h_res[R_MAX_DEPTH]); return GNXR_ERR_UNSUPPORTED; }
    r->n_nodes = N;
    r->max_depth = h_res[R_MAX_DEPTH];
    // ---- the 4-wide tree
    DevBuf<DNode4> tmp4;
    DevBuf<int> src_tmp, new_of;
    DevBuf<uint32_t> placed;
    if (n4 == 0) {   // a single leaf: the root reference is the leaf, the table one blank node
        if ((rc = r->nodes4.alloc(1)) || (rc = r->node4_src.alloc(4))) return rc;
        HIP_TRY(hipMemsetAsync(r->nodes4.p, 0, sizeof(DNode4), st));
        HIP_TRY(hipMemsetAsync(r->node4_src.p, 0xff, 4 * sizeof(int32_t), st));
        r->n_nodes4 = 1;
        r->root4 = ~(int32_t)(0u | (((uint32_t)n & 0x7fu) << 24));   // leaf_ref of the root: first triangle 0, n primitives
    } else {
        if ((rc = tmp4.alloc(n4)) || (rc = src_tmp.alloc(4 * (size_t)n4)) || (rc = new_of.alloc(n4)) || (rc = placed.alloc(n4)) || (rc = r->nodes4.alloc(n4)) ||
            (rc = r->node4_src.alloc(4 * (size_t)n4)))
            return rc;
        HIP_TRY(hipMemsetAsync(new_of.p, 0xff, (size_t)n4 * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(placed.p, 0, (size_t)n4 * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(r->nodes4.p, 0, (size_t)n4 * sizeof(DNode4), st));
        HIP_TRY(hipMemsetAsync(r->node4_src.p, 0xff, 4 * (size_t)n4 * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_rb_collapse, dim3(grid_for(N)), dim3(kB), 0, st, N, (const DNode *)r->nodes.p, (const unsigned char *)choice.p, (const unsigned char *)is_root4.p,
                           (const uint32_t *)id4.p, (int)n4, tmp4.p, src_tmp.p, res.p);
        hipLaunchKernelGGL(k_rb_bfs, dim3(1), dim3(kTopNodesMax), 0, st, (const DNode4 *)tmp4.p, (int)n4, new_of.p, placed.p, res.p);
        hl_scan(placed.p, (int)n4, sums.p, nullptr, st);
        hipLaunchKernelGGL(k_rb_renumber, dim3(grid_for(n4)), dim3(kB), 0, st, (int)n4, (const DNode4 *)tmp4.p, (const int *)src_tmp.p, (const int *)new_of.p,
                           (const uint32_t *)placed.p, r->nodes4.p, r->node4_src.p, res.p);
        r->n_nodes4 = (int)n4;
        r->root4 = 0;   // the root is the first node of the breadth-first block
    }
    // ---- everything held in leaf order
    const bool has_media = src.tri_media != nullptr, has_uv = src.tri_uv != nullptr, has_n = src.tri_n != nullptr, has_s = src.tri_s != nullptr;
    if ((rc = r->tris.alloc(n)) || (rc = r->tri_class.alloc(n)) || (rc = r->corner.alloc(3 * (size_t)n)) || (has_media && (rc = r->tri_media.alloc(2 * (size_t)n))) ||
        (has_uv && (rc = r->tri_uv.alloc(8 * (size_t)n))) || (has_n && (rc = r->tri_n.alloc(12 * (size_t)n))) || (has_s && (rc = r->tri_s.alloc(12 * (size_t)n))) ||
        (rc = r->lights.alloc(cs.lights.size())))
        return rc;
    LeafTables lt;
    lt.tris = src.tris; lt.tri_class = src.tri_class; lt.corner = src.corner;
    lt.tri_media = reinterpret_cast<const int2 *>(src.tri_media);
    lt.tri_uv = reinterpret_cast<const float4 *>(src.tri_uv); lt.tri_n = reinterpret_cast<const float4 *>(src.tri_n); lt.tri_s = reinterpret_cast<const float4 *>(src.tri_s);
    lt.tris_out = r->tris.p; lt.tri_class_out = r->tri_class.p; lt.corner_out = r->corner.p;
    lt.tri_media_out = reinterpret_cast<int2 *>(r->tri_media.p);
    lt.tri_uv_out = reinterpret_cast<float4 *>(r->tri_uv.p); lt.tri_n_out = reinterpret_cast<float4 *>(r->tri_n.p); lt.tri_s_out = reinterpret_cast<float4 *>(r->tri_s.p);
    HIP_TRY(hipMemsetAsync(new_of_old.p, 0xff, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL(k_rb_permute, dim3(grid_for(n)), dim3(kB), 0, st, n, hb.prims, (const int *)old_of_prim.p, lt, new_of_old.p, res.p);
    HIP_TRY(hipMemcpyAsync(r->lights.p, src.lights, cs.lights.size() * sizeof(DLight), hipMemcpyDeviceToDevice, st));
    if (n_lights > 0) hipLaunchKernelGGL(k_rb_lights, dim3(grid_for(n_lights)), dim3(kB), 0, st, r->lights.p, n_lights, n, (const int *)new_of_old.p, res.p);
    if (n_lights > 0 && src.refit_lights) hipLaunchKernelGGL(refit::k_refit_lights, dim3(grid_for(n_lights)), dim3(refit::kB), 0, st, r->lights.p, n_lights, (const DTri *)r->tris.p, n);
    hipLaunchKernelGGL(k_rb_leafcheck, dim3(grid_for(N)), dim3(kB), 0, st, N, (const DNode *)r->nodes.p, (const DTri *)r->tris.p, n, res.p);
    HIP_TRY(hipGetLastError());
    r->h_lights.resize(cs.lights.size());
    HIP_TRY(hipMemcpyAsync(r->h_lights.data(), r->lights.p, cs.lights.size() * sizeof(DLight), hipMemcpyDeviceToHost, st));
    HIP_TRY(fetch(h_res, res.p, sizeof(h_res)));
    if (h_res[R_ERROR] || (n4 > 0 && h_res[R_N_TOP] != (int)std::min<uint32_t>(n4, (uint32_t)kTopNodesMax))) {
        set_error("BVH rebuild: inconsistent 4-wide tree or primitive order (internal error)");
        return GNXR_ERR_RUNTIME;
    }
    r->stack4_need = h_res[R_STACK4_NEED];
    r->leaf1_from_verts = h_res[R_LEAF1_MISMATCH] ? 0 : 1;
    r->leaf_over_127 = h_res[R_LEAF_OVER_127] != 0;
    return GNXR_OK;
}

// The record in front of the materials (DTexTables) points at the per-corner tables: written BEFORE the swap, towards the buffers the swap
// will bring in (to_new) or back towards the ones the scene holds (undo), so that the swap itself cannot fail.
bool rebuild_has_attrs(const Rebuilt &r) { return r.tri_uv.p || r.tri_n.p || r.tri_s.p; }
int rebuild_point_tables(gnxr_scene *s, const Rebuilt &r, bool to_new) {
    if (!rebuild_has_attrs(r)) return GNXR_OK;
    const DTexTables at = to_new ? s->tex_tables(r.tri_uv.p, r.tri_n.p, r.tri_s.p) : s->tex_tables(s->tri_uv.p, s->tri_n.p, s->tri_s.p);
    return s->write_material_tables(s->cs.materials, s->cs.materials_single, at.tri_uv, at.tri_n, at.tri_s);   // (the materials stay what they are)
}

// The new tree into the scene, in two steps that cannot fail.  First the host scene, once, from the primary's result: the facts of the
// tree (the tables themselves exist on the devices only).
void rebuild_commit_host(gnxr_scene *s, Rebuilt &r) {
    SceneFacts &cs = s->cs;
    cs.n_nodes = (size_t)r.n_nodes; cs.n_nodes4 = (size_t)r.n_nodes4;
    cs.root4 = r.root4; cs.stack4_need = r.stack4_need; cs.bvh_max_depth = r.max_depth; cs.leaf1_from_verts = r.leaf1_from_verts;
    cs.lights = std::move(r.h_lights);
}
// ... then every copy's tables: pointer swaps, and what the copy derives from the host scene
void rebuild_commit_copy(gnxr_scene *s, Rebuilt &r) {
    swap_buf(s->nodes, r.nodes); swap_buf(s->nodes4, r.nodes4); swap_buf(s->tris, r.tris); swap_buf(s->leaf_boxes, r.leaf_boxes); swap_buf(s->tri_class, r.tri_class);
    swap_buf(s->lights, r.lights);
    if (r.tri_media.p) swap_buf(s->tri_media, r.tri_media);
    if (r.tri_uv.p) swap_buf(s->tri_uv, r.tri_uv);
    if (r.tri_n.p) swap_buf(s->tri_n, r.tri_n);
    if (r.tri_s.p) swap_buf(s->tri_s, r.tri_s);
    // the refit's tables were just computed for the new tree: they go in directly
    swap_buf(s->upd_corner, r.corner); swap_buf(s->upd_parent, r.parent); swap_buf(s->upd_node4_src, r.node4_src); swap_buf(s->upd_arrived, r.arrived);
    s->set_traversal(r.leaf_over_127);
    s->grid_strategy = -1;
}

}  // namespace

extern "C" int gnxr_scene_rebuild_bvh(gnxr_scene *s, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    int rc = s->bind();
    if (rc) return rc;
    // 1. every device builds into fresh buffers (the primary on the caller's stream), and all must have built the same tree
    std::vector<Rebuilt> built(s->n_copies());
    if ((rc = s->each_copy([&](gnxr_scene *c, size_t i) -> int {
            RebuildSource src;
            if (int rc_ = rebuild_source_of(c, &src)) return rc_;
            return rebuild_on_device(c, src, i == 0 ? (hipStream_t)hip_stream : nullptr, &built[i]);
        })))
        return rc;
    for (size_t i = 1; i < built.size(); ++i)
        if (!built[i].same_tree(built[0])) { set_error("BVH rebuild: the devices disagree (internal error)"); return GNXR_ERR_RUNTIME; }
    // 2. the only writes that can still fail; a failure points every record back at the tables the scene holds
    if ((rc = s->apply_or_put_back([&](gnxr_scene *c, size_t i) { return rebuild_point_tables(c, built[i], /*to_new=*/true); },
                                   [&](gnxr_scene *c, size_t i) { return rebuild_point_tables(c, built[i], /*to_new=*/false); })))
        return rc;
    // 3. the host scene, then the swaps
    rebuild_commit_host(s, built[0]);
    for (size_t i = 0; i < s->n_copies(); ++i) rebuild_commit_copy(s->copy(i), built[i]);
    // the old tables are released with `built` (hipFree waits for what still reads them)
    return GNXR_OK;
}

extern "C" int gnxr_scene_bvh4(const gnxr_scene *sc, void *nodes128, int64_t node_capacity, int64_t *n_nodes4, int32_t *root4, int32_t *stack_need) {
    if (!sc || !n_nodes4) { set_error("bad argument"); return GNXR_ERR_INVALID; }
    gnxr_scene *s = const_cast<gnxr_scene *>(sc);
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    *n_nodes4 = (int64_t)s->cs.n_nodes4;
    if (root4) *root4 = s->cs.root4;
    if (stack_need) *stack_need = s->cs.stack4_need;
    if (!nodes128 || node_capacity < *n_nodes4) return GNXR_OK;
    if (int rc = s->bind()) return rc;
    HIP_TRY(hipMemcpy(nodes128, s->nodes4.p, s->cs.n_nodes4 * sizeof(DNode4), hipMemcpyDeviceToHost));
    return GNXR_OK;
}
