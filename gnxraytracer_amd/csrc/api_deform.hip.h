// api_deform.hip.h -- deforming smooth meshes in place: gnxr_scene_update_attributes / gnxr_scene_triangle_attributes (per-corner uvs,
// shading normals and tangents of a live scene), gnxr_scene_recompute_normals (area-weighted normals from the vertices the scene holds) and
// gnxr_skin_vertices_device (linear-blend skinning, no scene involved).  The definitions: include/gnxr.h; the kernels: deform_kernel.hip.h.
// Part of api.hip's translation unit (after api_geometry.hip.h: geometry_side, swap_buf).  The scene edits follow api_edit.hip.h: under
// the primary's render_mutex, the primary on the caller's stream, then one loop over the other copies.
#pragma once

namespace {

// the scene's per-corner tables as the kernels see them (an empty upload still allocates: the host scene decides what exists)
deform::AttrTables attr_tables(gnxr_scene *s) {
    const SceneFacts &cs = s->cs;
    deform::AttrTables t;
    t.uv = cs.has_tri_uv ? reinterpret_cast<float4 *>(s->tri_uv.p) : nullptr;
    t.n = cs.has_tri_n ? reinterpret_cast<float4 *>(s->tri_n.p) : nullptr;
    t.s = cs.has_tri_s ? reinterpret_cast<float4 *>(s->tri_s.p) : nullptr;
    return t;
}

// the caller's rows on one device: the caller's own pointers, or copies the call owns (host rows -> the bound device, queued on st)
struct AttrStage {
    deform::AttrRows rows;
    DevBuf<float> uv, n, s;
    int stage(const float *h_uv, const float *h_n, const float *h_s, int first, int count, hipStream_t st) {
        rows.first = first; rows.count = count; rows.uv = rows.n = rows.s = nullptr;
        const size_t c = (size_t)count;
        int rc;
        if (h_uv) { if ((rc = uv.alloc(6 * c))) return rc; HIP_TRY(hipMemcpyAsync(uv.p, h_uv, 6 * c * sizeof(float), hipMemcpyHostToDevice, st)); rows.uv = uv.p; }
        if (h_n) { if ((rc = n.alloc(9 * c))) return rc; HIP_TRY(hipMemcpyAsync(n.p, h_n, 9 * c * sizeof(float), hipMemcpyHostToDevice, st)); rows.n = n.p; }
        if (h_s) { if ((rc = s.alloc(9 * c))) return rc; HIP_TRY(hipMemcpyAsync(s.p, h_s, 9 * c * sizeof(float), hipMemcpyHostToDevice, st)); rows.s = s.p; }
        return GNXR_OK;
    }
};

// The vertex -> corner table of the copy's mesh on its (bound) device, built once per topology: corner ids 3 t + k in authoring numbering,
// so a rebuild of the tree leaves it valid; gnxr_scene_set_geometry releases it.  Counts by integer atomics, offsets by the HLBVH stage's
// scan, the order within a vertex by its stable radix sort keyed by the vertex index (6 bits per pass, as many passes as the vertex count
// needs).  Everything is queued on st; the table becomes the copy's only when all of it has been queued without an error.
int normals_adjacency(gnxr_scene *s, hipStream_t st) {
    using namespace hlbvh;
    if (s->adj_offsets.p) return GNXR_OK;
    const SceneFacts &cs = s->cs;
    const long long n_tris = (long long)cs.n_triangles, n_corners = 3 * n_tris;
    const int V = cs.n_vertices;
    if (n_corners > 0x7fffffffLL) { set_error("recompute_normals: %lld corners exceed the sort's 2^31 - 1 items", n_corners); return GNXR_ERR_UNSUPPORTED; }
    const int n = (int)n_corners, n_tiles = (n + kTile - 1) / kTile;
    DevBuf<uint32_t> offsets, k_a, k_b, v_a, v_b, hist, sums;
    int rc;
    if ((rc = offsets.alloc((size_t)V + 1)) || (rc = k_a.alloc(n)) || (rc = k_b.alloc(n)) || (rc = v_a.alloc(n)) || (rc = v_b.alloc(n)) || (rc = hist.alloc((size_t)64 * n_tiles)) ||
        (rc = sums.alloc((size_t)std::max((V + 1 + kTile - 1) / kTile, (64 * n_tiles + kTile - 1) / kTile) + 1)))
        return rc;
    HIP_TRY(hipMemsetAsync(offsets.p, 0, ((size_t)V + 1) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(deform::k_adj_corners, dim3(grid_for(n_tris)), dim3(deform::kB), 0, st, (const DTri *)s->tris.p, (const int *)s->upd_corner.p, (int)n_tris, V, k_a.p, v_a.p, offsets.p);
    hl_scan(offsets.p, V + 1, sums.p, nullptr, st);   // counts -> offsets[0 .. V]; offsets[V] = the number of corners
    int bits = 0;
    while (bits < 32 && ((unsigned long long)(V > 0 ? V - 1 : 0) >> bits) != 0ull) ++bits;
    uint32_t *kin = k_a.p, *kout = k_b.p, *vin = v_a.p, *vout = v_b.p;
    for (int shift = 0; shift < bits; shift += 6) {
        hipLaunchKernelGGL(k_rs_hist, dim3(n_tiles), dim3(kB), 0, st, (const uint32_t *)kin, n, shift, n_tiles, hist.p);
        hl_scan(hist.p, 64 * n_tiles, sums.p, nullptr, st);
        hipLaunchKernelGGL(k_rs_scatter, dim3(n_tiles), dim3(kB), 0, st, (const uint32_t *)kin, (const uint32_t *)vin, n, shift, n_tiles, (const uint32_t *)hist.p, kout, vout);
        std::swap(kin, kout); std::swap(vin, vout);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    swap_buf(s->adj_offsets, offsets);
    swap_buf(s->adj_corners, vin == v_a.p ? v_a : v_b);
    return GNXR_OK;
}

// one copy's normals on its (bound) device, queued on st and waited for
int normals_apply(gnxr_scene *s, float sign, hipStream_t st) {
    const SceneFacts &cs = s->cs;
    const int n_tris = (int)cs.n_triangles, V = cs.n_vertices;
    int rc;
    if ((rc = refit_tables(s)) || (rc = normals_adjacency(s, st)) || (rc = s->nrm_face.alloc(n_tris)) || (rc = s->nrm_vsum.alloc(V))) return rc;
    float4 *tri_n = reinterpret_cast<float4 *>(s->tri_n.p);
    hipLaunchKernelGGL(deform::k_face_normals, dim3(grid_for(n_tris)), dim3(deform::kB), 0, st, (const DTri *)s->tris.p, n_tris, (const float4 *)tri_n, sign, s->nrm_face.p);
    hipLaunchKernelGGL(deform::k_vertex_normals, dim3(grid_for(V)), dim3(deform::kB), 0, st, V, (const uint32_t *)s->adj_offsets.p, (const uint32_t *)s->adj_corners.p,
                       (const float4 *)s->nrm_face.p, s->nrm_vsum.p);
    hipLaunchKernelGGL(deform::k_write_normals, dim3(grid_for(n_tris)), dim3(deform::kB), 0, st, (const DTri *)s->tris.p, (const int *)s->upd_corner.p, n_tris, V,
                       (const float4 *)s->nrm_vsum.p, tri_n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return GNXR_OK;
}

}  // namespace

extern "C" {

int gnxr_scene_update_attributes(gnxr_scene *s, int32_t first_triangle, int32_t n_triangles, const float *tri_uv, const float *tri_n, const float *tri_s, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    const int64_t have = (int64_t)s->cs.tri_material.size();
    if (first_triangle < 0 || n_triangles < 0 || (int64_t)first_triangle + n_triangles > have) {
        set_error("triangle range [%d, %lld) outside the scene's %lld triangles", first_triangle, (long long)first_triangle + n_triangles, (long long)have);
        return GNXR_ERR_INVALID;
    }
    if (n_triangles == 0) return GNXR_OK;
    if (!tri_uv && !tri_n && !tri_s) { set_error("update_attributes: no array given"); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    int rc = s->bind();
    if (rc) return rc;
    const SceneFacts &cs = s->cs;
    // all arrays on one side (the rule of gnxr_scene_set_geometry)
    const void *arrays[] = {tri_uv, tri_n, tri_s};
    int side = -2;
    for (const void *p : arrays) {
        if (!p) continue;
        const int sd = geometry_side(p, s->device);
        if (sd < 0) { set_error("update_attributes: an array lives on another device than the scene's first device %d", s->device); return GNXR_ERR_INVALID; }
        if (side != -2 && sd != side) { set_error("update_attributes: the arrays are partly host memory, partly device memory"); return GNXR_ERR_INVALID; }
        side = sd;
        if (sd == 1) {   // device rows are read where they lie: they must lie inside their allocation
            const size_t bytes = (size_t)n_triangles * (p == (const void *)tri_uv ? 6 : 9) * sizeof(float);
            hipDeviceptr_t base = nullptr;
            size_t size_b = 0;
            if (hipMemGetAddressRange(&base, &size_b, (hipDeviceptr_t)p) == hipSuccess && base && (const char *)p + bytes > (const char *)base + size_b) {
                set_error("update_attributes: %zu bytes from %p run past the end of their allocation (%zu bytes from %p)", bytes, p, size_b, (void *)base);
                return GNXR_ERR_INVALID;
            }
            (void)hipGetLastError();
            if (((uintptr_t)p & 3u) != 0) { set_error("update_attributes: a device array is not 4-byte aligned"); return GNXR_ERR_INVALID; }
        }
    }
    if ((tri_uv && !cs.has_tri_uv) || (tri_n && !cs.has_tri_n) || (tri_s && !cs.has_tri_s)) {
        set_error("update_attributes: the scene was created without per-corner %s (gnxr_scene_set_geometry adds the table)", tri_uv && !cs.has_tri_uv ? "uvs" : tri_n && !cs.has_tri_n ? "normals" : "tangents");
        return GNXR_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int nt = (int)cs.n_triangles;
    // the primary: rows staged (or read where they lie, behind what the caller queued on st), refusals first, then the write
    AttrStage prim;
    if (side == 0) { if ((rc = prim.stage(tri_uv, tri_n, tri_s, first_triangle, n_triangles, st)) != GNXR_OK) return rc; }
    else { prim.rows.uv = tri_uv; prim.rows.n = tri_n; prim.rows.s = tri_s; prim.rows.first = first_triangle; prim.rows.count = n_triangles; }
    if ((rc = s->attr_flag.alloc(1)) != GNXR_OK) return rc;
    int h_flag = 0;
    HIP_TRY(hipMemsetAsync(s->attr_flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL((deform::k_attr_edit<false>), dim3(grid_for(nt)), dim3(deform::kB), 0, st, (const DTri *)s->tris.p, nt, attr_tables(s), prim.rows, s->attr_flag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_flag, s->attr_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flag & (deform::A_EMISSIVE_NORMALS | deform::A_EMISSIVE_TANGENTS)) {
        set_error("update_attributes: per-vertex %s on an emissive triangle are not supported", (h_flag & deform::A_EMISSIVE_NORMALS) ? "normals" : "tangents");
        return GNXR_ERR_UNSUPPORTED;
    }
    if (h_flag & deform::A_OWN_CHANGES) {
        set_error("update_attributes: a triangle would gain or lose attributes of its own (uvs other than the defaults, a non-zero normal or tangent row): that "
                  "changes its material copy and shade class; gnxr_scene_set_geometry does it");
        return GNXR_ERR_UNSUPPORTED;
    }
    // the rows for the other copies come to the host before anything is written (the last step that can fail for a reason of the caller's)
    std::vector<float> h_uv, h_n, h_s;
    const float *r_uv = tri_uv, *r_n = tri_n, *r_s = tri_s;
    if (s->n_copies() > 1 && side == 1) {
        const size_t c = (size_t)n_triangles;
        if (tri_uv) { h_uv.resize(6 * c); HIP_TRY(hipMemcpy(h_uv.data(), tri_uv, 6 * c * sizeof(float), hipMemcpyDeviceToHost)); r_uv = h_uv.data(); }
        if (tri_n) { h_n.resize(9 * c); HIP_TRY(hipMemcpy(h_n.data(), tri_n, 9 * c * sizeof(float), hipMemcpyDeviceToHost)); r_n = h_n.data(); }
        if (tri_s) { h_s.resize(9 * c); HIP_TRY(hipMemcpy(h_s.data(), tri_s, 9 * c * sizeof(float), hipMemcpyDeviceToHost)); r_s = h_s.data(); }
    }
    return s->each_copy([&](gnxr_scene *c, size_t i) -> int {
        AttrStage rep;
        const deform::AttrRows *rows = &prim.rows;
        hipStream_t cst = i == 0 ? st : nullptr;
        if (i > 0) { if (int rc_ = rep.stage(r_uv, r_n, r_s, first_triangle, n_triangles, cst)) return rc_; rows = &rep.rows; }
        hipLaunchKernelGGL((deform::k_attr_edit<true>), dim3(grid_for(nt)), dim3(deform::kB), 0, cst, (const DTri *)c->tris.p, nt, attr_tables(c), *rows, (int *)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(cst));
        return GNXR_OK;
    });
}

// test hook: what the primary's device holds per triangle, back in authoring order and unpadded (which: 0 uv, 6 floats per triangle;
// 1 normals, 2 tangents, 9 each).  *n_floats: the size of the table, 0 where the scene has none
int gnxr_scene_triangle_attributes(gnxr_scene *s, int32_t which, float *out, int64_t capacity_floats, int64_t *n_floats) {
    if (!s || !n_floats) { set_error("null argument"); return GNXR_ERR_INVALID; }
    if (which < 0 || which > 2) { set_error("triangle_attributes: which = %d (0 uv, 1 normals, 2 tangents)", which); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    const SceneFacts &cs = s->cs;
    const deform::AttrTables tab = attr_tables(s);
    const float4 *table = which == 0 ? tab.uv : which == 1 ? tab.n : tab.s;
    const int nt = (int)cs.n_triangles;
    const int64_t n = table ? (int64_t)nt * (which == 0 ? 6 : 9) : 0;
    *n_floats = n;
    if (!out || capacity_floats < n || n == 0) return GNXR_OK;
    int rc = s->bind();
    if (rc) return rc;
    DevBuf<float> d_out;
    if ((rc = d_out.alloc((size_t)n)) != GNXR_OK) return rc;
    hipLaunchKernelGGL(deform::k_attr_gather, dim3(grid_for(nt)), dim3(deform::kB), 0, 0, (const DTri *)s->tris.p, nt, (int)which, table, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return GNXR_OK;
}

int gnxr_scene_recompute_normals(gnxr_scene *s, uint32_t flags, void *hip_stream) {
    if (!s) { set_error("null scene"); return GNXR_ERR_INVALID; }
    if (flags & ~(uint32_t)GNXR_NORMALS_FLIP) { set_error("unknown normals flags 0x%x", flags); return GNXR_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lock(s->render_mutex);
    if (!s->cs.has_tri_n) return GNXR_OK;   // no smooth triangle anywhere
    const float sign = (flags & GNXR_NORMALS_FLIP) ? -1.f : 1.f;
    // every copy computes its own: the same vertices, the same order of every sum, the same bits
    return s->each_copy([&](gnxr_scene *c, size_t i) -> int { return normals_apply(c, sign, i == 0 ? (hipStream_t)hip_stream : nullptr); });
}

int gnxr_skin_vertices_device(const gnxr_skin_params *p, const float *d_rest, const int32_t *d_bone_index, const float *d_bone_weight, const float *d_bones,
                              const float *d_morph_delta, const float *d_morph_weight, float *d_out, void *hip_stream) {
    if (!p) { set_error("skin vertices: null argument"); return GNXR_ERR_INVALID; }
    if (p->struct_size != (int32_t)sizeof(gnxr_skin_params)) { set_error("skin vertices: struct_size must be sizeof(gnxr_skin_params) = %zu", sizeof(gnxr_skin_params)); return GNXR_ERR_INVALID; }
    if (p->n_vertices < 0 || p->n_bones < 1 || p->n_morphs < 0) { set_error("skin vertices: n_vertices >= 0, n_bones >= 1 and n_morphs >= 0 are required"); return GNXR_ERR_INVALID; }
    if (!d_rest || !d_bone_index || !d_bone_weight || !d_bones || !d_out) { set_error("skin vertices: d_rest, d_bone_index, d_bone_weight, d_bones and d_out are required"); return GNXR_ERR_INVALID; }
    if (p->n_morphs > 0 && (!d_morph_delta || !d_morph_weight)) { set_error("skin vertices: n_morphs = %d without d_morph_delta and d_morph_weight", p->n_morphs); return GNXR_ERR_INVALID; }
    const size_t V = (size_t)p->n_vertices, B = (size_t)p->n_bones, M = (size_t)p->n_morphs;
    const int kArgs = 7;   // the output comes last
    const QueryArg args[kArgs] = {{d_rest, V * 12, "d_rest"}, {d_bone_index, V * 16, "d_bone_index"}, {d_bone_weight, V * 16, "d_bone_weight"}, {d_bones, B * 48, "d_bones"},
                                  {M ? d_morph_delta : nullptr, M * V * 12, "d_morph_delta"}, {M ? d_morph_weight : nullptr, M * 4, "d_morph_weight"}, {d_out, V * 12, "d_out"}};
    const unsigned align[kArgs] = {4u, 16u, 16u, 16u, 4u, 4u, 4u};   // the 16-byte rows: four indices, four weights, a matrix row
    if (int rc = check_aligned("skin vertices", args, align, kArgs)) return rc;
    if (V == 0) return GNXR_OK;
    for (int i = 0; i < kArgs - 1; ++i)
        if (ranges_overlap(args[i], args[kArgs - 1])) { set_error("skin vertices: d_out overlaps %s", args[i].what); return GNXR_ERR_INVALID; }
    if (int rc = ensure_device()) return rc;
    DeviceCall call;
    if (int rc = call.bind("skin vertices", args)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    StreamScratch scratch;   // the bad-index flag
    HIP_TRY(scratch.alloc(sizeof(int), st));
    int *d_flag = reinterpret_cast<int *>(scratch.p), h_flag = 0;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(deform::k_skin, dim3(grid_for((long long)V)), dim3(deform::kB), 0, st, p->n_vertices, p->n_bones, p->n_morphs, d_rest, reinterpret_cast<const int4 *>(d_bone_index),
                       reinterpret_cast<const float4 *>(d_bone_weight), reinterpret_cast<const float4 *>(d_bones), d_morph_delta, d_morph_weight, d_out, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // only the flag has to come back: the vertices are on the stream
    if (h_flag) { set_error("skin vertices: a bone index of a slot with a non-zero weight lies outside [0, %d); d_out is unspecified", p->n_bones); return GNXR_ERR_INVALID; }
    return GNXR_OK;
}

}  // extern "C"
