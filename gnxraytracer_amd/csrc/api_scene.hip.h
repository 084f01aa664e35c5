// api_scene.hip.h -- gnxr_scene: one copy of a scene (its device tables, per-render state and light-selection table) and the host scene
// all copies of a handle share: the scene's facts, no copy of anything the devices hold in leaf or node order.
// Part of api.hip's translation unit (after api_common.hip.h).
#pragma once

// The per-render state of a handle: path slots, queues and scratch, grown on demand by reserve() to what a launch plan needs (RenderPlan
// and the member functions: api_render.hip.h) and kept for the next render.
struct RenderPlan;
struct RenderState {
    DevBuf<float4> rec[kRecGroups], mis_Y;   // the record groups of the path slots (PathArrays, kernels.hip.h)
    static void record_ptrs(DevBuf<float4> *b, float4 *g[kRecGroups]) { for (int i = 0; i < kRecGroups; ++i) g[i] = b[i].p; }
    DevBuf<float4> L, accum;
    DevBuf<int> hit, queue_a, queue_b, queue_nee, queue_c0, queue_c1, queue_c2, queue_c3;
    DevBuf<unsigned char> pflags, pclass;
    DevBuf<unsigned int> nee_vis;
    // k_compact's scratch (compact_kernel.hip.h): a descriptor per (predicate, tile), the two alternating ticket counters, and the sequence
    // number of the handle's last compaction (descriptors of earlier passes carry earlier numbers: nothing is cleared between passes)
    DevBuf<unsigned long long> tile_desc;
    DevBuf<unsigned int> compact_ticket;
    unsigned int compact_seq = 0;
    DevBuf<int> trace_spill;   // global part of k_trace's per-lane traversal stacks
    DevBuf<float4> vol_n1, vol_f, vol_Li, vol_Tr, vol_Ld, vol_mres;   // VolPath light-estimate records (vol_kernel.hip.h)
    DevBuf<int4> vol_vs;
    DevBuf<unsigned char> vol_state;
    // VolPath packing (k_vol_pack): the second set of the state arrays, the original slot of every path, the renumbering map and the results
    DevBuf<float4> vol_alt[kVolPackF4], vol_alt_rec[kRecGroups], vol_Lout;
    DevBuf<unsigned char> vol_alt_state;
    DevBuf<int> vol_orig, vol_alt_orig, vol_newslot;
    DevBuf<float4> wh_o, wh_d, wh_L, wh_w;   // Whitted recursion frames (whitted_kernel.hip.h)
    DevBuf<float4> wh_rxo, wh_rxd, wh_ryo, wh_ryd;   // their ray differentials (scenes with image textures)
    DevBuf<float> wh_pdf;
    DevBuf<int> wh_rec;
    DevBuf<DCamera> view_cams;   // gnxr_render_views_device: the DCamera record of every view
    // gnxr_render_adaptive_device (adaptive_kernel.hip.h): per pixel the sums over the even samples (the sums over all samples and the count
    // live in accum), the two state bytes and the two list entries; the totals of the compaction that lists a round's pixels.  Allocated
    // by the first adaptive call of a size (reserve_adaptive), 26 bytes per pixel; other renders never touch them.
    DevBuf<float4> ad_A;
    DevBuf<unsigned char> ad_state[2];
    DevBuf<int> ad_list[2];
    DevBuf<unsigned int> ad_totals;

    int reserve(const RenderPlan &pl);
    int reserve_adaptive(const RenderPlan &pl);
    static unsigned long long state_bytes(const RenderPlan &pl);
    // the kernels' views of the arrays
    PathArrays path_arrays();
    VolArrays vol_arrays();
    WhittedArrays whitted_arrays(const RenderPlan &pl, int n_lights);
    VolPackSet pack_set(bool alt);
};

// The host side of a handle: ONE per gnxr_scene_create, shared by the copies on every device of gnxr_init_devices.  It holds the scene's
// FACTS only (SceneFacts, host_scene.h): what the host authored or keeps reading.  Nothing in leaf or node order lives here -- the devices
// hold the only copy of the geometry, attribute, media, texel and grid tables, and the editing calls change it there -- except the refit's
// seeds until every copy has uploaded them (SceneFacts::refit_seeds).  Written only under the primary's render_mutex (the editing calls);
// the workers of render_sharded and the calls bound to a replica read it.
struct SceneHost {
    SceneFacts cs;
    size_t copies_awaiting_seeds = 0;   // copies of the scene that have not uploaded cs.refit_seeds yet (refit_tables releases the seeds at 0)
    bool host_env_stale = false;     // after gnxr_scene_update_environment cs.env_texels / env_texels4 / env_cond_* / env_marg_* lag the devices until sync_host_env()
    std::mutex env_mutex;            // sync_host_env may be reached from the worker of any copy (ensure_grid)
};

struct gnxr_scene {
    const std::shared_ptr<SceneHost> host;
    SceneFacts &cs;   // host->cs
    explicit gnxr_scene(int device_, std::shared_ptr<SceneHost> h = std::make_shared<SceneHost>()) : host(std::move(h)), cs(host->cs), device(device_) {}
    // device tables
    DevBuf<DNode> nodes;
    DevBuf<DNode4> nodes4;
    DevBuf<DTri> tris;
    DevBuf<float> leaf_boxes;
    DevBuf<uint8_t> tri_class;
    DevBuf<DSphere> spheres;
    DevBuf<DMaterial> materials, materials_single;
    DevBuf<DTexture> textures;
    DevBuf<float> tex_texels, ewa_lut, tri_uv, tri_n, tri_s;
    DevBuf<float> aov_albedo;            // feature buffers (api_aov.hip.h): SceneFacts::aov_albedo / material_authored
    DevBuf<int32_t> material_authored;
    DevBuf<DLight> lights;
    DevBuf<int32_t> infinite;
    DevBuf<uint16_t> perms;
    DevBuf<int32_t> primes, prime_sums;
    DevBuf<uint32_t> prime_magic;
    DevBuf<float> env_texels4, env_cond_func, env_cond_cdf, env_cond_int, env_marg_func, env_marg_cdf;
    DevBuf<uint16_t> env_marg_guide, env_cond_guide;
    DevBuf<float> grid_table;
    DevBuf<DMedium> dmedia;
    DevBuf<float> grid_density;
    DevBuf<int32_t> tri_media;
    DLightGrid grid;
    int grid_strategy = -1;
    RenderState st;            // per-render state (grown on demand)
    DevBuf<float4> out;        // gnxr_render: the image on the device
    DevBuf<Counters> counters;
    Counters *h_counters = nullptr;  // pinned
    unsigned int *h_ad_count = nullptr;   // pinned: the size of an adaptive call's next round (run_adaptive), allocated by the first such call
    // the device-driven PathIntegrator loop: lagging copies of the counters (pinned ring, one event per slot) -- the host reads them
    // without ever waiting for the iteration it has just enqueued
    // k_shade runs one kernel per material class; the classes are independent, so they go to different streams and fill each other's ends
    hipStream_t aux_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    static constexpr int kRing = 8;
    Counters *h_ring = nullptr;      // pinned, kRing entries
    hipEvent_t ring_ev[kRing] = {};
    int stack_size = 32;
    bool wide_ok = true;   // 4-wide traversal usable (leaf sizes / triangle count fit the reference encoding)
    std::recursive_mutex render_mutex;   // one render in flight per handle; gnxr_render holds it around its staging buffer too
    const int device;                    // the HIP device the tables live on
    // the same scene on the other devices of gnxr_init_devices (element 0 of that list is this one), and all copies: 0 is this one, the primary
    std::vector<std::unique_ptr<gnxr_scene>> replicas;
    size_t n_copies() const { return 1 + replicas.size(); }
    gnxr_scene *copy(size_t i) { return i == 0 ? this : replicas[i - 1].get(); }
    // f(copy, i) on every copy in turn, its device bound.  The first failure ends the walk: the runtime's last error is cleared and that
    // status returned (its message stays).  Either way the primary's device is current afterwards.
    template <typename F>
    int each_copy(F &&f) {
        int rc = GNXR_OK;
        for (size_t i = 0; i < n_copies() && rc == GNXR_OK; ++i)
            if ((rc = copy(i)->bind()) == GNXR_OK) rc = f(copy(i), i);
        if (rc == GNXR_OK) return bind();
        (void)hipGetLastError(); (void)hipSetDevice(device);
        return rc;
    }
    // An edit that writes the copies in place: apply(copy, i) on every copy; after a failure put_back(copy, i) on every copy (its own
    // status does not count) and the failure's message and status stand.  put_back_after is the second half, for a failure found elsewhere.
    template <typename F>
    int put_back_after(int rc, F &&put_back) {
        const std::string why = get_error();
        (void)each_copy(put_back);
        set_error("%s", why.c_str());
        return rc;
    }
    template <typename A, typename F>
    int apply_or_put_back(A &&apply, F &&put_back) {
        const int rc = each_copy(apply);
        return rc == GNXR_OK ? rc : put_back_after(rc, put_back);
    }
    DevBuf<float4> shard_out;            // a replica's full-size output plane; its rows are peer-copied into the primary's image
    void *h_stage = nullptr;             // pinned: a replica's rows on their way to the primary when the two devices have no peer access
    size_t h_stage_bytes = 0;
    // gnxr_scene_update_vertices: the refit's tables (SceneFacts::refit_seeds, uploaded at the first update; a rebuild swaps its own in),
    // the arrival counters of k_refit_fit, the staged positions and the emissive-vertex flag
    DevBuf<int32_t> upd_corner, upd_parent, upd_node4_src;
    DevBuf<unsigned int> upd_arrived;
    DevBuf<float> upd_xyz;
    DevBuf<int> upd_flag;
    // gnxr_scene_update_materials / gnxr_scene_set_triangle_materials: SceneFacts::tri_material / tri_own_attr / mat_map, uploaded at the
    // first edit (material_tables; the map is allocated last: it marks the set complete) and kept current by every edit after it
    DevBuf<int32_t> mat_tri, mat_map;
    DevBuf<uint8_t> mat_own;
    // gnxr_scene_recompute_normals (api_deform.hip.h): the vertex -> corner table (CSR over authored corner ids 3 t + k, built at the first call
    // of a topology, released by gnxr_scene_set_geometry), the per-call face normals (per authored triangle) and vertex sums; and the
    // refusal flag of gnxr_scene_update_attributes
    DevBuf<uint32_t> adj_offsets, adj_corners;
    DevBuf<float4> nrm_face, nrm_vsum;
    DevBuf<int> attr_flag;
    // gnxr_render_views_device: the host copy of st.view_cams (what the stream-ordered upload reads; both only grow)
    std::vector<DCamera> h_view_cams;

    int bind() const { HIP_TRY(hipSetDevice(device)); return GNXR_OK; }
    // the host copies of the environment tables, downloaded on demand after gnxr_scene_update_environment (their one reader is the
    // host-built spatial light table: build_light_grid).  Every copy holds the same tables: the (bound) device of this one is read.
    int sync_host_env() {
        std::lock_guard<std::mutex> lock(host->env_mutex);
        if (!host->host_env_stale) return GNXR_OK;
        const size_t nt = (size_t)cs.env.w * cs.env.h, W2 = cs.env.dw, H2 = cs.env.dh;
        cs.env_texels4.resize(4 * nt); cs.env_texels.resize(3 * nt);
        cs.env_cond_func.resize(W2 * H2); cs.env_cond_cdf.resize((W2 + 1) * H2); cs.env_cond_int.resize(H2);
        cs.env_marg_func.resize(H2); cs.env_marg_cdf.resize(H2 + 1);
        cs.env_marg_guide.resize(kEnvGuideMarg + 1); cs.env_cond_guide.resize(H2 * (kEnvGuideCond + 1));
#define DOWN(field) HIP_TRY(hipMemcpy(cs.field.data(), field.p, cs.field.size() * sizeof(cs.field[0]), hipMemcpyDeviceToHost));
        DOWN(env_texels4) DOWN(env_cond_func) DOWN(env_cond_cdf) DOWN(env_cond_int) DOWN(env_marg_func) DOWN(env_marg_cdf) DOWN(env_marg_guide) DOWN(env_cond_guide)
#undef DOWN
        for (size_t i = 0; i < nt; ++i) { cs.env_texels[3 * i] = cs.env_texels4[4 * i]; cs.env_texels[3 * i + 1] = cs.env_texels4[4 * i + 1]; cs.env_texels[3 * i + 2] = cs.env_texels4[4 * i + 2]; }
        host->host_env_stale = false;
        return GNXR_OK;
    }
    ~gnxr_scene() {
        if (h_counters) (void)hipHostFree(h_counters);
        if (h_ad_count) (void)hipHostFree(h_ad_count);
        if (h_ring) (void)hipHostFree(h_ring);
        if (h_stage) (void)hipHostFree(h_stage);
        for (hipEvent_t e : ring_ev) if (e) (void)hipEventDestroy(e);
        for (hipStream_t a : aux_stream) if (a) (void)hipStreamDestroy(a);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        for (hipEvent_t e : ev_join) if (e) (void)hipEventDestroy(e);
    }

    // the lights and the environment map: what Sample_Li / Pdf_Li / Le read, without the selection table (grid, grid_table stay zero).
    // After the scene is created only the editing calls change what is behind these pointers: gnxr_scene_update_vertices refits the world radius
    // (cs.env, distant lights), GNXR_UPDATE_MOVE_LIGHTS moves the area lights, gnxr_scene_update_lights rewrites light records,
    // gnxr_scene_update_environment swaps in new environment tables (and cs.env with them), gnxr_scene_set_lights swaps in another list
    // (lights, infinite; the counts are read from the host scene here, at every call).
    DLightTables light_tables_static() const {
        DLightTables lt = {};
        lt.lights = lights.p;
        lt.n_lights = (int)cs.desc_lights.size();
        lt.infinite = infinite.p;
        lt.n_infinite = (int)cs.infinite_lights.size();
        lt.has_env = cs.has_env ? 1 : 0;
        lt.env = cs.env;
        lt.env_texels = reinterpret_cast<const float4 *>(env_texels4.p);
        lt.env_cond_func = env_cond_func.p; lt.env_cond_cdf = env_cond_cdf.p; lt.env_cond_int = env_cond_int.p;
        lt.env_marg_func = env_marg_func.p; lt.env_marg_cdf = env_marg_cdf.p;
        lt.env_marg_guide = env_marg_guide.p; lt.env_cond_guide = env_cond_guide.p;
        return lt;
    }
    DScene device_scene(int W, int H) {
        DScene d;
        d.nodes = reinterpret_cast<const float4 *>(nodes.p);
        d.nodes4 = reinterpret_cast<const float4 *>(nodes4.p);
        d.root4 = cs.root4;
        d.tris = tris.p;
        d.leaf_box = reinterpret_cast<const float4 *>(leaf_boxes.p);
        d.tri_class = tri_class.p;
        d.leaf1_from_verts = (cs.leaf1_from_verts && !Knobs::leaf_box_table()) ? 1 : 0;
        d.spheres = spheres.p;
        d.n_spheres = cs.n_spheres;
        d.materials = materials.p + 1;   // [0] carries the texture tables
        d.escape_class = 0;              // render_one (RenderPlan::escape_queue): 3 for the PathIntegrator in a scene without image-textured materials
        d.lt = light_tables_static();
        d.lt.grid = grid;
        d.lt.grid_table = grid_table.p;
        d.st.perms = perms.p; d.st.primes = primes.p; d.st.prime_sums = prime_sums.p; d.st.prime_magic = prime_magic.p;
        d.st.h = make_halton(W, H);
        return d;
    }
    // the record in front of the materials (tex_tables(), device_texture.h): the texture tables and the per-corner attribute tables the
    // scene has, at the given addresses (an empty upload still allocates, so an absent table is decided by the host scene)
    DTexTables tex_tables(const float *uv, const float *n, const float *s) const {
        DTexTables tt;
        tt.textures = textures.p; tt.texels = reinterpret_cast<const float4 *>(tex_texels.p); tt.ewa_lut = ewa_lut.p;
        tt.tri_uv = cs.has_tri_uv ? uv : nullptr; tt.tri_n = cs.has_tri_n ? n : nullptr; tt.tri_s = cs.has_tri_s ? s : nullptr;
        return tt;
    }
    // The one way to write the material tables of the (bound) device: record 0 with the texture tables and the per-corner attribute tables
    // at exactly the addresses given (null: absent), followed by the materials.  In place: upload_scene sized both buffers for the worst case.
    int write_material_tables(const std::vector<DMaterial> &mats, const std::vector<DMaterial> &mats_single, const float *uv, const float *n, const float *s) {
        DTexTables rec;
        rec.textures = textures.p; rec.texels = reinterpret_cast<const float4 *>(tex_texels.p); rec.ewa_lut = ewa_lut.p;
        rec.tri_uv = uv; rec.tri_n = n; rec.tri_s = s;
        for (int k = 0; k < 2; ++k) {
            const std::vector<DMaterial> &src = k == 0 ? mats : mats_single;
            std::vector<DMaterial> up(src.size() + 1);
            memset(&up[0], 0, sizeof(DMaterial));
            memcpy(&up[0], &rec, sizeof(rec));
            std::copy(src.begin(), src.end(), up.begin() + 1);
            HIP_TRY(hipMemcpy((k == 0 ? materials : materials_single).p, up.data(), up.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
        }
        return GNXR_OK;
    }
    // what the tree allows: the binary walk's stack size and whether the 4-wide traversal can hold it (leaf sizes / triangle count fit the
    // reference encoding).  leaf_over_127: some leaf holds more than 127 primitives.
    void set_traversal(bool leaf_over_127) {
        stack_size = cs.bvh_max_depth + 1 <= 32 ? 32 : 64;
        wide_ok = cs.n_triangles < (1u << 24) && cs.stack4_need + 1 <= 128 && !Knobs::binary_bvh() && !leaf_over_127;
    }
    DMediaTables media_tables() {
        DMediaTables m;
        m.media = dmedia.p;
        m.density = grid_density.p;
        m.tri_media = cs.has_tri_media ? reinterpret_cast<const int2 *>(tri_media.p) : nullptr;
        return m;
    }
    // light-selection table (core/LightDistribution.cpp).  The spatial strategy's dense voxel table is filled on the device
    // (k_light_grid, ~1 ms instead of ~1 s of host threads for 64^3 voxels); GNXR_HOST_LIGHT_GRID=1 forces the host
    // restatement, which produces the same bits (tests/test_gpu_parity.py::test_light_grid_device_equals_host).
    int ensure_grid(int strategy, bool force_host = false) {
        if (grid_strategy == strategy && !force_host) return GNXR_OK;
        const int nl = (int)cs.desc_lights.size();
        const bool on_device = strategy == GNXR_LIGHTS_SPATIAL && nl >= 2 && !force_host && !Knobs::host_light_grid();
        std::vector<float> table;
        build_light_grid(cs, strategy, &grid, &table, /*layout_only=*/true);
        {   // the dense spatial table holds nvox^3 x (2 lights + 1) floats: refuse what cannot fit instead of failing inside an allocation
            const unsigned long long bytes = (unsigned long long)grid.nvox[0] * grid.nvox[1] * grid.nvox[2] * (unsigned long long)grid.stride * sizeof(float);
            size_t free_b = 0, total_b = 0;
            unsigned long long limit = 64ull << 30;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) limit = std::min<unsigned long long>(limit, free_b / 2);
            if (bytes > limit) {
                set_error("spatial light distribution: %d x %d x %d voxels x %d lights need %.1f GB (limit %.1f GB); use GNXR_LIGHTS_POWER or GNXR_LIGHTS_UNIFORM for this many lights",
                          grid.nvox[0], grid.nvox[1], grid.nvox[2], nl, bytes * 1e-9, limit * 1e-9);
                return GNXR_ERR_UNSUPPORTED;
            }
        }
        if (!on_device && grid.spatial && cs.has_env)   // the host's probes sample the environment tables
            if (int src = sync_host_env()) return src;
        if (!on_device) build_light_grid(cs, strategy, &grid, &table, false);
        int rc;
        if (on_device) {
            const size_t nv = (size_t)grid.nvox[0] * grid.nvox[1] * grid.nvox[2];
            if ((rc = grid_table.alloc(nv * grid.stride)) != GNXR_OK) return rc;
            HIP_TRY(hipMemset(grid_table.p, 0, nv * grid.stride * sizeof(float)));   // padded records: the pad floats are zero, as in the host-built table
            float ri[5 * 128];
            light_grid_probes(cs, ri);
            DevBuf<float> d_ri;
            if ((rc = d_ri.upload(ri, 5 * 128)) != GNXR_OK) return rc;
            DLightTables lt = device_scene(1, 1).lt;
            bool area_only = true;
            for (const gnxr_light &l : cs.desc_lights) if (l.type != GNXR_LIGHT_AREA_TRI) area_only = false;
            const int blocks = (int)std::min<size_t>((nv + kBlock - 1) / kBlock, (size_t)g_num_cus * 8);
            if (nl > kGridMaxLights) {   // mesh lights: any number of lights, the table is the scratch space
                if (area_only) hipLaunchKernelGGL((k_light_grid_any<LT_AREA>), dim3(blocks), dim3(kBlock), 0, 0, lt, grid, (const float *)d_ri.p, grid_table.p);
                else hipLaunchKernelGGL((k_light_grid_any<LT_ALL>), dim3(blocks), dim3(kBlock), 0, 0, lt, grid, (const float *)d_ri.p, grid_table.p);
            } else if (area_only) hipLaunchKernelGGL((k_light_grid<LT_AREA>), dim3(blocks), dim3(kBlock), 0, 0, lt, grid, (const float *)d_ri.p, grid_table.p);
            else hipLaunchKernelGGL((k_light_grid<LT_ALL>), dim3(blocks), dim3(kBlock), 0, 0, lt, grid, (const float *)d_ri.p, grid_table.p);
            HIP_TRY(hipDeviceSynchronize());
        } else if ((rc = grid_table.upload(table)) != GNXR_OK) return rc;
        grid_strategy = force_host ? -1 : strategy;
        return GNXR_OK;
    }
};
