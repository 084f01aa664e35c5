// api_hlbvh.hip.h -- host driver of the HLBVH device build.  Part of api.hip's translation unit.
#pragma once

// ---- HLBVH on the device (hlbvh_build.hip.h): Morton codes, own LSD radix sort, the treelets' LBVHs and the SAH over their roots.  The host
// gets the finished build tree back (scene_compile.cpp flattens it and derives the 4-wide layout as for the other split methods).
namespace {
bool device_hlbvh_build(const float *prim_bounds6, const float *centroids3, int n, const float lo[3], const float hi[3], std::vector<HlbvhNode> *nodes_out, int *root_out,
                        uint32_t *prims_sorted) {
    using namespace hlbvh;
    if (ensure_device() != GNXR_OK) return false;
    if (n <= 0) { set_error("HLBVH: no primitives"); return false; }
    DevBuf<float> d_cen, d_pb;
    DevBuf<uint32_t> k_a, k_b, v_a, v_b, hist, sums, head, ukey, ustart, thead, total;
    DevBuf<int> parent, roots, tmp, flags;
    DevBuf<unsigned int> arrived;
    DevBuf<HlbvhNode> d_nodes;
    const int n_tiles = (n + kTile - 1) / kTile;
    const auto fail = [&](const char *what) { set_error("HLBVH device build: %s", what); return false; };
    if (d_cen.upload(centroids3, 3 * (size_t)n) || d_pb.upload(prim_bounds6, 6 * (size_t)n) || k_a.alloc(n) || k_b.alloc(n) || v_a.alloc(n) || v_b.alloc(n) ||
        hist.alloc((size_t)64 * n_tiles) || sums.alloc((size_t)std::max(n_tiles, (64 * n_tiles + kTile - 1) / kTile) + 1) || head.alloc(n) || ukey.alloc(n) || ustart.alloc(n) ||
        thead.alloc(n) || total.alloc(2) || flags.alloc(2))
        return fail("out of device memory");
    if (hipMemset(flags.p, 0, 2 * sizeof(int)) != hipSuccess) return fail("memset");
    const bool verbose = getenv("GNXR_VERBOSE") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto stage = [&](const char *name) {
        if (!verbose) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[gnxr] hlbvh %-10s %7.2f ms\n", name, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    stage("alloc");
    const int g = grid_for(n);
    hipLaunchKernelGGL(hlbvh::k_morton_codes, dim3(g), dim3(kB), 0, 0, (const float *)d_cen.p, n, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], k_a.p, v_a.p);
    // exclusive scan helper (in place); total (optional) lands in *d_total
    auto scan = [&](uint32_t *v, int m, uint32_t *d_total) {
        const int tiles = (m + kTile - 1) / kTile;
        hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(kB), 0, 0, v, m, sums.p);
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, 0, sums.p, tiles, d_total);
        hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(kB), 0, 0, v, m, (const uint32_t *)sums.p);
    };
    // RadixSort (BVHAccel.cpp:102-141): 30 bits, 6 per pass, least significant first, stable
    uint32_t *kin = k_a.p, *kout = k_b.p, *vin = v_a.p, *vout = v_b.p;
    for (int pass = 0; pass < 5; ++pass) {
        hipLaunchKernelGGL(k_rs_hist, dim3(n_tiles), dim3(kB), 0, 0, (const uint32_t *)kin, n, 6 * pass, n_tiles, hist.p);
        scan(hist.p, 64 * n_tiles, nullptr);
        hipLaunchKernelGGL(k_rs_scatter, dim3(n_tiles), dim3(kB), 0, 0, (const uint32_t *)kin, (const uint32_t *)vin, n, 6 * pass, n_tiles, (const uint32_t *)hist.p, kout, vout);
        std::swap(kin, kout); std::swap(vin, vout);
    }
    const uint32_t *codes = kin, *prims = vin;   // sorted
    stage("sort");
    // leaves = runs of equal codes
    hipLaunchKernelGGL(k_hl_flags, dim3(g), dim3(kB), 0, 0, codes, n, head.p);
    scan(head.p, n, total.p);
    hipLaunchKernelGGL(k_hl_runs, dim3(g), dim3(kB), 0, 0, codes, (const uint32_t *)head.p, n, ukey.p, ustart.p);
    uint32_t U = 0;
    if (hipMemcpy(&U, total.p, sizeof(U), hipMemcpyDeviceToHost) != hipSuccess || U == 0 || U > (uint32_t)n) return fail("run count");
    // treelets = runs of equal top 12 bits
    const int gu = grid_for(U);
    hipLaunchKernelGGL(k_hl_tflags, dim3(gu), dim3(kB), 0, 0, (const uint32_t *)ukey.p, (int)U, thead.p);
    scan(thead.p, (int)U, total.p + 1);
    uint32_t T = 0;
    if (hipMemcpy(&T, total.p + 1, sizeof(T), hipMemcpyDeviceToHost) != hipSuccess || T == 0 || T > 4096u) return fail("treelet count");
    const size_t cap = (size_t)2 * U + T;
    if (d_nodes.alloc(cap) || parent.alloc(cap) || arrived.alloc(cap) || roots.alloc(T) || tmp.alloc(T)) return fail("out of device memory");
    if (hipMemset(d_nodes.p, 0, cap * sizeof(HlbvhNode)) != hipSuccess || hipMemset(parent.p, 0xff, cap * sizeof(int)) != hipSuccess ||
        hipMemset(arrived.p, 0, cap * sizeof(unsigned int)) != hipSuccess)
        return fail("memset");
    hipLaunchKernelGGL(k_hl_leaves, dim3(gu), dim3(kB), 0, 0, (const uint32_t *)ustart.p, (int)U, n, prims, (const float *)d_pb.p, d_nodes.p, flags.p);
    if (U > 1) {
        hipLaunchKernelGGL(k_hl_internal, dim3(gu), dim3(kB), 0, 0, (const uint32_t *)ukey.p, (int)U, d_nodes.p, parent.p);
        hipLaunchKernelGGL(k_hl_fit, dim3(gu), dim3(kB), 0, 0, (int)U, d_nodes.p, (const int *)parent.p, arrived.p);
    }
    hipLaunchKernelGGL(k_hl_roots, dim3(gu), dim3(kB), 0, 0, (const uint32_t *)ukey.p, (const uint32_t *)thead.p, (int)U, roots.p);
    stage("treelets");
    // buildUpperSAH level by level: the ranges of a level are split by one wave each
    int h_flags[2] = {0, -1};
    if (T == 1) {
        if (hipMemcpy(flags.p + 1, roots.p, sizeof(int), hipMemcpyDeviceToDevice) != hipSuccess) return fail("copy");
    } else {
        DevBuf<UpRange> q_a, q_b;
        DevBuf<int> counters;   // [0] ranges of the next level, [1] upper nodes allocated
        if (q_a.alloc(T) || q_b.alloc(T) || counters.alloc(2) || hipMemset(counters.p, 0, 2 * sizeof(int)) != hipSuccess) return fail("out of device memory");
        UpRange first{0, (int)T, -1};
        if (hipMemcpy(q_a.p, &first, sizeof(first), hipMemcpyHostToDevice) != hipSuccess) return fail("upload");
        UpRange *qin = q_a.p, *qout = q_b.p;
        int n_in = 1;
        for (int level = 0; n_in > 0; ++level) {
            if (level > (int)T) return fail("upper SAH did not terminate");
            const int blocks = std::max(1, std::min((n_in * 64 + kB - 1) / kB, g_num_cus * 8));
            hipLaunchKernelGGL(k_hl_upper_level, dim3(blocks), dim3(kB), 0, 0, (const UpRange *)qin, n_in, qout, counters.p, roots.p, tmp.p, d_nodes.p, (int)(2 * U), counters.p + 1,
                               flags.p + 1, flags.p);
            if (hipMemcpy(&n_in, counters.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail("level count");
            if (hipMemset(counters.p, 0, sizeof(int)) != hipSuccess) return fail("memset");
            std::swap(qin, qout);
        }
    }
    stage("upper");
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return fail(hipGetErrorString(hipGetLastError()));
    if (hipMemcpy(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost) != hipSuccess) return fail("download");
    if (h_flags[0]) {
        set_error("HLBVH: the reference's build does not terminate on this input (coincident treelet centroids) or a leaf exceeds 65535 primitives");
        return false;
    }
    nodes_out->resize(cap);
    if (hipMemcpy(nodes_out->data(), d_nodes.p, cap * sizeof(HlbvhNode), hipMemcpyDeviceToHost) != hipSuccess) return fail("download");
    if (hipMemcpy(prims_sorted, prims, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("download");
    stage("download");
    *root_out = h_flags[1];
    return *root_out >= 0 && (size_t)*root_out < cap;
}
}  // namespace
