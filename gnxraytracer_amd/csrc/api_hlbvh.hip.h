// api_hlbvh.hip.h -- host driver of the HLBVH device build.  Part of api.hip's translation unit.
#pragma once

// ---- HLBVH on the device (hlbvh_build.hip.h): Morton codes, own LSD radix sort, the treelets' LBVHs and the SAH over their roots.  The host
// gets the finished build tree back (scene_compile.cpp flattens it and derives the 4-wide layout as for the other split methods).
namespace {
// exclusive scan of m unsigned values in place (hlbvh_build.hip.h); the total (optional) lands in *d_total.  `sums`: ceil(m / kTile) + 1 words
void hl_scan(uint32_t *v, int m, uint32_t *sums, uint32_t *d_total, hipStream_t st) {
    using namespace hlbvh;
    const int tiles = (m + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(kB), 0, st, v, m, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, sums, tiles, d_total);
    hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(kB), 0, st, v, m, (const uint32_t *)sums);
}

// What the device stage leaves on the device: the build tree (`cap` slots: leaves [0, U), treelet interiors [U, 2U), upper SAH nodes from
// 2U; unused slots are zero), the sorted primitive ids and the root.  The buffers live as long as this record.
struct HlbvhDevice {
    DevBuf<uint32_t> k_a, k_b, v_a, v_b, hist, sums, head, ukey, ustart, thead, total;
    DevBuf<int> parent, roots, tmp, flags, counters;
    DevBuf<unsigned int> arrived;
    DevBuf<hlbvh::UpRange> q_a, q_b;
    DevBuf<HlbvhNode> d_nodes;
    const uint32_t *prims = nullptr;
    size_t cap = 0;
    int U = 0, T = 0, root = -1;
};

// The build over device inputs (prim_bounds6 / centroids3 in primitive order, lo / hi: the bounds of the centroids), on stream `st`.
// GNXR_OK, or a status with the error text set: GNXR_ERR_INVALID where the reference's build does not terminate, GNXR_ERR_OOM, GNXR_ERR_RUNTIME.
int device_hlbvh_core(const float *d_pb, const float *d_cen, int n, const float lo[3], const float hi[3], hipStream_t st, HlbvhDevice *o) {
    using namespace hlbvh;
    DevBuf<uint32_t> &k_a = o->k_a, &k_b = o->k_b, &v_a = o->v_a, &v_b = o->v_b, &hist = o->hist, &sums = o->sums, &head = o->head, &ukey = o->ukey, &ustart = o->ustart,
                     &thead = o->thead, &total = o->total;
    DevBuf<int> &parent = o->parent, &roots = o->roots, &tmp = o->tmp, &flags = o->flags;
    DevBuf<unsigned int> &arrived = o->arrived;
    DevBuf<HlbvhNode> &d_nodes = o->d_nodes;
    const int n_tiles = (n + kTile - 1) / kTile;
    const auto fail = [&](const char *what, int rc = GNXR_ERR_RUNTIME) { set_error("HLBVH device build: %s", what); return rc; };
    const auto oom = [&]() { return fail("out of device memory", GNXR_ERR_OOM); };
    if (k_a.alloc(n) || k_b.alloc(n) || v_a.alloc(n) || v_b.alloc(n) ||
        hist.alloc((size_t)64 * n_tiles) || sums.alloc((size_t)std::max(n_tiles, (64 * n_tiles + kTile - 1) / kTile) + 1) || head.alloc(n) || ukey.alloc(n) || ustart.alloc(n) ||
        thead.alloc(n) || total.alloc(2) || flags.alloc(2))
        return oom();
    if (hipMemsetAsync(flags.p, 0, 2 * sizeof(int), st) != hipSuccess) return fail("memset");
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
    hipLaunchKernelGGL(hlbvh::k_morton_codes, dim3(g), dim3(kB), 0, st, d_cen, n, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], k_a.p, v_a.p);
    auto scan = [&](uint32_t *v, int m, uint32_t *d_total) { hl_scan(v, m, sums.p, d_total, st); };
    // RadixSort (BVHAccel.cpp:102-141): 30 bits, 6 per pass, least significant first, stable
    uint32_t *kin = k_a.p, *kout = k_b.p, *vin = v_a.p, *vout = v_b.p;
    for (int pass = 0; pass < 5; ++pass) {
        hipLaunchKernelGGL(k_rs_hist, dim3(n_tiles), dim3(kB), 0, st, (const uint32_t *)kin, n, 6 * pass, n_tiles, hist.p);
        scan(hist.p, 64 * n_tiles, nullptr);
        hipLaunchKernelGGL(k_rs_scatter, dim3(n_tiles), dim3(kB), 0, st, (const uint32_t *)kin, (const uint32_t *)vin, n, 6 * pass, n_tiles, (const uint32_t *)hist.p, kout, vout);
        std::swap(kin, kout); std::swap(vin, vout);
    }
    const uint32_t *codes = kin, *prims = vin;   // sorted
    stage("sort");
    // leaves = runs of equal codes
    hipLaunchKernelGGL(k_hl_flags, dim3(g), dim3(kB), 0, st, codes, n, head.p);
    scan(head.p, n, total.p);
    hipLaunchKernelGGL(k_hl_runs, dim3(g), dim3(kB), 0, st, codes, (const uint32_t *)head.p, n, ukey.p, ustart.p);
    // a scalar back to the host, ordered on the build's stream
    const auto fetch = [&](void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    };
    uint32_t U = 0;
    if (!fetch(&U, total.p, sizeof(U)) || U == 0 || U > (uint32_t)n) return fail("run count");
    // treelets = runs of equal top 12 bits
    const int gu = grid_for(U);
    hipLaunchKernelGGL(k_hl_tflags, dim3(gu), dim3(kB), 0, st, (const uint32_t *)ukey.p, (int)U, thead.p);
    scan(thead.p, (int)U, total.p + 1);
    uint32_t T = 0;
    if (!fetch(&T, total.p + 1, sizeof(T)) || T == 0 || T > 4096u) return fail("treelet count");
    const size_t cap = (size_t)2 * U + T;
    if (d_nodes.alloc(cap) || parent.alloc(cap) || arrived.alloc(cap) || roots.alloc(T) || tmp.alloc(T)) return oom();
    if (hipMemsetAsync(d_nodes.p, 0, cap * sizeof(HlbvhNode), st) != hipSuccess || hipMemsetAsync(parent.p, 0xff, cap * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(arrived.p, 0, cap * sizeof(unsigned int), st) != hipSuccess)
        return fail("memset");
    hipLaunchKernelGGL(k_hl_leaves, dim3(gu), dim3(kB), 0, st, (const uint32_t *)ustart.p, (int)U, n, prims, d_pb, d_nodes.p, flags.p);
    if (U > 1) {
        hipLaunchKernelGGL(k_hl_internal, dim3(gu), dim3(kB), 0, st, (const uint32_t *)ukey.p, (int)U, d_nodes.p, parent.p);
        hipLaunchKernelGGL(k_hl_fit, dim3(gu), dim3(kB), 0, st, (int)U, d_nodes.p, (const int *)parent.p, arrived.p);
    }
    hipLaunchKernelGGL(k_hl_roots, dim3(gu), dim3(kB), 0, st, (const uint32_t *)ukey.p, (const uint32_t *)thead.p, (int)U, roots.p);
    stage("treelets");
    // buildUpperSAH level by level: the ranges of a level are split by one wave each
    int h_flags[2] = {0, -1};
    if (T == 1) {
        if (hipMemcpyAsync(flags.p + 1, roots.p, sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail("copy");
    } else {
        DevBuf<UpRange> &q_a = o->q_a, &q_b = o->q_b;
        DevBuf<int> &counters = o->counters;   // [0] ranges of the next level, [1] upper nodes allocated
        if (q_a.alloc(T) || q_b.alloc(T) || counters.alloc(2)) return oom();
        if (hipMemsetAsync(counters.p, 0, 2 * sizeof(int), st) != hipSuccess) return fail("memset");
        const UpRange first{0, (int)T, -1};
        if (hipMemcpyAsync(q_a.p, &first, sizeof(first), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("upload");
        UpRange *qin = q_a.p, *qout = q_b.p;
        int n_in = 1;
        for (int level = 0; n_in > 0; ++level) {
            if (level > (int)T) return fail("upper SAH did not terminate");
            const int blocks = std::max(1, std::min((n_in * 64 + kB - 1) / kB, g_num_cus * 8));
            hipLaunchKernelGGL(k_hl_upper_level, dim3(blocks), dim3(kB), 0, st, (const UpRange *)qin, n_in, qout, counters.p, roots.p, tmp.p, d_nodes.p, (int)(2 * U), counters.p + 1,
                               flags.p + 1, flags.p);
            if (!fetch(&n_in, counters.p, sizeof(int))) return fail("level count");
            if (hipMemsetAsync(counters.p, 0, sizeof(int), st) != hipSuccess) return fail("memset");
            std::swap(qin, qout);
        }
    }
    stage("upper");
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return fail(hipGetErrorString(hipGetLastError()));
    if (!fetch(h_flags, flags.p, sizeof(h_flags))) return fail("download");
    if (h_flags[0]) {
        set_error("HLBVH: the reference's build does not terminate on this input (coincident treelet centroids) or a leaf exceeds 65535 primitives");
        return GNXR_ERR_INVALID;
    }
    o->prims = prims; o->cap = cap; o->U = (int)U; o->T = (int)T; o->root = h_flags[1];
    if (o->root < 0 || (size_t)o->root >= cap) return fail("no root");
    return GNXR_OK;
}

// gnxr_scene_create's form (compile_scene's HlbvhBuildFn): host inputs up, the build on the null stream, the build tree and the order down
bool device_hlbvh_build(const float *prim_bounds6, const float *centroids3, int n, const float lo[3], const float hi[3], std::vector<HlbvhNode> *nodes_out, int *root_out,
                        uint32_t *prims_sorted) {
    if (ensure_device() != GNXR_OK) return false;
    if (n <= 0) { set_error("HLBVH: no primitives"); return false; }
    DevBuf<float> d_cen, d_pb;
    if (d_cen.upload(centroids3, 3 * (size_t)n) || d_pb.upload(prim_bounds6, 6 * (size_t)n)) { set_error("HLBVH device build: out of device memory"); return false; }
    HlbvhDevice dev;
    if (device_hlbvh_core(d_pb.p, d_cen.p, n, lo, hi, nullptr, &dev) != GNXR_OK) return false;
    nodes_out->resize(dev.cap);
    if (hipMemcpy(nodes_out->data(), dev.d_nodes.p, dev.cap * sizeof(HlbvhNode), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(prims_sorted, dev.prims, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("HLBVH device build: download");
        return false;
    }
    *root_out = dev.root;
    return true;
}
}  // namespace
