// api_common.hip.h -- what every part of api.hip shares: HIP_TRY / hip_status, the process-wide device state, the tuning knobs, per-kernel
// timing, device buffers and grid sizing.  Part of api.hip's translation unit (included there after the kernel headers).
#pragma once

namespace { int hip_status(hipError_t e); }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);       \
            return hip_status(e_);                                                                      \
        }                                                                                               \
    } while (0)

namespace {

// hipError_t -> gnxr_status: allocation failures, "there is no (such) device", and everything else (a failed launch, an
// invalid argument, a fault reported at the next synchronisation) as GNXR_ERR_RUNTIME
int hip_status(hipError_t e) {
    if (e == hipErrorOutOfMemory) return GNXR_ERR_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver || e == hipErrorNotInitialized) return GNXR_ERR_NO_DEVICE;
    return GNXR_ERR_RUNTIME;
}

int g_device = -1;
std::vector<int> g_devices;        // gnxr_init_devices: every scene is replicated on these and renders shard their rows over them
std::vector<char> g_peer_ok;       // per entry of g_devices: the primary device and this one can address each other's memory (peer access enabled both ways)
int g_num_cus = 256;
int g_profiling = 0;
int g_grid_bpc = 8;   // blocks per CU that cap the grid of a grid-stride kernel (GNXR_GRID_BLOCKS_PER_CU: tuning knob)
int g_trace_blocks_per_cu = 5;   // persistent blocks of the traversal kernel per CU (5 waves per SIMD at its 96 VGPRs, 32 KB of LDS each); GNXR_TRACE_BLOCKS_PER_CU overrides (tuning)

// Per-kernel timing with HIP events on the render stream.  Events are recycled from a pool and resolved
// after the stream has been synchronised.
struct KernelTimer {
    std::vector<hipEvent_t> pool;
    struct Span { int kind; hipEvent_t a, b; };
    std::vector<Span> open;
    size_t used = 0;
    double seconds[3] = {0, 0, 0};
    unsigned launches[3] = {0, 0, 0};
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[used++];
    }
    void begin(int kind, hipStream_t st) { Span s{kind, get(), get()}; if (s.a && s.b) { (void)hipEventRecord(s.a, st); open.push_back(s); } }
    void end(hipStream_t st) { if (!open.empty()) (void)hipEventRecord(open.back().b, st); }
    // call only after the stream has been synchronised
    void collect() {
        for (auto &s : open) { float ms = 0; if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { seconds[s.kind] += ms * 1e-3; launches[s.kind]++; } }
        open.clear();
        used = 0;
    }
    ~KernelTimer() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// The GNXR_* tuning knobs and experiment switches of the render path.  "once": read at the knob's first use and kept for the life of the
// process; "per call": read every time the code asks, because tests vary it inside one process; "per init": read when a device is bound.
struct Knobs {
    static int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
    static bool env_set(const char *name) { return getenv(name) != nullptr; }
#define GX_ONCE(type, expr) do { static const type v = (expr); return v; } while (0)
    // GNXR_TRACE_BLOCKS_PER_CU: persistent blocks of the traversal kernel per CU, 1 .. 8 (default 5: g_trace_blocks_per_cu).  Per init; 0 = keep
    static int trace_blocks_per_cu() { const int v = env_int("GNXR_TRACE_BLOCKS_PER_CU", 0); return v >= 1 && v <= 8 ? v : 0; }
    // GNXR_GRID_BLOCKS_PER_CU: blocks per CU that cap a grid-stride kernel's grid, 1 .. 4096 (default 8: g_grid_bpc).  Per init; 0 = keep
    static int grid_blocks_per_cu() { const int v = env_int("GNXR_GRID_BLOCKS_PER_CU", 0); return v >= 1 && v <= 4096 ? v : 0; }
    // GNXR_TRACE_LDS_LEVELS: most levels of the traversal stack kept in LDS, at least 2 (default 64).  Once
    static int trace_lds_levels() { GX_ONCE(int, env_set("GNXR_TRACE_LDS_LEVELS") ? std::max(2, env_int("GNXR_TRACE_LDS_LEVELS", 0)) : 64); }
    // GNXR_TRACE_CHUNK: rays a wave takes per atomic, a multiple of 64 (default kTraceChunk).  Once
    static int trace_chunk() { GX_ONCE(int, env_set("GNXR_TRACE_CHUNK") ? std::max(64, env_int("GNXR_TRACE_CHUNK", 0) / 64 * 64) : kTraceChunk); }
    // GNXR_LEAF_BOX_TABLE: set = one-triangle leaves read leaf_boxes instead of their vertices (experiment; default unset).  Once
    static bool leaf_box_table() { GX_ONCE(bool, env_set("GNXR_LEAF_BOX_TABLE")); }
    // GNXR_REGIONS: sub-passes in flight when passes_in_flight is 0 (default 0 = 4).  Once
    static int regions() { GX_ONCE(int, env_int("GNXR_REGIONS", 0)); }
    // GNXR_PIPELINE: 0 = the PathIntegrator renders one sub-pass at a time (experiment; default 1).  Once
    static bool pipeline() { GX_ONCE(bool, env_int("GNXR_PIPELINE", 1) != 0); }
    // GNXR_PIPE_CUT: loop turns between sub-pass starts (default -1 = from max_depth, the lag and the regions).  Once
    static int pipe_cut() { GX_ONCE(int, env_int("GNXR_PIPE_CUT", -1)); }
    // GNXR_LOOP_LAG: loop turns the host may run ahead of the counters it has seen (default -1 = 2).  Once
    static int loop_lag() { GX_ONCE(int, env_int("GNXR_LOOP_LAG", -1)); }
    // GNXR_SHADE_BLOCKS_PER_CU: blocks per CU of a k_shade grid, at least 1 (default 32).  Once
    static int shade_blocks_per_cu() { GX_ONCE(int, env_set("GNXR_SHADE_BLOCKS_PER_CU") ? std::max(1, env_int("GNXR_SHADE_BLOCKS_PER_CU", 0)) : 32); }
    // GNXR_SHADE_LDS_DIMS: Halton dimensions whose tables k_shade keeps in LDS, 0 .. 128 (default 64).  Once
    static int shade_lds_dims() { GX_ONCE(int, env_set("GNXR_SHADE_LDS_DIMS") ? std::max(0, std::min(128, env_int("GNXR_SHADE_LDS_DIMS", 0))) : 64); }
    // GNXR_SHADE_LDS_TABLES: 0 = small material and light tables stay in global memory (experiment; default 1).  Once
    static bool shade_lds_tables() { GX_ONCE(bool, env_int("GNXR_SHADE_LDS_TABLES", 1) != 0); }
    // GNXR_SHADE_STREAMS: 0 / 1 = never / always run the class kernels on the auxiliary streams (default -1 = with three or more).  Once
    static int shade_streams() { GX_ONCE(int, env_int("GNXR_SHADE_STREAMS", -1)); }
    // GNXR_VOL_PACK: 0 = VolPath never packs its survivors to the front of the state arrays (experiment; default 1).  Once
    static bool vol_pack() { GX_ONCE(bool, env_int("GNXR_VOL_PACK", 1) != 0); }
#undef GX_ONCE
    // GNXR_VOLMEDIA_STEP_CAP: tracking steps k_vol_media takes before it hands a segment back, 0 = no cap (default 64).  Per call (launch)
    static int volmedia_step_cap() { return env_set("GNXR_VOLMEDIA_STEP_CAP") ? std::max(0, env_int("GNXR_VOLMEDIA_STEP_CAP", 0)) : 64; }
    // GNXR_NO_ESCAPE_QUEUE: set = escaped rays share the shade queues of the material classes (default unset).  Per call (render)
    static bool no_escape_queue() { return env_set("GNXR_NO_ESCAPE_QUEUE"); }
    // GNXR_NO_MATERIAL_QUEUES: set = all class-1 (glossy) materials share one shade queue and k_shade<LM_GLOSSY>, whatever their kind (default
    // unset: a queue and a narrow kernel per kind where the four queues allow, plan_shade_queues).  Per call (render)
    static bool no_material_queues() { return env_set("GNXR_NO_MATERIAL_QUEUES"); }
    // GNXR_NO_NARROW_SHADE: set = the queues of the kinds launch k_shade<LM_GLOSSY> instead of their narrow kernels (experiment: the split
    // without the specialisation; default unset).  Per call (render)
    static bool no_narrow_shade() { return env_set("GNXR_NO_NARROW_SHADE"); }
    // GNXR_NO_MIS_DEFER: set = a scene lit by area lights alone is shaded by k_shade<LM, LT_AREA> as every other scene, not by the kernels with
    // the MIS half of EstimateDirect reordered (SM_DIR_FIRST / SM_DEFER; same image and counts bit for bit: the A/B and test switch; default
    // unset).  Per call (render)
    static bool no_mis_defer() { return env_set("GNXR_NO_MIS_DEFER"); }
    // GNXR_MIS_DEFER_STEP: 1 = direction first only (SM_DIR_FIRST), 2 = and the rare vertices deferred to a list per wave (SM_DEFER)
    // (experiment: each step's A/B; default 2).  Per call (render)
    static int mis_defer_step() { const int v = env_int("GNXR_MIS_DEFER_STEP", 2); return v == 1 ? 1 : 2; }
    // GNXR_MIS_DEFER_DRAIN_AT: entries of a wave's list at which the wave drains it between two vertices, 1 .. 64 (default 64; small values
    // let tests reach the drains inside the loop).  Per call (render)
    static int mis_defer_drain_at() { return std::max(1, std::min(64, env_int("GNXR_MIS_DEFER_DRAIN_AT", 64))); }
    // GNXR_NO_TRACE_NEE_APPLY: set = k_trace4 adds no light estimates in its set-up batches; k_nee_combine adds them all after the launch (same
    // image and counts bit for bit: the A/B and test switch; default unset).  Per call (render)
    static bool no_trace_nee_apply() { return env_set("GNXR_NO_TRACE_NEE_APPLY"); }
    // GNXR_HOST_LIGHT_GRID: set = the spatial light table is built on the host (default unset).  Per call (ensure_grid)
    static bool host_light_grid() { return env_set("GNXR_HOST_LIGHT_GRID"); }
    // GNXR_BINARY_BVH: set = the scene renders on the binary tree, never the 4-wide one (default unset).  Per call (scene creation)
    static bool binary_bvh() { return env_set("GNXR_BINARY_BVH"); }
    // GNXR_CLOSEST_LDS_LEVELS: most levels of a closest-point walk's stack kept in LDS, 1 .. 24 (default 16; small values let tests reach the
    // global spill on shallow trees).  Per call (launch)
    // GNXR_CLOSEST_BIN_MIN: queries of a closest-point call from which it bins them by Morton key before the walk, at least 1 (default 65536;
    // 1 lets tests bin small batches, a huge value switches binning off for A/B timing).  Per call (launch)
    static long long closest_bin_min() { const char *e = getenv("GNXR_CLOSEST_BIN_MIN"); return e ? std::max(1ll, atoll(e)) : 65536ll; }
    static int closest_lds_levels() { return std::max(1, std::min(24, env_int("GNXR_CLOSEST_LDS_LEVELS", 16))); }
    // GNXR_ALLHITS_LDS_LEVELS: most levels of an all-hits walk's stack kept in LDS, 1 .. 32 (default 16; small values let tests reach the
    // global spill on shallow trees).  Per call (launch)
    static int allhits_lds_levels() { return std::max(1, std::min(32, env_int("GNXR_ALLHITS_LDS_LEVELS", 16))); }
    // GNXR_NEAR_LDS_LEVELS: most levels of a neighbour walk's stack kept in LDS, 1 .. 24 (default 16: with the 8-byte entries of the
    // NEAREST mode a block's stack is 32 KB, five blocks fill a CU's LDS; small values let tests reach the global spill on shallow
    // trees).  Per call (launch)
    static int near_lds_levels() { return std::max(1, std::min(24, env_int("GNXR_NEAR_LDS_LEVELS", 16))); }
    // GNXR_SPHERECAST_LDS_LEVELS: most levels of a sphere cast's stack (8-byte entries) kept in LDS, 1 .. 24 (default 16: a block's stack
    // is 32 KB, five blocks fill a CU's LDS; small values let tests reach the global spill on shallow trees).  Per call (launch)
    static int spherecast_lds_levels() { return std::max(1, std::min(24, env_int("GNXR_SPHERECAST_LDS_LEVELS", 16))); }
    // GNXR_OVERLAP_LDS_LEVELS: most levels of a box overlap walk's stack (4-byte entries) kept in LDS, 1 .. 32 (default 16: a block's stack
    // is 16 KB; small values let tests reach the global spill on shallow trees).  Per call (launch)
    static int overlap_lds_levels() { return std::max(1, std::min(32, env_int("GNXR_OVERLAP_LDS_LEVELS", 16))); }
};

int ensure_device() {
    // the current device is per host thread in HIP: a call from a thread other than the one that ran gnxr_init (the Qt
    // RenderThread of INTEGRATION.md) must not silently land on device 0
    if (g_device >= 0) { HIP_TRY(hipSetDevice(g_device)); return GNXR_OK; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (%s); libgnxr has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "0 devices");
        return GNXR_ERR_NO_DEVICE;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    g_num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    g_device = dev;
    if (const int v = Knobs::trace_blocks_per_cu()) g_trace_blocks_per_cu = v;
    if (const int v = Knobs::grid_blocks_per_cu()) g_grid_bpc = v;
    return GNXR_OK;
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    int alloc(size_t count) {
        if (count <= n && p) return GNXR_OK;
        release();
        if (count == 0) count = 1;
        HIP_TRY(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
        return GNXR_OK;
    }
    int upload(const T *src, size_t count) {
        int rc = alloc(count);
        if (rc) return rc;
        if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return GNXR_OK;
    }
    template <typename V> int upload(const V &v) { return upload(v.data(), v.size()); }
};

int grid_for(long long n, int blocks_per_cu = 0) {
    if (blocks_per_cu <= 0) blocks_per_cu = g_grid_bpc;
    long long need = (n + kBlock - 1) / kBlock;
    long long cap = (long long)g_num_cus * blocks_per_cu;
    return (int)std::max<long long>(1, std::min(need, cap));
}

}  // namespace
