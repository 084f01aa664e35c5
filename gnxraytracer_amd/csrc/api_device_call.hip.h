// api_device_call.hip.h -- the front end the entry points on device memory share: which copy of the scene a call works on (DeviceCall),
// its stream-ordered scratch (StreamScratch), the parameter checks, and the small pieces render_one and the feature buffers both need.
// Part of api.hip's translation unit (after api_scene.hip.h, before api_render.hip.h).
#pragma once

// ---- the copy of the scene that holds a call's arrays ----

// The copy of `s` on the device that holds `ptr` (nullptr and the error set when `ptr` is not device memory, or no copy lives there).
// `bytes`: the extent the call reads or writes, checked against the allocation whenever the runtime reports its range.
static gnxr_scene *query_replica(gnxr_scene *s, const void *ptr, size_t bytes, const char *what) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, ptr);
    (void)hipGetLastError();   // memory the runtime has never seen makes the call fail: that is the answer, not an error of later calls
    if (e != hipSuccess || a.type != hipMemoryTypeDevice) {
        set_error("%s is not device memory (host arrays go through gnxr_trace_closest / gnxr_trace_any)", what);
        return nullptr;
    }
    gnxr_scene *r = nullptr;
    for (size_t i = 0; !r && i < s->n_copies(); ++i) if (s->copy(i)->device == a.device) r = s->copy(i);
    if (!r) { set_error("%s lives on device %d, which holds no copy of the scene", what, a.device); return nullptr; }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) == hipSuccess && base && (const char *)ptr + bytes > (const char *)base + size) {
        set_error("%s: %zu bytes from %p run past the end of its allocation (%zu bytes from %p)", what, bytes, ptr, size, (void *)base);
        return nullptr;
    }
    (void)hipGetLastError();
    return r;
}

// The copy of `s` on the device that holds every listed array (nullptr and the error set otherwise)
struct QueryArg { const void *p; size_t bytes; const char *what; };
static gnxr_scene *query_replica_all(gnxr_scene *s, const QueryArg *args, int n_args) {
    gnxr_scene *r = nullptr;
    for (int i = 0; i < n_args; ++i) {
        if (!args[i].p) continue;   // an optional array that was not given
        gnxr_scene *ri = query_replica(s, args[i].p, args[i].bytes, args[i].what);
        if (!ri) return nullptr;
        if (r && ri != r) { set_error("%s and %s live on different devices", args[0].what, args[i].what); return nullptr; }
        r = ri;
    }
    return r;
}

// One call on device memory: binds the copy of the scene that holds the call's arrays (`r`) and, when the call ends on whatever path,
// makes the primary's device current again -- every entry point leaves the device current that gnxr_init bound.
// Locks are the entry point's own business, taken after bind() and in one order: the primary's render_mutex, then the replica's
// (render_sharded's order).  A call that needs state a render rebuilds on `r` takes both (gnxr_light_sample_device: the selection
// table); one that runs render_one's loops or its own passes on `r` holds r's alone (gnxr_li_device, views, feature buffers); the
// others read tables that never change and take none.
struct DeviceCall {
    gnxr_scene *r = nullptr;
    int restore = -1;   // the device to make current again (-1: it never changed)
    template <int N>
    int bind(gnxr_scene *s, const QueryArg (&args)[N]) {
        if (!(r = query_replica_all(s, args, N))) return GNXR_ERR_INVALID;
        if (r != s) restore = s->device;
        return r->bind();
    }
    // a call without a scene (gnxr_camera_rays_device): the device of its arrays
    int bind(int device) {
        if (device != g_device) restore = g_device;
        HIP_TRY(hipSetDevice(device));
        return GNXR_OK;
    }
    ~DeviceCall() { if (restore >= 0) (void)hipSetDevice(restore); }
};

// A call's scratch on its stream: allocated, used and returned in stream order, on every exit path.  Its size never depends on what
// another stream does, so calls on several streams and a render in flight share nothing.
struct StreamScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    hipError_t alloc(size_t bytes, hipStream_t stream) {
        st = stream;
        const hipError_t e = hipMallocAsync((void **)&p, bytes, st);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    ~StreamScratch() { if (p) (void)hipFreeAsync(p, st); }
};

// start and end of a call's work on its stream (gnxr_stats::seconds_render); destroyed on every exit path
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// ---- parameter checks (no device, no handle: they run before ensure_device()) ----

static int invalid_render_params() { set_error("invalid render parameters"); return GNXR_ERR_INVALID; }

// the image size and the range of samples [spp_begin, spp_end) of spp (spp_end <= 0: up to spp)
static bool image_and_samples_ok(const gnxr_render_params &p) {
    return p.width > 0 && p.height > 0 && p.spp > 0 && p.spp_begin >= 0 && p.spp_end <= p.spp && p.spp_begin < (p.spp_end > 0 ? p.spp_end : p.spp);
}

// the calls that do not shard (Li for caller rays, views, feature buffers); `why`: what a caller that shards does instead
static int check_unsharded(const gnxr_render_params &p, const char *call, const char *why) {
    if (p.shard_index == 0 && p.shard_count >= 0 && p.shard_count <= 1 && p.shard_rows >= 0 && p.shard_rows <= 1) return GNXR_OK;
    set_error("%s: shard_index must be 0, shard_count and shard_rows 0 or 1 (%s)", call, why);
    return GNXR_ERR_INVALID;
}

// A list of views is one path population of n_views * W * H pixels: a slot is sample * pixels + pixel in an int, and the traversal's
// work cursor counts three items per slot in 32 bits.  The pixel count goes to *total.
static int check_view_pixels(const gnxr_render_params &p, int n_views, const char *call, long long *total) {
    const long long kMaxViewPixels = ((1ll << 32) - 1) / 3;
    *total = (long long)n_views * p.width * p.height;
    if (*total <= kMaxViewPixels) return GNXR_OK;
    set_error("%s: n_views * width * height = %lld pixels overflow the 32-bit path indexing (at most %lld per call); split the list of views", call, *total, kMaxViewPixels);
    return GNXR_ERR_INVALID;
}
// ... and every view sits in no medium (-1) or in one of the scene's (camera_media == nullptr: none does).  Reads the handle.
static int check_view_media(const gnxr_scene *s, const int32_t *camera_media, int n_views, const char *call) {
    const int n_media = (int)s->cs.media.size();
    for (int v = 0; camera_media && v < n_views; ++v)
        if (camera_media[v] < -1 || camera_media[v] >= n_media) { set_error("%s: camera_media[%d] = %d is outside [-1, %d)", call, v, camera_media[v], n_media); return GNXR_ERR_INVALID; }
    return GNXR_OK;
}

// ---- shared by render_one and the feature buffers ----

// The device sampler keeps the Halton index in 32 bits.  Every index a call draws is below stride * (spp * light_samples + 1)
// (light_samples: the largest Light::nSamples the array samples multiply the index by, else 1); reversedDigits of base b stays below
// b * index (device_sampler.h), which is what base32_max records.
static int halton_index_bound(DHalton *h, int spp, int light_samples) {
    const unsigned long long bound = (unsigned long long)h->stride * ((unsigned long long)spp * light_samples + 1);
    if (bound >= (1ull << 32)) { set_error("spp too large for 32-bit Halton indices"); return GNXR_ERR_UNSUPPORTED; }
    h->base32_max = (int32_t)std::min<unsigned long long>(0x7fffffffull, 0xffffffffull / bound);
    return GNXR_OK;
}

// the DCamera record of every view; media: one medium per view (checked by check_view_media), or nullptr: all -1
static void make_view_cameras(const gnxr_camera *cameras, const int32_t *media, int n_views, int W, int H, DCamera *out) {
    for (int v = 0; v < n_views; ++v) out[v] = make_camera(cameras[v], W, H, media ? media[v] : -1);
}

// ---- the reference's binary walk over caller rays: trees the 4-wide encoding cannot hold (or GNXR_BINARY_BVH at creation) ----
// 64 stack entries run at 2 blocks per CU, 32 at 5.  any == false: Scene::Intersect, out = gnxr_hit[n]; any == true: Scene::IntersectP, out = uint8_t[n]
static int binary_trace_api(const gnxr_scene *r, const DScene &sc, const gnxr_ray *d_rays, long long n, void *out, bool any, hipStream_t st) {
    const bool big = r->stack_size > 32;
    if (!any) {
        if (big) hipLaunchKernelGGL((k_trace_closest_api<64>), dim3(grid_for(n, 2)), dim3(kBlock), 0, st, sc, d_rays, n, (gnxr_hit *)out);
        else hipLaunchKernelGGL((k_trace_closest_api<32>), dim3(grid_for(n, 5)), dim3(kBlock), 0, st, sc, d_rays, n, (gnxr_hit *)out);
    } else {
        if (big) hipLaunchKernelGGL((k_trace_any_api<64>), dim3(grid_for(n, 2)), dim3(kBlock), 0, st, sc, d_rays, n, (unsigned char *)out);
        else hipLaunchKernelGGL((k_trace_any_api<32>), dim3(grid_for(n, 5)), dim3(kBlock), 0, st, sc, d_rays, n, (unsigned char *)out);
    }
    HIP_TRY(hipGetLastError());
    return GNXR_OK;
}
