// api_device_call.hip.h -- the front end the entry points on device memory share: the one walk over a call's arrays (array_device,
// arrays_device, query_replica) with the checks that need no runtime (check_aligned, ranges_overlap), which device or copy of the scene a
// call works on (DeviceCall), its stream-ordered scratch (StreamScratch, StatusWord), the parameter checks, and the small pieces
// render_one and the feature buffers both need.  Part of api.hip's translation unit (after api_scene.hip.h, before api_render.hip.h).
#pragma once

// ---- the arrays of a call ----

// One array of a call: `bytes` is the extent the call reads or writes, `what` its name in the messages.  p == nullptr in a list: an
// optional array that was not given.
struct QueryArg { const void *p; size_t bytes; const char *what; };

// The device that holds `a` (-1 and the error set otherwise): `a` is device memory, accept(device) has nothing against its device (it
// sets the error when it has) and its extent ends inside its allocation whenever the runtime reports the range.  The only place that
// asks the runtime about a caller's array.  `name`: the call's name in front of every message ("": none); `hint`: what follows "is not
// device memory".
template <class Accept>
static int array_device(const char *name, const char *hint, const QueryArg &a, Accept accept) {
    const char *sep = *name ? ": " : "";
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, a.p);
    (void)hipGetLastError();   // memory the runtime has never seen makes the call fail: that is the answer, not an error of later calls
    if (e != hipSuccess || at.type != hipMemoryTypeDevice) { set_error("%s%s%s is not device memory%s", name, sep, a.what, hint); return -1; }
    if (!accept(at.device)) return -1;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a.p) == hipSuccess && base && (const char *)a.p + a.bytes > (const char *)base + size) {
        set_error("%s%s%s: %zu bytes from %p run past the end of its allocation (%zu bytes from %p)", name, sep, a.what, a.bytes, a.p, size, (void *)base);
        return -1;
    }
    (void)hipGetLastError();
    return at.device;
}

// The one device that holds every given array of the list (-1 and the error set otherwise): a call without a scene
static int arrays_device(const char *name, const char *hint, const QueryArg *args, int n_args) {
    int device = -1;
    for (int i = 0; i < n_args; ++i) {
        if (!args[i].p) continue;
        const int d = array_device(name, hint, args[i], [&](int on) {
            if (device < 0 || on == device) return true;
            set_error("%s%s%s and %s live on different devices", name, *name ? ": " : "", args[0].what, args[i].what);
            return false;
        });
        if (d < 0) return -1;
        device = d;
    }
    return device;
}

// every array of the list on a multiple of its align[i] bytes (a power of two; null is aligned).  No runtime.
static int check_aligned(const char *name, const QueryArg *args, const unsigned *align, int n_args) {
    for (int i = 0; i < n_args; ++i)
        if (((uintptr_t)args[i].p & (align[i] - 1)) != 0) { set_error("%s: %s is not %u-byte aligned", name, args[i].what, align[i]); return GNXR_ERR_INVALID; }
    return GNXR_OK;
}

// the byte ranges of two arrays share a byte (an array that was not given overlaps nothing)
static bool ranges_overlap(const QueryArg &a, const QueryArg &b) {
    const char *x = (const char *)a.p, *y = (const char *)b.p;
    return x && y && x < y + b.bytes && y < x + a.bytes;
}

// ---- the copy of the scene that holds a call's arrays ----

// The copy of `s` on the device that holds `a` (nullptr and the error set when `a` is not device memory, no copy lives there, or its
// extent runs past its allocation)
static gnxr_scene *query_replica(gnxr_scene *s, const QueryArg &a) {
    gnxr_scene *r = nullptr;
    const int device = array_device("", " (host arrays go through gnxr_trace_closest / gnxr_trace_any)", a, [&](int on) {
        for (size_t i = 0; !r && i < s->n_copies(); ++i) if (s->copy(i)->device == on) r = s->copy(i);
        if (!r) set_error("%s lives on device %d, which holds no copy of the scene", a.what, on);
        return r != nullptr;
    });
    return device < 0 ? nullptr : r;
}

// The copy of `s` on the device that holds every listed array (nullptr and the error set otherwise)
static gnxr_scene *query_replica_all(gnxr_scene *s, const QueryArg *args, int n_args) {
    gnxr_scene *r = nullptr;
    for (int i = 0; i < n_args; ++i) {
        if (!args[i].p) continue;   // an optional array that was not given
        gnxr_scene *ri = query_replica(s, args[i]);
        if (!ri) return nullptr;
        if (r && ri != r) { set_error("%s and %s live on different devices", args[0].what, args[i].what); return nullptr; }
        r = ri;
    }
    return r;
}

// One call on device memory: binds the copy of the scene that holds the call's arrays (`r`) or, for a call without a scene, the device
// that holds them (`device`) and, when the call ends on whatever path, makes the primary's device current again -- every entry point
// leaves the device current that gnxr_init bound.
// Locks are the entry point's own business, taken after bind() and in one order: the primary's render_mutex, then the replica's
// (render_sharded's order).  A call that needs state a render rebuilds on `r` takes both (gnxr_light_sample_device: the selection
// table); one that runs render_one's loops or its own passes on `r` holds r's alone (gnxr_li_device, views, feature buffers); the
// others read tables that never change and take none.
struct DeviceCall {
    gnxr_scene *r = nullptr;
    int device = -1;
    int restore = -1;   // the device to make current again (-1: it never changed)
    template <int N>
    int bind(gnxr_scene *s, const QueryArg (&args)[N]) {
        if (!(r = query_replica_all(s, args, N))) return GNXR_ERR_INVALID;
        if (r != s) restore = s->device;
        return r->bind();
    }
    // a call without a scene: the device of its arrays, or of the first n_args of them (`name`, `hint`: array_device's)
    int bind(const char *name, const QueryArg *args, int n_args, const char *hint = "") {
        if ((device = arrays_device(name, hint, args, n_args)) < 0) return GNXR_ERR_INVALID;
        if (device != g_device) restore = g_device;
        HIP_TRY(hipSetDevice(device));
        return GNXR_OK;
    }
    template <int N>
    int bind(const char *name, const QueryArg (&args)[N], const char *hint = "") { return bind(name, args, N, hint); }
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

// The 8-byte word in which a kernel flags a bad record, for a call whose scratch is that word alone
struct StatusWord {
    StreamScratch scratch;
    unsigned long long *d = nullptr;   // the kernel's argument
    int alloc(hipStream_t stream) {    // allocated and cleared on `stream`
        HIP_TRY(scratch.alloc(sizeof(*d), stream));
        d = reinterpret_cast<unsigned long long *>(scratch.p);
        HIP_TRY(hipMemsetAsync(d, 0, sizeof(*d), stream));
        return GNXR_OK;
    }
    int fetch(unsigned long long *word) {   // back on the host once the kernel has run: only the word is waited for, the records are on the stream
        HIP_TRY(hipMemcpyAsync(word, d, sizeof(*word), hipMemcpyDeviceToHost, scratch.st));
        HIP_TRY(hipStreamSynchronize(scratch.st));
        return GNXR_OK;
    }
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
static int check_view_pixels(int width, int height, int n_views, const char *call, long long *total) {
    const long long kMaxViewPixels = ((1ll << 32) - 1) / 3;
    *total = (long long)n_views * width * height;
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
