// ctx.hip -- library / context entry points of include/tscode_hip.h and the tunables
// gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"

// --------------------------------------------------------------------------------------------------
// library / context

extern "C" __attribute__((visibility("default"))) int tsc_version(void) { return TSC_VERSION; }
extern "C" __attribute__((visibility("default"))) const char *tsc_last_error(void) { return g_err; }
#ifndef TSC_CSRC_DIGEST
#define TSC_CSRC_DIGEST "unrecorded"
#endif
extern "C" __attribute__((visibility("default"))) const char *tsc_build_digest(void) { return TSC_CSRC_DIGEST; }

extern "C" __attribute__((visibility("default"))) int tsc_device_count(void) {
    TSC_API_GUARD_BEGIN
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(TSC_ERR_NO_DEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    return n;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_ctx_create(int device, tsc_ctx **out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(out != nullptr, "tsc_ctx_create: out is null");
    *out = nullptr;
    int n = tsc_device_count();
    if (n < 0) return n;
    if (n == 0) return fail(TSC_ERR_NO_DEVICE, "no HIP device visible: libtscode_hip has no CPU path");
    TSC_REQUIRE(device >= 0 && device < n, "tsc_ctx_create: device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    TSC_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TSC_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    DeviceGuard guard(device);
    tsc_ctx *c = new (std::nothrow) tsc_ctx();
    if (!c) return fail(TSC_ERR_NOMEM, "out of host memory");
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        // the side chain of the pipeline (sample embed, moments, basis) is three tiny kernels running beside the clash kernel, which
        // fills the device: at the highest priority their workgroups are placed as soon as any of the clash kernel's retire
        int lo = 0, hi = 0;
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->basis_stream, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) {
        c->pinned_bytes = 16384;
        e = hipHostMalloc(&c->pinned, c->pinned_bytes, hipHostMallocDefault);
    }
    if (e != hipSuccess) {
        (void)tsc_ctx_destroy(c);       // streams, events and the pinned buffer created so far
        return fail(TSC_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_ctx_destroy(tsc_ctx *c) {
    TSC_API_GUARD_BEGIN
    if (!c) return 0;
    DeviceGuard guard(c->device);
    // everything enqueued on any of the context's streams ends before what it uses is freed (also the teardown of a context
    // whose creation failed half way: whatever exists by then is released here)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    if (c->basis_stream) (void)hipStreamSynchronize(c->basis_stream);
    // objects that are still alive go with their context, newest first (their blocks are the context's, a prune run's events join its
    // pool below, an exchange closes its peers' mappings): a host whose finalisers come in no particular order -- Python collecting a run
    // and its engine in one cycle -- must not hand one to its tsc_*_destroy after this
    c->owned.destroy_all();
    for (auto &kv : c->cache) (void)hipFree(kv.second);
    for (auto &kv : c->live) (void)hipFree(kv.first);
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev_sync) (void)hipEventDestroy(c->ev_sync);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->basis_stream) (void)hipStreamDestroy(c->basis_stream);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
    TSC_API_GUARD_END
}

static hipStream_t g_dummy;
extern "C" __attribute__((visibility("default"))) int tsc_ctx_set_stream(tsc_ctx *c, void *hip_stream) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c != nullptr, "null context");
    DeviceGuard guard(c->device);
    TSC_HIP(hipStreamSynchronize(c->stream));
    if (hip_stream) {
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        c->stream = static_cast<hipStream_t>(hip_stream);
        c->own_stream = false;
    } else if (!c->own_stream) {
        TSC_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    (void)g_dummy;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_ctx_synchronize(tsc_ctx *c) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c != nullptr, "null context");
    DeviceGuard guard(c->device);
    TSC_HIP(hipStreamSynchronize(c->stream));
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_malloc(tsc_ctx *c, size_t bytes, void **dptr) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && dptr, "null argument");
    DeviceGuard guard(c->device);
    TSC_HIP(hipMalloc(dptr, bytes ? bytes : 8));
    return 0;
    TSC_API_GUARD_END
}
extern "C" __attribute__((visibility("default"))) int tsc_free(tsc_ctx *c, void *dptr) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c != nullptr, "null context");
    DeviceGuard guard(c->device);
    TSC_HIP(hipStreamSynchronize(c->stream));
    if (dptr) TSC_HIP(hipFree(dptr));
    return 0;
    TSC_API_GUARD_END
}
extern "C" __attribute__((visibility("default"))) int tsc_memcpy_h2d(tsc_ctx *c, void *dst, const void *src, size_t bytes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && (bytes == 0 || (dst && src)), "null argument");
    DeviceGuard guard(c->device);
    if (bytes) {
        TSC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        TSC_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
    TSC_API_GUARD_END
}
extern "C" __attribute__((visibility("default"))) int tsc_memcpy_d2h(tsc_ctx *c, void *dst, const void *src, size_t bytes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && (bytes == 0 || (dst && src)), "null argument");
    DeviceGuard guard(c->device);
    if (bytes) {
        TSC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        TSC_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
    TSC_API_GUARD_END
}
extern "C" __attribute__((visibility("default"))) int tsc_timer_begin(tsc_ctx *c) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c != nullptr, "null context");
    DeviceGuard guard(c->device);
    TSC_HIP(hipEventRecord(c->ev0, c->stream));
    return 0;
    TSC_API_GUARD_END
}
extern "C" __attribute__((visibility("default"))) int tsc_timer_end(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "null argument");
    DeviceGuard guard(c->device);
    TSC_HIP(hipEventRecord(c->ev1, c->stream));
    TSC_HIP(hipEventSynchronize(c->ev1));
    TSC_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return 0;
    TSC_API_GUARD_END
}


#ifdef TSC_DBG_STAMPS
// measurement builds only: the time stamps of the last stamped pair-kernel launch, 8 per wavefront (tools/stamps.py)
extern "C" __attribute__((visibility("default"))) int tsc_debug_stamps(tsc_ctx *c, unsigned long long *dst, int64_t max_waves, int64_t *n_waves) {
    TSC_API_GUARD_BEGIN
    DeviceGuard guard(c->device);
    TSC_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = std::min(max_waves, c->dbg_waves);
    if (n > 0) TSC_HIP(hipMemcpy(dst, c->dbg_buf, size_t(n) * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n_waves = n;
    return 0;
    TSC_API_GUARD_END
}
#endif

// Tunables: the table of options.hpp holds each option's name, member and rule; the defaults are the initialisers of tsc_options.
extern "C" __attribute__((visibility("default"))) int tsc_ctx_set_option(tsc_ctx *c, const char *name, double value) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && name, "null argument");
    return option_set(c->opt, name, value, g_err, sizeof(g_err));
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_ctx_get_option(tsc_ctx *c, const char *name, double *value) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && name && value, "null argument");
    return option_get(c->opt, name, value, g_err, sizeof(g_err));
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_option_info(int index, const char **name, double *default_value) {
    TSC_API_GUARD_BEGIN
    if (option_info(index, name, default_value) != 0) return fail(TSC_ERR_INVALID, "tsc_option_info: no option %d", index);
    return 0;
    TSC_API_GUARD_END
}
