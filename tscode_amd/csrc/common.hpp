// common.hpp -- context, error plumbing and the stream-ordered scratch cache of libtscode_hip.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/tscode_hip.h"
#include "options.hpp"
#include "owned.hpp"

namespace tsc {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define TSC_HIP(call)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return ::tsc::fail(e_ == hipErrorOutOfMemory ? TSC_ERR_NOMEM : TSC_ERR_HIP, "%s failed: %s (%s:%d)", \
                               #call, hipGetErrorString(e_), __FILE__, __LINE__);                          \
    } while (0)

#define TSC_TRY(call)          \
    do {                       \
        int rc_ = (call);      \
        if (rc_ != 0) return rc_; \
    } while (0)

#define TSC_REQUIRE(cond, ...)                                        \
    do {                                                              \
        if (!(cond)) return ::tsc::fail(TSC_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// No C++ exception crosses the C ABI: every `extern "C"` entry point that returns a status runs its body between these two.
// The containers of tsc_ctx (std::map / std::vector) and `new` are what can throw in this library: std::bad_alloc -> TSC_ERR_NOMEM.
#define TSC_API_GUARD_BEGIN try {
#define TSC_API_GUARD_END                                                                                  \
    }                                                                                                      \
    catch (const std::bad_alloc &) {                                                                       \
        return ::tsc::fail(TSC_ERR_NOMEM, "%s: out of host memory", __func__);                             \
    }                                                                                                      \
    catch (const std::exception &e_) {                                                                     \
        return ::tsc::fail(TSC_ERR_INVALID, "%s: unexpected C++ exception: %s", __func__, e_.what());     \
    }                                                                                                      \
    catch (...) {                                                                                          \
        return ::tsc::fail(TSC_ERR_INVALID, "%s: unexpected C++ exception", __func__);                    \
    }

constexpr int WAVE = 64;

template <typename T>
__host__ __device__ inline T ceil_div(T a, T b) {
    return (a + b - 1) / b;
}

}  // namespace tsc

// One per (process, device).  All work is enqueued on `stream`; scratch blocks are recycled in
// stream order, so a block handed back by one call can be reused by the next without a sync.
struct tsc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;     // scalar read-backs that should not wait for work enqueued after their producer
    bool own_stream = true;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_sync = nullptr;         // orders the auxiliary stream behind the main one (no timing)
    hipStream_t basis_stream = nullptr;   // the descriptor basis of the pipeline, built beside the clash kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::multimap<size_t, void *> cache;  // free scratch blocks by size
    std::map<void *, size_t> live;        // blocks handed out
    void *pinned = nullptr;               // small pinned host buffer for scalar read-backs
    size_t pinned_bytes = 0;
    tsc_options opt;                      // the tunables (options.hpp)
    void *dbg_buf = nullptr;              // -DTSC_DBG_STAMPS builds: time stamps of the pair kernel's wavefronts
    size_t dbg_bytes = 0;
    int64_t dbg_waves = 0;
    // basis estimated by tsc_embed_clash_compact_dev beside its clash kernel, for the tsc_prune_create that follows (consumed once)
    double *eb_block = nullptr;           // [sample coordinates | moment accumulators | basis]
    int eb_h = 0, eb_samples = 0;
    bool eb_valid = false;
    // descriptors written by tsc_embed_masked_dev with the poses it embeds, for the tsc_prune_create that follows on the same
    // structures (consumed once; the run borrows the buffers until it is destroyed)
    float *xd_D = nullptr;
    double *xd_G = nullptr;
    unsigned *xd_dmax = nullptr;
    float *xd_heavy32 = nullptr;          // ... and the float32 copy of the heavy atoms written beside them (large runs)
    int64_t xd_h32_cap = 0;               // floats
    bool xd_h32_valid = false;
    int64_t xd_cap = 0;                   // structures the buffers hold
    int xd_h = 0;
    const double *xd_heavy = nullptr;     // the heavy-atom array they describe
    bool xd_valid = false;
    int xd_borrowers = 0;                 // live prune runs that read the xd_* buffers (tsc_prune_create borrowed them): no release / regrow meanwhile
    // The objects created from this context that are alive (owned.hpp); tsc_ctx_destroy destroys them with the context -- a host whose
    // finalisers run in no particular order cannot leak a run's blocks and events, or free them after the context.  The list's mutex also
    // guards the bookkeeping that prune runs of one context driven from DIFFERENT host threads touch (tsc_prune_create / tsc_prune_destroy):
    // the pinned flag words handed to runs (prune_api.hpp: PINNED_FLAG_OFFSET; bit s set = word s is some live run's) and xd_borrowers.
    tsc::OwnedList owned;
    unsigned long long flag_slots_used = 0;
    std::vector<int32_t> sample_host;     // pose indices of the basis sample of the last tsc_pipeline_dev call and their device copy
    int32_t *sample_dev = nullptr;
    double *mom_acc = nullptr;            // moment accumulators of the pipeline's basis chain (k_sample_moments adds, k_descriptor_basis clears)
    size_t mom_cap = 0;                   // doubles
    bool mom_clean = false;               // all zero (as far as the host can tell: every chain enqueued so far ended with the clearing kernel)
    std::vector<int32_t> slot_host;       // heavy-atom slot table of the last tsc_pipeline_dev call and its device copy
    int32_t *slot_dev = nullptr;
    std::vector<hipEvent_t> event_pool;   // recycled timing events of prune runs

    int alloc(size_t bytes, void **out) {
        if (bytes == 0) bytes = 8;
        bytes = (bytes + 255) & ~size_t(255);
        auto it = cache.lower_bound(bytes);
        if (it != cache.end() && it->first <= bytes * 2 + (1u << 20)) {
            *out = it->second;
            live[*out] = it->first;
            cache.erase(it);
            return 0;
        }
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            // drop the cache and retry once
            (void)hipGetLastError();
            trim();
            e = hipMalloc(&p, bytes);
            if (e != hipSuccess) return tsc::fail(TSC_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
        live[p] = bytes;
        *out = p;
        return 0;
    }
    void release(void *p) {
        if (!p) return;
        auto it = live.find(p);
        if (it == live.end()) return;
        cache.emplace(it->second, p);
        live.erase(it);
    }
    void trim() {
        (void)hipStreamSynchronize(stream);
        for (auto &kv : cache) (void)hipFree(kv.second);
        cache.clear();
    }
};

namespace tsc {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---- what owned.hpp declares and only the context can do ----
inline Scratch::~Scratch() {
    for (void *p : blocks) ctx->release(p);
}
inline int Scratch::take(size_t bytes, void **out) {
    TSC_TRY(ctx->alloc(bytes, out));
    blocks.push_back(*out);
    return 0;
}
inline void Scratch::give_back(void *p) {
    auto it = std::find(blocks.begin(), blocks.end(), p);
    if (it == blocks.end()) return;
    blocks.erase(it);
    ctx->release(p);
}

// The body of every tsc_<kind>_destroy.  What a kind holds beside its blocks goes in its destructor, what it keeps in the context in
// unlisted(); whether it waits is said in owned.hpp (destroy_waits), nowhere else.
template <typename T>
int destroy_owned(T *o) {
    if (!o) return 0;
    tsc_ctx *c = o->ctx;
    DeviceGuard guard(c->device);
    if (destroy_waits<T>) (void)hipStreamSynchronize(c->stream);
    c->owned.disown(o);
    delete o;
    return 0;
}

}  // namespace tsc
