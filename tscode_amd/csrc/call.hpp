// call.hpp -- what the entry points that take host arrays and hand host arrays back share (topology, nci, orbitals, diverse,
// rot_corr, adjacent, prune_batch): the device side of one such call (HostCall), the event timer of the profiling option (StageTimer), the
// dispatch on a kernel's word count (with_words) and the two argument checks that topology and nci have in common.
#pragma once

#include <type_traits>
#include <vector>

#include "common.hpp"
#include "embed_clash.hpp"

namespace tsc {

// The device side of one host-array entry point.  Copies from and into the CALLER's host arrays are enqueued long before the entry
// returns: whatever path leaves it -- an error included -- the stream is idle first, so that no copy reads or lands in memory the
// caller (or the entry itself: a std::vector, a stack variable) has meanwhile freed.  A host variable that fetch() fills is
// declared in front of the HostCall, so that it outlives it.
class HostCall {
    tsc_ctx *c_;
    DeviceGuard guard_;   // (members in this order: scratch goes back to the cache before the device is restored)
    Scratch s_;
    struct Out {
        void *host;
        const void *dev;
        size_t bytes;
    };
    std::vector<Out> outs_;
    bool pending_ = false;   // something was enqueued through this object that the stream has not been waited for since

   public:
    explicit HostCall(tsc_ctx *c) : c_(c), guard_(c->device), s_(c) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    // (the body runs before the members go: the stream is idle before the blocks are handed back and the device restored)
    ~HostCall() {
        if (pending_) (void)hipStreamSynchronize(c_->stream);
    }

    Scratch &scratch() { return s_; }   // blocks that are neither uploaded nor copied back

    // a device copy of host[count] (one element is allocated for none)
    template <typename T>
    int in(const T *host, size_t count, T **dev) {
        TSC_TRY(s_.get(count ? count : 1, dev));
        if (count) {
            pending_ = true;
            TSC_HIP(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, c_->stream));
        }
        return 0;
    }
    template <typename T>
    int in(const T *host, size_t count, const T **dev) {
        T *d = nullptr;
        TSC_TRY(in(host, count, &d));
        *dev = d;
        return 0;
    }

    // device room for an output the caller wants (host != null), copied to host[count] by finish(); no room and *dev = null otherwise
    template <typename T>
    int out(T *host, size_t count, T **dev) {
        *dev = nullptr;
        if (!host) return 0;
        TSC_TRY(s_.get(count, dev));
        outs_.push_back({host, *dev, count * sizeof(T)});
        return 0;
    }

    // dev[count] to host[count] at this point of the stream
    template <typename T>
    int fetch(T *host, const T *dev, size_t count) {
        pending_ = true;
        TSC_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c_->stream));
        return 0;
    }

    // the outputs in the order they were registered, then the call's one wait for the stream
    int finish() {
        for (const Out &o : outs_)
            if (o.bytes) TSC_TRY(fetch(static_cast<char *>(o.host), static_cast<const char *>(o.dev), o.bytes));
        TSC_HIP(hipStreamSynchronize(c_->stream));
        pending_ = false;
        return 0;
    }
};

// HIP-event times of the stages of a call, taken only under the context option "pass_timing" >= 1 (the tools/*_profile.py).  Where
// an event cannot be created the slot keeps its -1: a timed call is a measurement, not the product's path.
struct StageTimer {
    tsc_ctx *c;
    bool on;
    hipEvent_t ev[2] = {nullptr, nullptr};
    explicit StageTimer(tsc_ctx *ctx) : c(ctx), on(ctx->opt.pass_timing >= 1) {
        if (on && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) on = false;
    }
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void begin() {
        if (on) (void)hipEventRecord(ev[0], c->stream);
    }
    void end(float *slot) {   // (synchronises)
        if (!on) return;
        (void)hipEventRecord(ev[1], c->stream);
        (void)hipEventSynchronize(ev[1]);
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *slot = ms;
    }
};

// f(std::integral_constant<int, W>{}) for W = w clamped to 1 .. 8: the widths the kernels templated on a word or tile count exist in
template <typename F>
void with_width(int w, F &&f) {
    switch (w) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}
// ... for the 64-bit words that hold one bit per atom of n
template <typename F>
void with_words(int n, F &&f) {
    with_width(ceil_div(n, 64), std::forward<F>(f));
}

// The class of every atom and the thresholds of the class pairs, as topology and nci take them: atom_class u8[n_atoms] below
// n_classes, thr f64[n_classes, n_classes] finite and not negative.  table f64[T, T] (T > n_classes) receives the squared bound
// of every pair in its leading n_classes x n_classes corner (0 for a threshold of 0: never); the rest is left as it is.
inline int check_class_table(const char *who, const uint8_t *atom_class, int n_atoms, const double *thr, int n_classes, double *table, int T) {
    for (int i = 0; i < n_atoms; ++i)
        TSC_REQUIRE(atom_class[i] < n_classes, "%s: class %d of atom %d with %d classes", who, int(atom_class[i]), i, n_classes);
    for (int p = 0; p < n_classes; ++p)
        for (int q = 0; q < n_classes; ++q) {
            const double t = thr[p * n_classes + q];
            TSC_REQUIRE(std::isfinite(t) && t >= 0.0, "%s: thr[%d][%d] = %g is negative or not finite", who, p, q, t);
            table[p * T + q] = clash_sq_bound(t);
        }
    return 0;
}

// A list of atoms set apart (`noun`: "excluded", "constrained"): idx i32[n_idx] shared by all structures, or with per_struct
// i32[n_structs, n_idx] padded with -1, which is checked only where it lies on the host (on_host).  A shared list sets its bits in
// words u64[ceil_div(n_atoms, 64)] (zeroed by the caller) and *n_per_struct = 0; a per-structure list leaves the words alone and
// *n_per_struct = n_idx, for the kernel to read the rows.
inline int check_index_list(const char *who, const char *noun, const int32_t *idx, int n_idx, int per_struct, bool on_host, int64_t n_structs,
                            int n_atoms, uint64_t *words, int *n_per_struct) {
    const bool rows = n_idx > 0 && per_struct != 0;
    *n_per_struct = rows ? n_idx : 0;
    if (n_idx > 0 && (!rows || on_host)) {
        const int64_t count = rows ? n_structs * n_idx : n_idx;
        for (int64_t q = 0; q < count; ++q) {
            const int32_t e = idx[q];
            TSC_REQUIRE(e >= -1 && e < n_atoms, "%s: %s atom %d with %d atoms", who, noun, e, n_atoms);
            if (!rows && e >= 0) words[e >> 6] |= 1ull << (e & 63);
        }
    }
    return 0;
}

}  // namespace tsc
