// host.hpp -- host-side helpers shared by every translation unit of libtscode_hip (one .hip per kernel family; what only the entry points on
// host arrays need is in call.hpp, what only the prune and the units around it need in prune_api.hpp and prune_host.hpp).  The library is built with -fvisibility=hidden, so none of this is exported.
#pragma once

#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>

#include "common.hpp"
#include "embed_clash.hpp"

using namespace tsc;

static inline int make_frag_table(const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf, int n_mols, FragTable *ft) {
    TSC_REQUIRE(frag_off && n_atoms && n_conf, "null fragment table");
    TSC_REQUIRE(n_mols >= 1 && n_mols <= MAX_MOLS, "n_mols = %d not in 1..%d", n_mols, MAX_MOLS);
    memset(ft, 0, sizeof(*ft));
    ft->n_mols = n_mols;
    int off = 0;
    for (int m = 0; m < n_mols; ++m) {
        TSC_REQUIRE(n_atoms[m] > 0 && n_conf[m] > 0 && frag_off[m] >= 0, "bad fragment %d", m);
        ft->frag_off[m] = frag_off[m];
        ft->n_atoms[m] = n_atoms[m];
        ft->n_conf[m] = n_conf[m];
        ft->atom_off[m] = off;
        off += n_atoms[m];
    }
    for (int m = n_mols; m <= MAX_MOLS; ++m) ft->atom_off[m] = off;
    ft->n_total = off;
    return 0;
}

static inline int grid_for(int64_t work_items, int per_block, int cap = 256 * 16) {
    return int(std::max<int64_t>(1, std::min<int64_t>(ceil_div<int64_t>(work_items, per_block), cap)));
}

// a launch with more dynamic LDS than the 64 KB a kernel may use without asking
template <typename K>
static inline int lds_attribute(K kernel, size_t lds) {
    if (lds > 64 * 1024) TSC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    return 0;
}

template <typename T>
static inline int upload(tsc_ctx *c, Scratch &s, const T *host, size_t count, T **dev) {
    TSC_TRY(s.get(count ? count : 1, dev));
    if (count) TSC_HIP(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}

static inline int64_t frags_total_doubles(const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf, int n_mols) {
    int64_t end = 0;
    for (int m = 0; m < n_mols; ++m) end = std::max<int64_t>(end, frag_off[m] + int64_t(n_conf[m]) * n_atoms[m] * 3);
    return end;
}


// Fetch a device scalar that the work enqueued so far has produced WITHOUT waiting for what is enqueued after this call:
// the copy goes to the auxiliary stream behind an event; read_i32_finish waits for that stream only.
static inline int read_i32_begin(tsc_ctx *c, const int32_t *dev) {
    TSC_HIP(hipEventRecord(c->ev_sync, c->stream));
    TSC_HIP(hipStreamWaitEvent(c->aux_stream, c->ev_sync, 0));
    TSC_HIP(hipMemcpyAsync(c->pinned, dev, sizeof(int32_t), hipMemcpyDeviceToHost, c->aux_stream));
    return 0;
}
static inline int read_i32_finish(tsc_ctx *c, int32_t *host_out) {
    TSC_HIP(hipStreamSynchronize(c->aux_stream));
    *host_out = *static_cast<int32_t *>(c->pinned);
    return 0;
}

static inline int read_i32(tsc_ctx *c, const int32_t *dev, int32_t *host_out) {
    TSC_HIP(hipMemcpyAsync(c->pinned, dev, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    *host_out = *static_cast<int32_t *>(c->pinned);
    return 0;
}


static inline int get_event(tsc_ctx *c, hipEvent_t *e) {
    if (!c->event_pool.empty()) {
        *e = c->event_pool.back();
        c->event_pool.pop_back();
        return 0;
    }
    TSC_HIP(hipEventCreate(e));
    return 0;
}

