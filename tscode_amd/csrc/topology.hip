// topology.hip -- launches and C ABI of the batched bond-graph / scramble check (topology.hpp; tscode/graph_manipulations.py:28-55,
// tscode/utils.py:293-314, :341-387).  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "topology.hpp"

#include <vector>

namespace {

using namespace tsc;

// HIP-event time of the kernel of the calling thread's latest tsc_bond_delta / tsc_bond_delta_dev, taken only under the context
// option "pass_timing" >= 1 (tools/topology_profile.py); -1 otherwise
thread_local float g_kernel_ms = -1.f;

struct Tables {
    TopoArgs a;
    std::vector<uint64_t> ref;  // the expected bonds as handed in, checked (empty: none)
};

// Everything that can be refused is refused here, before anything touches the device.
int make_tables(const char *who, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr, int n_classes,
                const uint8_t *active, const uint64_t *ref_bits, const int32_t *excluded, int n_excl, int excl_per_struct,
                bool excluded_on_host, int64_t max_newbonds, Tables *out) {
    TSC_REQUIRE(atom_class && thr, "%s: null argument", who);
    TSC_REQUIRE(n_structs >= 0, "%s: %lld structures", who, (long long)n_structs);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= TP_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, TP_MAX_ATOMS);
    TSC_REQUIRE(n_classes >= 1 && n_classes <= TP_MAX_CLASSES, "%s: %d element classes (1 .. %d)", who, n_classes, TP_MAX_CLASSES);
    TSC_REQUIRE(n_excl >= 0 && n_excl <= TP_MAX_EXCL, "%s: %d excluded atoms per structure (0 .. %d)", who, n_excl, TP_MAX_EXCL);
    TSC_REQUIRE(n_excl == 0 || excluded, "%s: %d excluded atoms without an array", who, n_excl);
    const int W = ceil_div(n_atoms, 64), T = n_classes + 1;
    TopoArgs &a = out->a;
    memset(&a, 0, sizeof(a));
    a.n_structs = n_structs, a.n = n_atoms, a.n_tab = T, a.max_newbonds = max_newbonds;
    for (int i = 0; i < n_atoms; ++i) {
        TSC_REQUIRE(atom_class[i] < n_classes, "%s: class %d of atom %d with %d classes", who, int(atom_class[i]), i, n_classes);
        a.cls[i] = (!active || active[i]) ? atom_class[i] : uint8_t(n_classes);
    }
    for (int p = 0; p < n_classes; ++p)
        for (int q = 0; q < n_classes; ++q) {
            const double t = thr[p * n_classes + q];
            TSC_REQUIRE(std::isfinite(t) && t >= 0.0, "%s: thr[%d][%d] = %g is negative or not finite", who, p, q, t);
            a.bound[p * T + q] = clash_sq_bound(t);  // (0 for a threshold of 0: never bonded)
        }
    const bool per_struct = n_excl > 0 && excl_per_struct != 0;
    a.n_excl = per_struct ? n_excl : 0;
    if (n_excl > 0 && (!per_struct || excluded_on_host)) {
        const int64_t count = per_struct ? n_structs * n_excl : n_excl;
        for (int64_t q = 0; q < count; ++q) {
            const int32_t e = excluded[q];
            TSC_REQUIRE(e >= -1 && e < n_atoms, "%s: excluded atom %d with %d atoms", who, e, n_atoms);
            if (!per_struct && e >= 0) a.excl_words[e >> 6] |= 1ull << (e & 63);
        }
    }
    if (ref_bits) {
        for (int i = 0; i < n_atoms; ++i)
            for (int w = 0; w < W; ++w) {
                uint64_t allowed = 0;  // columns j with i < j < n_atoms
                for (int b = 0; b < 64; ++b)
                    if (64 * w + b > i && 64 * w + b < n_atoms) allowed |= 1ull << b;
                TSC_REQUIRE((ref_bits[size_t(i) * W + w] & ~allowed) == 0, "%s: ref_bits row %d has bits outside the strict upper triangle", who,
                            i);
            }
        out->ref.assign(ref_bits, ref_bits + size_t(n_atoms) * W);
    }
    return 0;
}

template <int W>
void launch_w(tsc_ctx *c, const TopoArgs &a, const double *coords, const uint64_t *ref, const int32_t *excl, uint8_t *mask, int32_t *formed,
              int32_t *broken, uint64_t *adj) {
    const int blocks = grid_for(a.n_structs, 4);
    hipLaunchKernelGGL(k_bond_delta<W>, dim3(blocks), dim3(256), topo_lds_bytes(a.n), c->stream, a, coords, ref, excl, mask, formed, broken, adj);
}

// device pointers throughout, except the tables
int run_dev(tsc_ctx *c, Scratch &s, const Tables &t, const double *coords, const int32_t *excl_dev, uint8_t *mask, int32_t *formed,
            int32_t *broken, uint64_t *adj) {
    const TopoArgs &a = t.a;
    uint64_t *d_ref = nullptr;
    if (!t.ref.empty()) TSC_TRY(upload(c, s, t.ref.data(), t.ref.size(), &d_ref));
    const bool timed = c->pass_timing >= 1;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventPair {   // (a profiling path: the events live for this call only, whichever way it ends)
        hipEvent_t *e;
        ~EventPair() {
            for (int q = 0; q < 2; ++q)
                if (e[q]) (void)hipEventDestroy(e[q]);
        }
    } owner{ev};
    if (timed) {
        TSC_HIP(hipEventCreate(&ev[0]));
        TSC_HIP(hipEventCreate(&ev[1]));
        TSC_HIP(hipEventRecord(ev[0], c->stream));
    }
    switch (ceil_div(a.n, 64)) {
        case 1: launch_w<1>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 2: launch_w<2>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 3: launch_w<3>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 4: launch_w<4>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 5: launch_w<5>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 6: launch_w<6>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        case 7: launch_w<7>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
        default: launch_w<8>(c, a, coords, d_ref, excl_dev, mask, formed, broken, adj); break;
    }
    hipError_t launched = hipGetLastError();
    if (timed) {
        float ms = -1.f;
        if (launched == hipSuccess && hipEventRecord(ev[1], c->stream) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
            g_kernel_ms = ms;
    }
    TSC_HIP(launched);
    // the expected rows were uploaded from this call's own memory: they must have left it before it is freed
    if (d_ref) TSC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_topology_timings(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "tsc_topology_timings: null argument");
    *ms = g_kernel_ms;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_bond_delta_dev(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                         const uint8_t *atom_class, const double *thr, int n_classes,
                                                                         const uint8_t *active, const uint64_t *ref_bits, const int32_t *excluded,
                                                                         int n_excl, int excl_per_struct, int64_t max_newbonds, uint8_t *mask,
                                                                         int32_t *formed, int32_t *broken, uint64_t *adj) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && mask, "tsc_bond_delta_dev: null argument");
    Tables t;
    TSC_TRY(make_tables("tsc_bond_delta_dev", n_structs, n_atoms, atom_class, thr, n_classes, active, ref_bits, excluded, n_excl, excl_per_struct,
                        false, max_newbonds, &t));
    g_kernel_ms = -1.f;
    if (n_structs == 0) return 0;
    DeviceGuard guard(c->device);
    Scratch s(c);
    return run_dev(c, s, t, coords, t.a.n_excl ? excluded : nullptr, mask, formed, broken, adj);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_bond_delta(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                     const uint8_t *atom_class, const double *thr, int n_classes,
                                                                     const uint8_t *active, const uint64_t *ref_bits, const int32_t *excluded,
                                                                     int n_excl, int excl_per_struct, int64_t max_newbonds, uint8_t *mask,
                                                                     int32_t *formed, int32_t *broken, uint64_t *adj) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && mask, "tsc_bond_delta: null argument");
    Tables t;
    TSC_TRY(make_tables("tsc_bond_delta", n_structs, n_atoms, atom_class, thr, n_classes, active, ref_bits, excluded, n_excl, excl_per_struct, true,
                        max_newbonds, &t));
    g_kernel_ms = -1.f;
    if (n_structs == 0) return 0;
    DeviceGuard guard(c->device);
    Scratch s(c);
    const size_t N = size_t(n_structs), rows = N * n_atoms * ceil_div(n_atoms, 64);
    double *d_coords;
    int32_t *d_excl = nullptr, *d_formed = nullptr, *d_broken = nullptr;
    uint8_t *d_mask;
    uint64_t *d_adj = nullptr;
    TSC_TRY(upload(c, s, coords, N * n_atoms * 3, &d_coords));
    if (t.a.n_excl) TSC_TRY(upload(c, s, excluded, N * n_excl, &d_excl));
    TSC_TRY(s.get(N, &d_mask));
    if (formed) TSC_TRY(s.get(N, &d_formed));
    if (broken) TSC_TRY(s.get(N, &d_broken));
    if (adj) TSC_TRY(s.get(rows, &d_adj));
    TSC_TRY(run_dev(c, s, t, d_coords, d_excl, d_mask, d_formed, d_broken, d_adj));
    TSC_HIP(hipMemcpyAsync(mask, d_mask, N, hipMemcpyDeviceToHost, c->stream));
    if (formed) TSC_HIP(hipMemcpyAsync(formed, d_formed, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (broken) TSC_HIP(hipMemcpyAsync(broken, d_broken, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (adj) TSC_HIP(hipMemcpyAsync(adj, d_adj, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    return 0;
    TSC_API_GUARD_END
}
