// topology.hip -- launches and C ABI of the batched bond-graph / scramble check (topology.hpp; tscode/graph_manipulations.py:28-55,
// tscode/utils.py:293-314, :341-387).  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
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
    TSC_TRY(check_class_table(who, atom_class, n_atoms, thr, n_classes, a.bound, T));  // (a bound of 0: never bonded)
    for (int i = 0; i < n_atoms; ++i) a.cls[i] = (!active || active[i]) ? atom_class[i] : uint8_t(n_classes);
    TSC_TRY(check_index_list(who, "excluded", excluded, n_excl, excl_per_struct, excluded_on_host, n_structs, n_atoms, a.excl_words, &a.n_excl));
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

// device pointers throughout, except the tables
int run_dev(tsc_ctx *c, Scratch &s, const Tables &t, const double *coords, const int32_t *excl_dev, uint8_t *mask, int32_t *formed,
            int32_t *broken, uint64_t *adj) {
    const TopoArgs &a = t.a;
    uint64_t *d_ref = nullptr;
    if (!t.ref.empty()) TSC_TRY(upload(c, s, t.ref.data(), t.ref.size(), &d_ref));
    StageTimer tm(c);
    tm.begin();
    with_words(a.n, [&](auto w) {
        hipLaunchKernelGGL(k_bond_delta<decltype(w)::value>, dim3(grid_for(a.n_structs, 4)), dim3(256), topo_lds_bytes(a.n), c->stream, a, coords, d_ref, excl_dev,
                           mask, formed, broken, adj);
    });
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_kernel_ms);
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
    HostCall h(c);
    const size_t N = size_t(n_structs);
    double *d_coords;
    int32_t *d_excl = nullptr, *d_formed, *d_broken;
    uint8_t *d_mask;
    uint64_t *d_adj;
    TSC_TRY(h.in(coords, N * n_atoms * 3, &d_coords));
    if (t.a.n_excl) TSC_TRY(h.in(excluded, N * n_excl, &d_excl));
    TSC_TRY(h.out(mask, N, &d_mask));
    TSC_TRY(h.out(formed, N, &d_formed));
    TSC_TRY(h.out(broken, N, &d_broken));
    TSC_TRY(h.out(adj, N * n_atoms * ceil_div(n_atoms, 64), &d_adj));
    TSC_TRY(run_dev(c, h.scratch(), t, d_coords, d_excl, d_mask, d_formed, d_broken, d_adj));
    return h.finish();
    TSC_API_GUARD_END
}
