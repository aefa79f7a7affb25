// torsions.hip -- launches and C ABI of the hydrogen-bond finder, the torsion reachability and the torsion grouping kernels
// (torsions.hpp; tscode/torsion_module.py:54-61, :120-132, :233-325, :373-397, :559-606).  gfx950 only.  There is deliberately no CPU implementation behind
// these entry points.
#include "host.hpp"
#include "call.hpp"
#include "torsions.hpp"

#include <vector>

namespace {

using namespace tsc;

// HIP-event times of the kernels of the calling thread's latest tsc_hbonds[_dev] ([0]) and tsc_torsion_reach[_dev] ([1]), taken
// only under the context option "pass_timing" >= 1 (tools/torsion_sets_profile.py); -1 otherwise
thread_local float g_kernel_ms[2] = {-1.f, -1.f};
// ... and of its latest tsc_torsion_groups[_dev] (tsc_torsion_groups_timings; tools/clustered_csearch_profile.py)
thread_local float g_groups_ms = -1.f;

// Largest double x with sqrt(x) <= thresh, so that (thresh < sqrt(d2)) == (d2 > x) for every d2 >= 0: the strict lower bound of
// _get_hydrogen_bonds on squared distances, the counterpart of clash_sq_bound.  A negative threshold lets every distance pass.
double lower_sq_bound(double thresh) {
    if (thresh < 0) return -1.0;
    double x = thresh * thresh;
    while (std::sqrt(x) > thresh) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= thresh) x = std::nextafter(x, INFINITY);
    return x;
}

// Everything that can be refused is refused here, before anything touches the device.
int make_hb_args(const char *who, int64_t n_structs, int n_atoms, const uint8_t *hetero, const uint8_t *hydrogen, const int32_t *extra, int n_extra,
                 bool extra_on_host, double d_min, double d_max, double max_angle, int mode, int max_hb, HbArgs *a) {
    TSC_REQUIRE(hetero && hydrogen, "%s: null argument", who);
    TSC_REQUIRE(n_structs >= 0, "%s: %lld structures", who, (long long)n_structs);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= TOR_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, TOR_MAX_ATOMS);
    TSC_REQUIRE(n_extra >= 0 && n_extra <= TOR_MAX_EXTRA, "%s: %d constraint pairs per structure (0 .. %d)", who, n_extra, TOR_MAX_EXTRA);
    TSC_REQUIRE(n_extra == 0 || extra || n_structs == 0, "%s: %d constraint pairs without an array", who, n_extra);
    TSC_REQUIRE(max_hb >= 0, "%s: %d pair slots per structure", who, max_hb);
    TSC_REQUIRE(mode == TOR_MODE_ALL || mode == TOR_MODE_LINK, "%s: mode %d (0: every hetero pair, 1: pairs that link components)", who, mode);
    TSC_REQUIRE(std::isfinite(d_min) && std::isfinite(d_max) && std::isfinite(max_angle), "%s: a threshold is not finite", who);
    TSC_REQUIRE(d_min < d_max, "%s: d_min %g is not below d_max %g", who, d_min, d_max);
    memset(a, 0, sizeof(*a));
    a->n_structs = n_structs, a->n = n_atoms, a->n_extra = n_extra, a->mode = mode, a->max_hb = max_hb;
    a->lo_sq = lower_sq_bound(d_min), a->hi_sq = clash_sq_bound(d_max), a->max_angle = max_angle;
    for (int i = 0; i < n_atoms; ++i) {
        TSC_REQUIRE(!(hetero[i] && hydrogen[i]), "%s: atom %d is flagged both as a hetero atom and as a hydrogen", who, i);
        if (hetero[i]) a->het[i >> 6] |= 1ull << (i & 63);
        if (hydrogen[i]) a->hyd[i >> 6] |= 1ull << (i & 63);
    }
    if (extra_on_host)
        for (int64_t q = 0; q < n_structs * n_extra * 2; ++q)
            TSC_REQUIRE(extra[q] >= -1 && extra[q] < n_atoms, "%s: constraint atom %d with %d atoms", who, extra[q], n_atoms);
    return 0;
}

template <typename K, typename... Args>
int launch_tor(tsc_ctx *c, K kernel, int64_t work, int wpb, size_t lds, Args... args) {
    TSC_TRY(lds_attribute(kernel, lds));
    hipLaunchKernelGGL(kernel, dim3(grid_for(work, wpb)), dim3(64 * wpb), lds, c->stream, args...);
    return 0;
}

// device pointers throughout
int run_hbonds(tsc_ctx *c, const HbArgs &a, const double *coords, const uint64_t *bonds, const int32_t *extra, int32_t *hb, int32_t *n_hb,
               uint8_t *status, int32_t *n_before, uint64_t *graph) {
    StageTimer tm(c);
    tm.begin();
    int rc = 0;
    with_words(a.n, [&](auto w) {
        constexpr int W = decltype(w)::value, WPB = W <= 4 ? 4 : 1;
        rc = launch_tor(c, k_hbonds<W, WPB>, a.n_structs, WPB, WPB * hbonds_wave_bytes(a.n, W), a, coords, bonds, extra, hb, n_hb, status, n_before,
                        graph);
    });
    TSC_TRY(rc);
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_kernel_ms[0]);
    TSC_HIP(launched);
    return 0;
}

// set_off on the host in both forms: the work items (class, first torsion, torsions) are made from it
int make_items(const char *who, int n_graphs, int n_atoms, const int32_t *set_off, int n_con, const int32_t *constrained, std::vector<int32_t> *items) {
    TSC_REQUIRE(n_graphs >= 0, "%s: %d graphs", who, n_graphs);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= TOR_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, TOR_MAX_ATOMS);
    TSC_REQUIRE(n_con >= 0, "%s: %d constrained slots", who, n_con);
    TSC_REQUIRE(n_con == 0 || constrained, "%s: %d constrained slots without an array", who, n_con);
    TSC_REQUIRE(n_graphs == 0 || set_off, "%s: null argument", who);
    if (n_graphs == 0) return 0;
    TSC_REQUIRE(set_off[0] == 0, "%s: set_off[0] = %d", who, set_off[0]);
    for (int g = 0; g < n_graphs; ++g) {
        TSC_REQUIRE(set_off[g + 1] >= set_off[g], "%s: set_off decreases at class %d", who, g);
        for (int t0 = set_off[g]; t0 < set_off[g + 1]; t0 += TOR_CHUNK) {
            items->push_back(g), items->push_back(t0), items->push_back(std::min(TOR_CHUNK, set_off[g + 1] - t0));
        }
    }
    return 0;
}

int run_reach(tsc_ctx *c, Scratch &s, int n_atoms, const std::vector<int32_t> &items, const uint64_t *graph, const int32_t *torsions,
              const int32_t *constrained, int n_con, uint8_t *flags, uint8_t *masks) {
    int32_t *d_items = nullptr;
    TSC_TRY(upload(c, s, items.data(), items.size(), &d_items));
    const int64_t n_items = int64_t(items.size() / 3);
    StageTimer tm(c);
    tm.begin();
    int rc = 0;
    with_words(n_atoms, [&](auto w) {
        constexpr int W = decltype(w)::value, WPB = W <= 4 ? 4 : 1;
        rc = launch_tor(c, k_torsion_reach<W, WPB>, n_items, WPB, WPB * tor_adj_bytes(W), n_atoms, n_items, (const int32_t *)d_items, graph, torsions,
                        constrained, n_con, flags, masks);
    });
    const hipError_t launched = hipGetLastError();
    if (rc == 0 && launched == hipSuccess) tm.end(&g_kernel_ms[1]);
    // the items were uploaded from this call's own memory: they must have left it before it is freed
    (void)hipStreamSynchronize(c->stream);
    TSC_TRY(rc);
    TSC_HIP(launched);
    return 0;
}

// What both forms of tsc_torsion_groups refuse; *t_max = the most torsions of one structure.
int check_groups(const char *who, int n_structs, int n_atoms, const int32_t *set_off, int max_size, int *t_max) {
    TSC_REQUIRE(n_structs >= 0, "%s: %d structures", who, n_structs);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= TOR_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, TOR_MAX_ATOMS);
    TSC_REQUIRE(max_size >= 1, "%s: max_size = %d", who, max_size);
    TSC_REQUIRE(n_structs == 0 || set_off, "%s: null argument", who);
    *t_max = 0;
    if (n_structs == 0) return 0;
    TSC_REQUIRE(set_off[0] == 0, "%s: set_off[0] = %d", who, set_off[0]);
    for (int s = 0; s < n_structs; ++s) {
        TSC_REQUIRE(set_off[s + 1] >= set_off[s], "%s: set_off decreases at structure %d", who, s);
        const int T = set_off[s + 1] - set_off[s];
        TSC_REQUIRE(T <= GRP_MAX_TORSIONS, "%s: %d torsions in structure %d (at most %d)", who, T, s, GRP_MAX_TORSIONS);
        *t_max = std::max(*t_max, T);
    }
    return 0;
}

// device pointers throughout
int run_groups(tsc_ctx *c, int n_structs, int n_atoms, int t_max, const double *coords, const int32_t *torsions, const int32_t *set_off,
               int max_size, int min_torsions, int32_t *group_of, int32_t *n_groups, int32_t *eps_index, uint8_t *oversize) {
    StageTimer tm(c);
    tm.begin();
    with_width(ceil_div(t_max, 64), [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_torsion_groups<K>, dim3(grid_for(n_structs, 1)), dim3(64), groups_lds_bytes(t_max), c->stream, n_structs, n_atoms,
                           t_max, coords, torsions, set_off, max_size, min_torsions, group_of, n_groups, eps_index, oversize);
    });
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_groups_ms);
    TSC_HIP(launched);
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_torsion_groups_timings(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "tsc_torsion_groups_timings: null argument");
    *ms = g_groups_ms;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsion_groups_dev(tsc_ctx *c, const double *coords, int n_structs, int n_atoms,
                                                                             const int32_t *torsions, const int32_t *set_off, int max_size,
                                                                             int min_torsions, int32_t *group_of, int32_t *n_groups,
                                                                             int32_t *eps_index, uint8_t *oversize) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_torsion_groups_dev: null argument");
    int t_max;
    TSC_TRY(check_groups("tsc_torsion_groups_dev", n_structs, n_atoms, set_off, max_size, &t_max));
    g_groups_ms = -1.f;
    if (n_structs == 0 || set_off[n_structs] == 0) return 0;   // (nothing to read or write: the array pointers may be anything)
    TSC_REQUIRE(coords && torsions && group_of && n_groups && eps_index && oversize, "tsc_torsion_groups_dev: null argument");
    DeviceGuard guard(c->device);
    Scratch s(c);
    int32_t *d_off = nullptr;
    TSC_TRY(upload(c, s, set_off, size_t(n_structs) + 1, &d_off));
    const int rc = run_groups(c, n_structs, n_atoms, t_max, coords, torsions, d_off, max_size, min_torsions, group_of, n_groups, eps_index, oversize);
    // set_off was uploaded from the caller's memory: it must have left it before the call returns
    (void)hipStreamSynchronize(c->stream);
    return rc;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsion_groups(tsc_ctx *c, const double *coords, int n_structs, int n_atoms,
                                                                         const int32_t *torsions, const int32_t *set_off, int max_size,
                                                                         int min_torsions, int32_t *group_of, int32_t *n_groups,
                                                                         int32_t *eps_index, uint8_t *oversize) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_torsion_groups: null argument");
    int t_max;
    TSC_TRY(check_groups("tsc_torsion_groups", n_structs, n_atoms, set_off, max_size, &t_max));
    g_groups_ms = -1.f;
    if (n_structs == 0 || set_off[n_structs] == 0) return 0;   // (nothing to read or write: the array pointers may be anything)
    TSC_REQUIRE(coords && torsions && group_of && n_groups && eps_index && oversize, "tsc_torsion_groups: null argument");
    const size_t S = size_t(n_structs), T = size_t(set_off[n_structs]);
    for (size_t q = 0; q < 4 * T; ++q)
        TSC_REQUIRE(torsions[q] >= 0 && torsions[q] < n_atoms, "tsc_torsion_groups: torsion %zu holds atom %d with %d atoms", q / 4, torsions[q], n_atoms);
    HostCall h(c);
    const double *d_coords;
    const int32_t *d_tors, *d_off;
    int32_t *d_group, *d_ng, *d_eps;
    uint8_t *d_over;
    TSC_TRY(h.in(coords, S * n_atoms * 3, &d_coords));
    TSC_TRY(h.in(torsions, T * 4, &d_tors));
    TSC_TRY(h.in(set_off, S + 1, &d_off));
    TSC_TRY(h.out(group_of, T, &d_group));
    TSC_TRY(h.out(n_groups, S, &d_ng));
    TSC_TRY(h.out(eps_index, S, &d_eps));
    TSC_TRY(h.out(oversize, S, &d_over));
    TSC_TRY(run_groups(c, n_structs, n_atoms, t_max, d_coords, d_tors, d_off, max_size, min_torsions, d_group, d_ng, d_eps, d_over));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsions_timings(tsc_ctx *c, float *ms2) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms2, "tsc_torsions_timings: null argument");
    ms2[0] = g_kernel_ms[0], ms2[1] = g_kernel_ms[1];
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_hbonds_dev(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                     const uint8_t *hetero, const uint8_t *hydrogen, const uint64_t *bonds,
                                                                     const int32_t *extra, int n_extra, double d_min, double d_max,
                                                                     double max_angle, int mode, int max_hb, int32_t *hb, int32_t *n_hb,
                                                                     uint8_t *status, int32_t *n_components_before, uint64_t *graph) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_hbonds_dev: null argument");
    HbArgs a;
    TSC_TRY(make_hb_args("tsc_hbonds_dev", n_structs, n_atoms, hetero, hydrogen, extra, n_extra, false, d_min, d_max, max_angle, mode, max_hb, &a));
    g_kernel_ms[0] = -1.f;
    if (n_structs == 0) return 0;   // (nothing to read or write: the array pointers may be anything)
    TSC_REQUIRE(coords && bonds && n_hb && status && (hb || max_hb <= 0), "tsc_hbonds_dev: null argument");
    DeviceGuard guard(c->device);
    return run_hbonds(c, a, coords, bonds, n_extra ? extra : nullptr, hb, n_hb, status, n_components_before, graph);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_hbonds(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                 const uint8_t *hetero, const uint8_t *hydrogen, const uint64_t *bonds,
                                                                 const int32_t *extra, int n_extra, double d_min, double d_max, double max_angle,
                                                                 int mode, int max_hb, int32_t *hb, int32_t *n_hb, uint8_t *status,
                                                                 int32_t *n_components_before, uint64_t *graph) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_hbonds: null argument");
    HbArgs a;
    TSC_TRY(make_hb_args("tsc_hbonds", n_structs, n_atoms, hetero, hydrogen, extra, n_extra, true, d_min, d_max, max_angle, mode, max_hb, &a));
    g_kernel_ms[0] = -1.f;
    if (n_structs == 0) return 0;   // (nothing to read or write: the array pointers may be anything)
    TSC_REQUIRE(coords && bonds && n_hb && status && (hb || max_hb <= 0), "tsc_hbonds: null argument");
    HostCall h(c);
    const size_t N = size_t(n_structs), W = size_t(ceil_div(n_atoms, 64));
    const double *d_coords;
    const uint64_t *d_bonds;
    const int32_t *d_extra = nullptr;
    int32_t *d_hb, *d_nhb, *d_before;
    uint8_t *d_status;
    uint64_t *d_graph;
    TSC_TRY(h.in(coords, N * n_atoms * 3, &d_coords));
    TSC_TRY(h.in(bonds, N * n_atoms * W, &d_bonds));
    if (n_extra) TSC_TRY(h.in(extra, N * n_extra * 2, &d_extra));
    TSC_TRY(h.out(max_hb > 0 ? hb : nullptr, N * max_hb * 2, &d_hb));
    // (the kernel writes a structure's pairs only: the slots behind them come back as -1)
    if (d_hb) TSC_HIP(hipMemsetAsync(d_hb, 0xff, N * max_hb * 2 * sizeof(int32_t), c->stream));
    TSC_TRY(h.out(n_hb, N, &d_nhb));
    TSC_TRY(h.out(status, N, &d_status));
    TSC_TRY(h.out(n_components_before, N, &d_before));
    TSC_TRY(h.out(graph, N * n_atoms * W, &d_graph));
    TSC_TRY(run_hbonds(c, a, d_coords, d_bonds, d_extra, d_hb, d_nhb, d_status, d_before, d_graph));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsion_reach_dev(tsc_ctx *c, const uint64_t *graph, int n_graphs, int n_atoms,
                                                                            const int32_t *torsions, const int32_t *set_off,
                                                                            const int32_t *constrained, int n_con, uint8_t *flags,
                                                                            uint8_t *masks) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_torsion_reach_dev: null argument");
    std::vector<int32_t> items;
    TSC_TRY(make_items("tsc_torsion_reach_dev", n_graphs, n_atoms, set_off, n_con, constrained, &items));
    g_kernel_ms[1] = -1.f;
    if (items.empty()) return 0;
    TSC_REQUIRE(graph && torsions && flags && masks, "tsc_torsion_reach_dev: null argument");
    DeviceGuard guard(c->device);
    Scratch s(c);
    return run_reach(c, s, n_atoms, items, graph, torsions, n_con ? constrained : nullptr, n_con, flags, masks);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsion_reach(tsc_ctx *c, const uint64_t *graph, int n_graphs, int n_atoms,
                                                                        const int32_t *torsions, const int32_t *set_off,
                                                                        const int32_t *constrained, int n_con, uint8_t *flags, uint8_t *masks) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_torsion_reach: null argument");
    std::vector<int32_t> items;
    TSC_TRY(make_items("tsc_torsion_reach", n_graphs, n_atoms, set_off, n_con, constrained, &items));
    g_kernel_ms[1] = -1.f;
    if (items.empty()) return 0;
    TSC_REQUIRE(graph && torsions && flags && masks, "tsc_torsion_reach: null argument");
    const size_t G = size_t(n_graphs), T = size_t(set_off[n_graphs]), W = size_t(ceil_div(n_atoms, 64));
    for (size_t t = 0; t < T; ++t) {
        for (int k = 0; k < 4; ++k)
            TSC_REQUIRE(torsions[4 * t + k] >= 0 && torsions[4 * t + k] < n_atoms, "tsc_torsion_reach: torsion %zu holds atom %d with %d atoms", t,
                        torsions[4 * t + k], n_atoms);
        TSC_REQUIRE(torsions[4 * t + 1] != torsions[4 * t + 2], "tsc_torsion_reach: torsion %zu has no central bond (i2 == i3)", t);
    }
    for (size_t q = 0; q < G * n_con; ++q)
        TSC_REQUIRE(constrained[q] >= -1 && constrained[q] < n_atoms, "tsc_torsion_reach: constrained atom %d with %d atoms", constrained[q], n_atoms);
    HostCall h(c);
    const uint64_t *d_graph;
    const int32_t *d_tors, *d_con = nullptr;
    uint8_t *d_flags, *d_masks;
    TSC_TRY(h.in(graph, G * n_atoms * W, &d_graph));
    TSC_TRY(h.in(torsions, T * 4, &d_tors));
    if (n_con) TSC_TRY(h.in(constrained, G * n_con, &d_con));
    TSC_TRY(h.out(flags, T, &d_flags));
    TSC_TRY(h.out(masks, T * n_atoms, &d_masks));
    TSC_TRY(run_reach(c, h.scratch(), n_atoms, items, d_graph, d_tors, d_con, n_con, d_flags, d_masks));
    return h.finish();
    TSC_API_GUARD_END
}
