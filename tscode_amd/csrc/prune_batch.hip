// prune_batch.hip -- launch and C ABI of the batched prune_conformers_rmsd (tscode/rmsd_pruning.py:43-206, one run of :164-206 per segment),
// both routes: a workgroup per segment (prune_batch.hpp) and a team of workgroups per segment (prune_team.hpp).  Their tables come from
// prune_batch_plan.hpp.  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "prune_team.hpp"

namespace {

using namespace tsc;

// A route: its tables (every refusal is past before anything touches the device), and its launches, on device pointers throughout,
// which wait for nothing.
struct BatchRoute {
    int (*plan)(const char *who, const tsc_ctx *c, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments,
                int mode, PbPlan *out);
    int (*launch)(tsc_ctx *c, Scratch &s, const PbPlan &plan, const PbSegment *d_segs, const int2 *d_items, int mode, const double *heavy, uint8_t *mask,
                  tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite);
};

int plan_batch(const char *who, const tsc_ctx *c, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments, int mode,
               PbPlan *out) {
    TSC_TRY(segments(who, offsets, n, h, thr, n_segments, mode, c->opt.prune_batch_max_n, "\"prune_batch_max_n\"", out));
    launch_order(out);
    return 0;
}

int launch_batch(tsc_ctx *c, Scratch &s, const PbPlan &plan, const PbSegment *d_segs, const int2 *, int mode, const double *heavy, uint8_t *mask,
                 tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    const size_t S = plan.segs.size(), T = size_t(std::max<int64_t>(plan.total_structs, 1));
    double *d_G;
    int2 *d_keys;
    TSC_TRY(s.get(T, &d_G));
    TSC_TRY(s.get(T, &d_keys));
    if (stats) TSC_HIP(hipMemsetAsync(stats, 0, S * TSC_MAX_PASSES * sizeof(tsc_batch_pass_stats), c->stream));
    hipLaunchKernelGGL(k_prune_batch, dim3(unsigned(S)), dim3(PB_THREADS), 0, c->stream, d_segs, heavy, mode == 0 ? 1 : 0, d_G, d_keys, mask, stats, n_passes,
                       nonfinite);
    TSC_HIP(hipGetLastError());
    return 0;
}

int plan_team(const char *who, const tsc_ctx *, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments, int mode,
              PbPlan *out) {
    TSC_TRY(segments(who, offsets, n, h, thr, n_segments, mode, PT_MAX_N, "TSC_PRUNE_TEAM_MAX_N", out));
    return team_tables(who, out);
}

int launch_team(tsc_ctx *c, Scratch &s, const PbPlan &plan, const PbSegment *d_segs, const int2 *d_items, int mode, const double *heavy, uint8_t *mask,
                tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    const size_t S = plan.segs.size(), W = size_t(std::max<int64_t>(plan.total_words, 1)), T = size_t(std::max<int64_t>(plan.total_structs, 1));
    const unsigned n_items = unsigned(plan.items.size());
    PtState st;
    TSC_TRY(s.get(W, &st.in));
    TSC_TRY(s.get(W, &st.out));
    TSC_TRY(s.get(W, &st.view));
    TSC_TRY(s.get(T, &st.G));
    TSC_TRY(s.get(T, &st.keys));
    TSC_TRY(s.get(S, &st.rec));
    if (stats) TSC_HIP(hipMemsetAsync(stats, 0, S * TSC_MAX_PASSES * sizeof(tsc_batch_pass_stats), c->stream));
    hipLaunchKernelGGL(k_team_init, dim3(unsigned(ceil_div<size_t>(S, PT_THREADS))), dim3(PT_THREADS), 0, c->stream, st, d_segs, int(S));
    if (n_items) hipLaunchKernelGGL(k_team_prologue, dim3(n_items), dim3(PT_ROWS), 0, c->stream, st, d_segs, d_items, heavy);
    for (int k : plan.slots) {
        hipLaunchKernelGGL(k_team_turn, dim3(unsigned(S)), dim3(PT_THREADS), 0, c->stream, st, d_segs, k, mode == 0 ? 1 : 0, stats, n_passes, nonfinite);
        hipLaunchKernelGGL(k_team_rows, dim3(n_items), dim3(PT_THREADS), 0, c->stream, st, d_segs, d_items, heavy);
    }
    hipLaunchKernelGGL(k_team_turn, dim3(unsigned(S)), dim3(PT_THREADS), 0, c->stream, st, d_segs, 0, 0, stats, n_passes, nonfinite);
    if (n_items) hipLaunchKernelGGL(k_team_finish, dim3(n_items), dim3(PT_ROWS), 0, c->stream, st, d_segs, d_items, mask);
    TSC_HIP(hipGetLastError());
    return 0;
}

constexpr BatchRoute ROUTE_BATCH{plan_batch, launch_batch}, ROUTE_TEAM{plan_team, launch_team};

// prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on n_segments heavy-atom arrays at once; everything but the tables on the device.
int prune_batch_dev(const char *who, const BatchRoute &route, tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                    const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    TSC_REQUIRE(c, "%s: null argument", who);
    PbPlan plan;
    TSC_TRY(route.plan(who, c, offsets, n, h, thr, n_segments, mode, &plan));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || plan.total_doubles == 0) && (mask || plan.total_structs == 0), "%s: null argument", who);
    DeviceGuard guard(c->device);
    Scratch s(c);
    PbSegment *d_segs;
    int2 *d_items = nullptr;
    TSC_TRY(s.get(plan.segs.size(), &d_segs));
    if (!plan.items.empty()) TSC_TRY(s.get(plan.items.size(), &d_items));
    // the tables are uploaded from this call's own memory: they must have left it before it is freed, whatever happens after
    hipError_t copied = hipMemcpyAsync(d_segs, plan.segs.data(), plan.segs.size() * sizeof(PbSegment), hipMemcpyHostToDevice, c->stream);
    if (copied == hipSuccess && d_items) copied = hipMemcpyAsync(d_items, plan.items.data(), plan.items.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    const int rc = copied == hipSuccess ? route.launch(c, s, plan, d_segs, d_items, mode, heavy, mask, stats, n_passes, nonfinite) : 0;
    const hipError_t waited = hipStreamSynchronize(c->stream);
    TSC_HIP(copied);
    TSC_TRY(rc);
    TSC_HIP(waited);
    return 0;
}

// ... the same on host arrays
int prune_batch_host(const char *who, const BatchRoute &route, tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                     const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    TSC_REQUIRE(c, "%s: null argument", who);
    PbPlan plan;  // (in front of the HostCall: it outlives the call's wait for the stream)
    TSC_TRY(route.plan(who, c, offsets, n, h, thr, n_segments, mode, &plan));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || plan.total_doubles == 0) && (mask || plan.total_structs == 0), "%s: null argument", who);
    HostCall call(c);
    const size_t S = size_t(n_segments);
    double *d_heavy;
    uint8_t *d_mask, *d_nonfinite;
    tsc_batch_pass_stats *d_stats;
    int32_t *d_np;
    const PbSegment *d_segs;
    const int2 *d_items = nullptr;
    TSC_TRY(call.in(plan.segs.data(), S, &d_segs));
    if (!plan.items.empty()) TSC_TRY(call.in(plan.items.data(), plan.items.size(), &d_items));
    TSC_TRY(call.in(heavy, size_t(plan.total_doubles), &d_heavy));
    TSC_TRY(call.out(mask, size_t(plan.total_structs), &d_mask));
    if (!d_mask) TSC_TRY(call.scratch().get(1, &d_mask));  // (no structures at all)
    TSC_TRY(call.out(stats, S * TSC_MAX_PASSES, &d_stats));
    TSC_TRY(call.out(n_passes, S, &d_np));
    TSC_TRY(call.out(nonfinite, S, &d_nonfinite));
    TSC_TRY(route.launch(c, call.scratch(), plan, d_segs, d_items, mode, d_heavy, d_mask, d_stats, d_np, d_nonfinite));
    return call.finish();
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_batch(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                                                                           const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                                                                           int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    return prune_batch_host("tsc_prune_rmsd_batch", ROUTE_BATCH, c, heavy, offsets, n, h, thr, n_segments, mode, mask, stats, n_passes, nonfinite);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_batch_dev(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                                                                               const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                                                                               int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    return prune_batch_dev("tsc_prune_rmsd_batch_dev", ROUTE_BATCH, c, heavy, offsets, n, h, thr, n_segments, mode, mask, stats, n_passes, nonfinite);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_team(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                                                                          const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                                                                          int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    return prune_batch_host("tsc_prune_rmsd_team", ROUTE_TEAM, c, heavy, offsets, n, h, thr, n_segments, mode, mask, stats, n_passes, nonfinite);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_team_dev(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h,
                                                                              const double *thr, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                                                                              int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    return prune_batch_dev("tsc_prune_rmsd_team_dev", ROUTE_TEAM, c, heavy, offsets, n, h, thr, n_segments, mode, mask, stats, n_passes, nonfinite);
    TSC_API_GUARD_END
}
