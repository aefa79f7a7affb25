// prune_team.hip -- launch and C ABI of the team route of the batched prune_conformers_rmsd (prune_team.hpp; tscode/rmsd_pruning.py:43-206,
// one run of :164-206 per segment).  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "pass_plan.hpp"
#include "prune_team.hpp"

#include <algorithm>
#include <vector>

namespace {

using namespace tsc;

constexpr int PT_KS[TSC_MAX_PASSES] = {500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1};  // :186-188

struct TeamPlan {
    std::vector<PtSegment> segs;  // the caller's order
    std::vector<int2> items;      // (segment, row tile), the long column ranges first
    std::vector<int> slots;       // the k some segment can take by its N alone
    int64_t total_structs = 0, total_doubles = 0, total_words = 0;
};

// Everything that can be refused is refused here, before anything touches the device.
int make_plan(const char *who, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments, int mode, TeamPlan *out) {
    TSC_REQUIRE(n_segments >= 0 && n_segments <= INT_MAX / TSC_MAX_PASSES, "%s: %lld segments", who, (long long)n_segments);
    TSC_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 = reference-exact, 1 = cache-free)", who, mode);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(offsets && n && h && thr, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    out->segs.resize(size_t(n_segments));
    int64_t moff = 0, woff = 0;
    int n_max = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        TSC_REQUIRE(h[s] >= 1, "%s: segment %lld has %d heavy atoms (at least 1)", who, (long long)s, h[s]);
        TSC_REQUIRE(n[s] >= 0, "%s: segment %lld has %d structures", who, (long long)s, n[s]);
        TSC_REQUIRE(n[s] <= PT_MAX_N, "%s: segment %lld has %d structures, more than TSC_PRUNE_TEAM_MAX_N = %d", who, (long long)s, n[s], PT_MAX_N);
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == int64_t(n[s]) * h[s] * 3, "%s: offsets[%lld] .. offsets[%lld] span %lld doubles, segment is %d x %d x 3", who,
                    (long long)s, (long long)s + 1, (long long)(offsets[s + 1] - offsets[s]), n[s], h[s]);
        TSC_REQUIRE(std::isfinite(thr[s]), "%s: thr[%lld] is not finite", who, (long long)s);
        const Thresholds t = thresholds(h[s], thr[s]);
        PtSegment &g = out->segs[size_t(s)];
        g.off = offsets[s], g.moff = moff, g.woff = woff, g.n = n[s], g.h = h[s];
        g.thr = t.thr, g.maxdev_thr = t.maxdev_thr, g.half_h_thr2 = t.half_h_thr2, g.two_thr2 = t.two_thr2;
        moff += n[s], woff += ceil_div(n[s], 64);
        n_max = std::max(n_max, n[s]);
    }
    TSC_REQUIRE(woff * PT_PER_WORD <= INT_MAX, "%s: %lld work items in all", who, (long long)(woff * PT_PER_WORD));
    out->total_structs = moff, out->total_doubles = offsets[n_segments], out->total_words = woff;
    out->items.reserve(size_t(woff * PT_PER_WORD));
    for (int64_t s = 0; s < n_segments; ++s)
        for (int t = 0; t < ceil_div(n[s], PT_ROWS); ++t) out->items.push_back(make_int2(int(s), t));
    // the items whose rows can have the longest walks start first: a tile in front of many columns started last would be the launch's
    // tail.  The order changes no result: the items of a launch share only counters.
    std::stable_sort(out->items.begin(), out->items.end(), [&](const int2 &a, const int2 &b) {
        return int64_t(n[a.x] - PT_ROWS * a.y) * h[a.x] > int64_t(n[b.x] - PT_ROWS * b.y) * h[b.x];
    });
    for (int ks = 0; ks < TSC_MAX_PASSES; ++ks)
        if (n_max > 0 && (PT_KS[ks] == 1 || 20ll * PT_KS[ks] < n_max)) out->slots.push_back(PT_KS[ks]);  // :192 with nothing removed yet
    return 0;
}

// device pointers throughout; nothing here waits for the stream
int run_dev(tsc_ctx *c, Scratch &s, const TeamPlan &plan, const PtSegment *d_segs, const int2 *d_items, int mode, const double *heavy, uint8_t *mask,
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

}  // namespace

// prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on n_segments heavy-atom arrays at once; everything but the tables on the device.
extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_team_dev(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n,
                                                                              const int32_t *h, const double *thr, int64_t n_segments, int mode,
                                                                              uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes,
                                                                              uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_prune_rmsd_team_dev: null argument");
    TeamPlan plan;
    TSC_TRY(make_plan("tsc_prune_rmsd_team_dev", offsets, n, h, thr, n_segments, mode, &plan));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || plan.total_doubles == 0) && (mask || plan.total_structs == 0), "tsc_prune_rmsd_team_dev: null argument");
    DeviceGuard guard(c->device);
    Scratch s(c);
    PtSegment *d_segs;
    int2 *d_items;
    TSC_TRY(s.get(plan.segs.size(), &d_segs));
    TSC_TRY(s.get(std::max<size_t>(plan.items.size(), 1), &d_items));
    // the tables are uploaded from this call's own memory: they must have left it before it is freed, whatever happens after
    hipError_t copied = hipMemcpyAsync(d_segs, plan.segs.data(), plan.segs.size() * sizeof(PtSegment), hipMemcpyHostToDevice, c->stream);
    if (copied == hipSuccess && !plan.items.empty())
        copied = hipMemcpyAsync(d_items, plan.items.data(), plan.items.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    const int rc = copied == hipSuccess ? run_dev(c, s, plan, d_segs, d_items, mode, heavy, mask, stats, n_passes, nonfinite) : 0;
    const hipError_t waited = hipStreamSynchronize(c->stream);
    TSC_HIP(copied);
    TSC_TRY(rc);
    TSC_HIP(waited);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_team(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n,
                                                                          const int32_t *h, const double *thr, int64_t n_segments, int mode, uint8_t *mask,
                                                                          tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_prune_rmsd_team: null argument");
    TeamPlan plan;  // (in front of the HostCall: it outlives the call's wait for the stream)
    TSC_TRY(make_plan("tsc_prune_rmsd_team", offsets, n, h, thr, n_segments, mode, &plan));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || plan.total_doubles == 0) && (mask || plan.total_structs == 0), "tsc_prune_rmsd_team: null argument");
    HostCall call(c);
    const size_t S = size_t(n_segments);
    double *d_heavy;
    uint8_t *d_mask, *d_nonfinite;
    tsc_batch_pass_stats *d_stats;
    int32_t *d_np;
    const PtSegment *d_segs;
    const int2 *d_items;
    TSC_TRY(call.in(plan.segs.data(), S, &d_segs));
    TSC_TRY(call.in(plan.items.data(), plan.items.size(), &d_items));
    TSC_TRY(call.in(heavy, size_t(plan.total_doubles), &d_heavy));
    TSC_TRY(call.out(mask, size_t(plan.total_structs), &d_mask));
    if (!d_mask) TSC_TRY(call.scratch().get(1, &d_mask));  // (no structures at all)
    TSC_TRY(call.out(stats, S * TSC_MAX_PASSES, &d_stats));
    TSC_TRY(call.out(n_passes, S, &d_np));
    TSC_TRY(call.out(nonfinite, S, &d_nonfinite));
    TSC_TRY(run_dev(c, call.scratch(), plan, d_segs, d_items, mode, d_heavy, d_mask, d_stats, d_np, d_nonfinite));
    return call.finish();
    TSC_API_GUARD_END
}
