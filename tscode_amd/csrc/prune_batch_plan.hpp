// prune_batch_plan.hpp -- what a many-ensembles RMSD prune (prune_batch.hip) hands its kernels, as tables: the segments with their offsets
// and thresholds, the launch order of the one-workgroup route (prune_batch.hpp), the work items and the schedule slots of the team route
// (prune_team.hpp).  Plain functions that make no HIP call, and every refusal of an argument list: tools/probe/prune_batch_plan_check.cpp
// runs them on the CPU at sizes worked out by hand.
#pragma once

#include <algorithm>
#include <vector>

#include "pass_plan.hpp"
#include "prune_schedule.hpp"

namespace tsc {

constexpr int PT_ROWS = 16;                // rows of a work item of the team route: four per wavefront.  A lone ensemble of 4096 structures makes
                                           // 256 items of them, 1024 wavefronts; with 64 rows it was one wavefront per compute unit
constexpr int PT_PER_WORD = 64 / PT_ROWS;  // items that share a word of the segment's bit arrays
static_assert(PT_ROWS * PT_PER_WORD == 64 && PT_ROWS <= 64, "the rows of an item lie in one mask word");

struct PbSegment {   // one per segment
    long long off;   // first double of the segment's [n, h, 3] block in `heavy`
    long long moff;  // first structure of the segment in the batch (mask, squared norms, key list)
    int n, h;
    int seg;         // the segment's index in the caller's arrays (stats, n_passes, nonfinite)
    double thr, maxdev_thr, half_h_thr2, two_thr2;  // pass_plan.hpp: thresholds()
    long long woff;  // first 64-bit word of the segment in the team route's bit arrays: each segment starts on a word of its own.  (Last: the
                     // one-workgroup kernel reads the fields in front of it where it always did -- MEASURED.md section 31)
};

struct PbPlan {
    std::vector<PbSegment> segs;  // the caller's order (segments); the launch order after launch_order()
    std::vector<int2> items;      // team_tables: (segment, tile of PT_ROWS rows), the long column ranges first
    std::vector<int> slots;       // team_tables: the k some segment can take by its N alone
    int64_t total_structs = 0, total_doubles = 0, total_words = 0;
};

// 64 bits of a segment's bit array of nw words from bit t on (words at nw and beyond read as zero)
__host__ __device__ inline unsigned long long pt_bits(const unsigned long long *__restrict__ bits, int nw, int t) {
    const int w = t >> 6, s = t & 63;
    unsigned long long v = w < nw ? bits[w] >> s : 0ull;
    if (s && w + 1 < nw) v |= bits[w + 1] << (64 - s);
    return v;
}

// Everything that can be refused is refused here, before anything touches the device.  max_n / max_n_name: the structures a segment of
// the route may have, and what the message calls that cap.
inline int segments(const char *who, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments, int mode, int max_n,
                    const char *max_n_name, PbPlan *out) {
    TSC_REQUIRE(n_segments >= 0 && n_segments <= INT_MAX / TSC_MAX_PASSES, "%s: %lld segments", who, (long long)n_segments);
    TSC_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 = reference-exact, 1 = cache-free)", who, mode);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(offsets && n && h && thr, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    out->segs.resize(size_t(n_segments));
    int64_t moff = 0, woff = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        TSC_REQUIRE(h[s] >= 1, "%s: segment %lld has %d heavy atoms (at least 1)", who, (long long)s, h[s]);
        TSC_REQUIRE(n[s] >= 0, "%s: segment %lld has %d structures", who, (long long)s, n[s]);
        TSC_REQUIRE(n[s] <= max_n, "%s: segment %lld has %d structures, more than %s = %d", who, (long long)s, n[s], max_n_name, max_n);
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == int64_t(n[s]) * h[s] * 3, "%s: offsets[%lld] .. offsets[%lld] span %lld doubles, segment is %d x %d x 3", who,
                    (long long)s, (long long)s + 1, (long long)(offsets[s + 1] - offsets[s]), n[s], h[s]);
        TSC_REQUIRE(std::isfinite(thr[s]), "%s: thr[%lld] is not finite", who, (long long)s);
        const Thresholds t = thresholds(h[s], thr[s]);
        PbSegment &g = out->segs[size_t(s)];
        g.off = offsets[s], g.moff = moff, g.woff = woff, g.n = n[s], g.h = h[s], g.seg = int(s);
        g.thr = t.thr, g.maxdev_thr = t.maxdev_thr, g.half_h_thr2 = t.half_h_thr2, g.two_thr2 = t.two_thr2;
        moff += n[s], woff += ceil_div(n[s], 64);
    }
    out->total_structs = moff, out->total_doubles = offsets[n_segments], out->total_words = woff;
    return 0;
}

// The one-workgroup route launches in decreasing n^2 h, the long segments first (ties in the caller's order) -- a workgroup's time grows
// with that product, and the longest one started last would be the launch's tail.  The order changes no result: the workgroups share nothing.
inline void launch_order(PbPlan *p) {
    std::stable_sort(p->segs.begin(), p->segs.end(), [](const PbSegment &a, const PbSegment &b) {
        return double(a.n) * double(a.n) * double(a.h) > double(b.n) * double(b.n) * double(b.h);
    });
}

// The team route's work items and schedule slots, from segments in the caller's order.
inline int team_tables(const char *who, PbPlan *p) {
    TSC_REQUIRE(p->total_words * PT_PER_WORD <= INT_MAX, "%s: %lld work items in all", who, (long long)(p->total_words * PT_PER_WORD));
    const std::vector<PbSegment> &g = p->segs;
    int n_max = 0;
    p->items.reserve(size_t(p->total_words * PT_PER_WORD));
    for (size_t s = 0; s < g.size(); ++s) {
        for (int t = 0; t < ceil_div(g[s].n, PT_ROWS); ++t) p->items.push_back(make_int2(int(s), t));
        n_max = std::max(n_max, g[s].n);
    }
    // the items whose rows can have the longest walks start first: a tile in front of many columns started last would be the launch's
    // tail.  The order changes no result: the items of a launch share only counters.
    std::stable_sort(p->items.begin(), p->items.end(), [&](const int2 &a, const int2 &b) {
        return int64_t(g[a.x].n - PT_ROWS * a.y) * g[a.x].h > int64_t(g[b.x].n - PT_ROWS * b.y) * g[b.x].h;
    });
    for (int k : KS)
        if (n_max > 0 && pass_gate(k, n_max)) p->slots.push_back(k);  // :192 with nothing removed yet
    return 0;
}

}  // namespace tsc
