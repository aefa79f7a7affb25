// prune_batch.hip -- launch and C ABI of the batched prune_conformers_rmsd (prune_batch.hpp; tscode/rmsd_pruning.py:43-206, one run of
// :164-206 per segment).  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "pass_plan.hpp"
#include "prune_batch.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

namespace {

using namespace tsc;

// Everything that can be refused is refused here, before anything touches the device.  The table comes out in launch order:
// decreasing n^2 h, the long segments first (ties in the caller's order) -- a workgroup's time grows with that product, and the
// longest one started last would be the launch's tail.  The order changes no result: the workgroups share nothing.
int make_segments(const char *who, const tsc_ctx *c, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr, int64_t n_segments,
                  int mode, std::vector<PbSegment> *out, int64_t *total_structs, int64_t *total_doubles) {
    TSC_REQUIRE(n_segments >= 0 && n_segments <= INT_MAX / TSC_MAX_PASSES, "%s: %lld segments", who, (long long)n_segments);
    TSC_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 = reference-exact, 1 = cache-free)", who, mode);
    *total_structs = *total_doubles = 0;
    if (n_segments == 0) return 0;
    TSC_REQUIRE(offsets && n && h && thr, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    out->resize(size_t(n_segments));
    int64_t moff = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        TSC_REQUIRE(h[s] >= 1, "%s: segment %lld has %d heavy atoms (at least 1)", who, (long long)s, h[s]);
        TSC_REQUIRE(n[s] >= 0, "%s: segment %lld has %d structures", who, (long long)s, n[s]);
        TSC_REQUIRE(n[s] <= c->opt.prune_batch_max_n, "%s: segment %lld has %d structures, more than \"prune_batch_max_n\" = %d", who, (long long)s, n[s],
                    c->opt.prune_batch_max_n);
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == int64_t(n[s]) * h[s] * 3, "%s: offsets[%lld] .. offsets[%lld] span %lld doubles, segment is %d x %d x 3", who,
                    (long long)s, (long long)s + 1, (long long)(offsets[s + 1] - offsets[s]), n[s], h[s]);
        TSC_REQUIRE(std::isfinite(thr[s]), "%s: thr[%lld] is not finite", who, (long long)s);
        const Thresholds t = thresholds(h[s], thr[s]);
        PbSegment &g = (*out)[size_t(s)];
        g.off = offsets[s], g.moff = moff, g.n = n[s], g.h = h[s], g.seg = int(s), g.pad = 0;
        g.thr = t.thr, g.maxdev_thr = t.maxdev_thr, g.half_h_thr2 = t.half_h_thr2, g.two_thr2 = t.two_thr2;
        moff += n[s];
    }
    *total_structs = moff, *total_doubles = offsets[n_segments];
    std::stable_sort(out->begin(), out->end(), [](const PbSegment &a, const PbSegment &b) {
        return double(a.n) * double(a.n) * double(a.h) > double(b.n) * double(b.n) * double(b.h);
    });
    return 0;
}

// device pointers throughout
int run_dev(tsc_ctx *c, Scratch &s, const PbSegment *d_segs, size_t n_segs, int64_t total_structs, int mode, const double *heavy, uint8_t *mask,
            tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    double *d_G;
    int2 *d_keys;
    TSC_TRY(s.get(size_t(std::max<int64_t>(total_structs, 1)), &d_G));
    TSC_TRY(s.get(size_t(std::max<int64_t>(total_structs, 1)), &d_keys));
    if (stats) TSC_HIP(hipMemsetAsync(stats, 0, n_segs * TSC_MAX_PASSES * sizeof(tsc_batch_pass_stats), c->stream));
    hipLaunchKernelGGL(k_prune_batch, dim3(unsigned(n_segs)), dim3(PB_THREADS), 0, c->stream, d_segs, heavy, mode == 0 ? 1 : 0, d_G,
                       d_keys, mask, stats, n_passes, nonfinite);
    TSC_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on n_segments heavy-atom arrays at once; everything but the tables on the device.
extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_batch_dev(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n,
                                                                               const int32_t *h, const double *thr, int64_t n_segments, int mode,
                                                                               uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes,
                                                                               uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_prune_rmsd_batch_dev: null argument");
    std::vector<PbSegment> segs;
    int64_t total_structs, total_doubles;
    TSC_TRY(make_segments("tsc_prune_rmsd_batch_dev", c, offsets, n, h, thr, n_segments, mode, &segs, &total_structs, &total_doubles));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || total_doubles == 0) && (mask || total_structs == 0), "tsc_prune_rmsd_batch_dev: null argument");
    DeviceGuard guard(c->device);
    Scratch s(c);
    PbSegment *d_segs;
    TSC_TRY(s.get(segs.size(), &d_segs));
    // the table is uploaded from this call's own memory: it must have left it before it is freed, whatever happens after
    const hipError_t copied = hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(PbSegment), hipMemcpyHostToDevice, c->stream);
    const int rc = copied == hipSuccess ? run_dev(c, s, d_segs, segs.size(), total_structs, mode, heavy, mask, stats, n_passes, nonfinite) : 0;
    const hipError_t waited = hipStreamSynchronize(c->stream);
    TSC_HIP(copied);
    TSC_TRY(rc);
    TSC_HIP(waited);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_batch(tsc_ctx *c, const double *heavy, const int64_t *offsets, const int32_t *n,
                                                                           const int32_t *h, const double *thr, int64_t n_segments, int mode, uint8_t *mask,
                                                                           tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c, "tsc_prune_rmsd_batch: null argument");
    std::vector<PbSegment> segs;  // (in front of the HostCall: it outlives the call's wait for the stream)
    int64_t total_structs, total_doubles;
    TSC_TRY(make_segments("tsc_prune_rmsd_batch", c, offsets, n, h, thr, n_segments, mode, &segs, &total_structs, &total_doubles));
    if (n_segments == 0) return 0;
    TSC_REQUIRE((heavy || total_doubles == 0) && (mask || total_structs == 0), "tsc_prune_rmsd_batch: null argument");
    HostCall call(c);
    const size_t S = size_t(n_segments);
    double *d_heavy;
    uint8_t *d_mask, *d_nonfinite;
    tsc_batch_pass_stats *d_stats;
    int32_t *d_np;
    const PbSegment *d_segs;
    TSC_TRY(call.in(segs.data(), S, &d_segs));
    TSC_TRY(call.in(heavy, size_t(total_doubles), &d_heavy));
    TSC_TRY(call.out(mask, size_t(total_structs), &d_mask));
    if (!d_mask) TSC_TRY(call.scratch().get(1, &d_mask));  // (no structures at all)
    TSC_TRY(call.out(stats, S * TSC_MAX_PASSES, &d_stats));
    TSC_TRY(call.out(n_passes, S, &d_np));
    TSC_TRY(call.out(nonfinite, S, &d_nonfinite));
    TSC_TRY(run_dev(c, call.scratch(), d_segs, S, total_structs, mode, d_heavy, d_mask, d_stats, d_np, d_nonfinite));
    return call.finish();
    TSC_API_GUARD_END
}
