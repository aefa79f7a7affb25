// refine_batch.hip -- launches and C ABI of the two similarity stages of Embedder.similarity_refining (tscode/embedder.py:1310-1388) that
// take many ensembles per call beside the TFD and RMSD batches: the symmetry-corrected RMSD prune (rot_corr.hpp;
// tscode/torsion_module.py:1013-1161, one schedule :1076-1152 per segment) and the moments of inertia with their pair search (moi.hpp;
// tscode/algebra.py:165-213, tscode/optimization_methods.py:327-358 per segment).  gfx950 only.  There is deliberately no CPU
// implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "refine_batch.hpp"

#include <algorithm>
#include <memory>
#include <vector>

// One run over many ensembles: every segment's centred structures live on the device from tsc_rot_corr_batch_begin to
// tsc_rot_corr_batch_end and are turned in place by the slots, as the reference turns its array; the caches of dissimilar pairs
// (:1121-1123) lie beside them, segment after segment.
struct tsc_rot_corr_batch : tsc::Owned {
    using Owned::Owned;
    std::vector<tsc::RotCorrSegment> segs;   // per segment: device pointers of its set-up, its offsets and words; d, num_active, thr per slot
    std::vector<int32_t> N;
    int64_t total_rows = 0, total_doubles = 0;
    double *coords = nullptr;
    uint32_t *cache = nullptr;
    int32_t *first = nullptr;
    unsigned long long *evaluated = nullptr;   // [segments]
};

using namespace tsc;

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_batch_destroy(tsc_rot_corr_batch *r) {
    TSC_API_GUARD_BEGIN
    return destroy_owned(r);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_batch_begin(tsc_ctx *c, const double *coords, const int64_t *offsets,
                                                                               const int32_t *n_structs, const int32_t *n_atoms,
                                                                               const int32_t *heavy, const int32_t *n_heavy,
                                                                               const int32_t *torsions, const int32_t *n_tors,
                                                                               const double *angles, const int32_t *n_angles,
                                                                               const uint8_t *move_mask, const int32_t *sub_ptr,
                                                                               const int32_t *sub_idx, int64_t n_segments,
                                                                               tsc_rot_corr_batch **out) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_rot_corr_batch_begin";
    TSC_REQUIRE(c && out, "%s: null argument", who);
    *out = nullptr;
    TSC_REQUIRE(n_segments >= 1 && n_segments <= (1 << 20), "%s: %lld segments", who, (long long)n_segments);
    TSC_REQUIRE(offsets && n_structs && n_atoms && n_heavy && n_tors && sub_ptr, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    const size_t S = size_t(n_segments);
    std::unique_ptr<tsc_rot_corr_batch> run(new tsc_rot_corr_batch(c));   // (in front of the HostCall: it outlives the call's wait for the stream)
    run->segs.resize(S);
    run->N.resize(S);
    // everything that can be refused is refused here, before anything touches the device; the message names the segment
    std::vector<int64_t> heavy0(S), tors0(S), mask0(S), ptr0(S), idx0(S);
    int64_t h0 = 0, t0 = 0, m0 = 0, p0 = 0, i0 = 0, row0 = 0, cache0 = 0;
    for (size_t s = 0; s < S; ++s) {
        const int64_t N = n_structs[s];
        const int n = n_atoms[s], T = n_tors[s], h = n_heavy[s];
        TSC_REQUIRE(T >= 0 && T <= RC_MAX_TORS && n >= 1 && n <= RC_MAX_ATOMS && h >= 0 && N >= 0,
                    "%s: segment %zu: %lld structures, %d atoms (1 .. %d), %d heavy, %d torsions (0 .. %d)", who, s, (long long)N, n, RC_MAX_ATOMS, h, T,
                    RC_MAX_TORS);
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == N * n * 3, "%s: segment %zu: offsets span %lld doubles, the segment is %lld x %d x 3", who, s,
                    (long long)(offsets[s + 1] - offsets[s]), (long long)N, n);
        TSC_REQUIRE(coords || offsets[s + 1] == 0, "%s: null argument", who);
        if (int rc = rot_corr_check_setup(N, n, heavy ? heavy + h0 : nullptr, h, torsions ? torsions + 4 * t0 : nullptr, T,
                                          angles ? angles + RC_MAX_ANGLES * t0 : nullptr, n_angles ? n_angles + t0 : nullptr,
                                          move_mask ? move_mask + m0 : nullptr, sub_ptr + p0, sub_idx ? sub_idx + i0 : nullptr)) {
            char msg[sizeof(g_err)];
            snprintf(msg, sizeof(msg), "%s", g_err);
            return fail(rc, "%s: segment %zu: %.400s", who, s, msg);
        }
        heavy0[s] = h0, tors0[s] = t0, mask0[s] = m0, ptr0[s] = p0, idx0[s] = i0;
        RotCorrSegment &g = run->segs[s];
        g.a.n = n, g.a.h = h, g.a.n_tors = T;
        g.coord0 = offsets[s], g.cache0 = cache0, g.row0 = row0, g.words = (N + 31) / 32;
        g.d = 0, g.num_active = 0, g.thr = 0.0, g.evaluated = nullptr;
        run->N[s] = int32_t(N);
        h0 += h, t0 += T, m0 += int64_t(T) * n, p0 += T + 1, i0 += sub_ptr[p0 - 1], row0 += N, cache0 += N * g.words;
        TSC_REQUIRE(row0 < INT32_MAX, "%s: the batch passes %d rows", who, INT32_MAX - 1);
    }
    run->total_rows = row0, run->total_doubles = offsets[S];
    // the run's blocks are the call's until everything is in place: an error hands them back behind an idle stream
    HostCall h(c);
    const int32_t *d_heavy, *d_tors, *d_n_angles, *d_sub_ptr, *d_sub_idx;
    const double *d_angles;
    const uint8_t *d_masks;
    TSC_TRY(h.in(heavy, size_t(h0), &d_heavy));
    TSC_TRY(h.in(torsions, size_t(t0) * 4, &d_tors));
    TSC_TRY(h.in(angles, size_t(t0) * RC_MAX_ANGLES, &d_angles));
    TSC_TRY(h.in(n_angles, size_t(t0), &d_n_angles));
    TSC_TRY(h.in(move_mask, size_t(m0), &d_masks));
    TSC_TRY(h.in(sub_ptr, size_t(p0), &d_sub_ptr));
    TSC_TRY(h.in(sub_idx, size_t(i0), &d_sub_idx));
    TSC_TRY(h.in(coords, size_t(run->total_doubles), &run->coords));
    TSC_TRY(h.scratch().get(size_t(std::max<int64_t>(cache0, 1)), &run->cache));
    TSC_TRY(h.scratch().get(size_t(std::max<int64_t>(row0, 1)), &run->first));
    TSC_TRY(h.scratch().get(S, &run->evaluated));
    if (cache0) TSC_HIP(hipMemsetAsync(run->cache, 0, size_t(cache0) * sizeof(uint32_t), c->stream));
    for (size_t s = 0; s < S; ++s) {
        RotCorrArgs &a = run->segs[s].a;
        a.heavy = d_heavy + heavy0[s], a.tors = d_tors + 4 * tors0[s], a.angles = d_angles + RC_MAX_ANGLES * tors0[s];
        a.n_angles = d_n_angles + tors0[s], a.masks = d_masks + mask0[s], a.sub_ptr = d_sub_ptr + ptr0[s], a.sub_idx = d_sub_idx + idx0[s];
    }
    TSC_TRY(h.finish());
    run->take_blocks(h.scratch());
    c->owned.adopt(run.get());   // (listed once complete: destroyed with the context, tsc_ctx_destroy)
    *out = run.release();
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_batch_pass(tsc_rot_corr_batch *r, const int32_t *open, const int64_t *d, int64_t k,
                                                                              const int64_t *num_active, const double *max_rmsd, int64_t n_open,
                                                                              int32_t *first, int64_t *pairs_evaluated) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_rot_corr_batch_pass";
    TSC_REQUIRE(r && (first || r->total_rows == 0), "%s: null argument", who);
    const int64_t S = int64_t(r->segs.size());
    TSC_REQUIRE(n_open >= 0 && n_open <= S, "%s: %lld open segments of %lld", who, (long long)n_open, (long long)S);
    TSC_REQUIRE(n_open == 0 || (open && d && num_active && max_rmsd && pairs_evaluated), "%s: null argument", who);
    TSC_REQUIRE(k > 0 && k < INT32_MAX && n_open * k < INT32_MAX, "%s: k = %lld with %lld open segments", who, (long long)k, (long long)n_open);
    std::vector<RotCorrSegment> segs{};   // (both in front of the HostCall: they outlive the call's wait for the stream)
    std::vector<unsigned long long> ev(size_t(n_open), 0ull);
    segs.resize(size_t(n_open));
    size_t lds = 0;
    for (int64_t q = 0; q < n_open; ++q) {
        const int64_t s = open[q];
        TSC_REQUIRE(s >= 0 && s < S && (q == 0 || s > open[q - 1]), "%s: open[%lld] = %lld: not an ascending list of segments below %lld", who, (long long)q,
                    (long long)s, (long long)S);
        const int64_t N = r->N[size_t(s)];
        TSC_REQUIRE(d[q] > 0 && num_active[q] >= 0 && num_active[q] <= N && d[q] <= N / k,
                    "%s: segment %lld: bad pass geometry (n = %lld, d = %lld, k = %lld, active = %lld)", who, (long long)s, (long long)N, (long long)d[q],
                    (long long)k, (long long)num_active[q]);
        TSC_REQUIRE(std::isfinite(max_rmsd[q]), "%s: segment %lld: max_rmsd not finite", who, (long long)s);
        RotCorrSegment &g = segs[size_t(q)];
        g = r->segs[size_t(s)];
        g.d = d[q], g.num_active = num_active[q], g.thr = max_rmsd[q], g.evaluated = r->evaluated + q;
        lds = std::max(lds, rot_corr_lds_bytes(g.a.n_tors, g.a.n, RC_WAVES));
    }
    tsc_ctx *c = r->ctx;
    HostCall h(c);
    if (r->total_rows) TSC_HIP(hipMemsetAsync(r->first, 0xff, size_t(r->total_rows) * sizeof(int32_t), c->stream));
    if (n_open) {
        const RotCorrSegment *d_segs;
        TSC_TRY(h.in(segs.data(), segs.size(), &d_segs));
        TSC_HIP(hipMemsetAsync(r->evaluated, 0, size_t(n_open) * sizeof(unsigned long long), c->stream));
        TSC_TRY(lds_attribute(&k_rot_corr_pass_seg, lds));
        hipLaunchKernelGGL(k_rot_corr_pass_seg, dim3(unsigned(n_open * k)), dim3(64 * RC_WAVES), lds, c->stream, d_segs, k, r->coords, r->cache, r->first);
        TSC_HIP(hipGetLastError());
        TSC_TRY(h.fetch(ev.data(), r->evaluated, size_t(n_open)));
    }
    if (r->total_rows) TSC_TRY(h.fetch(first, r->first, size_t(r->total_rows)));
    TSC_TRY(h.finish());
    for (int64_t q = 0; q < n_open; ++q) pairs_evaluated[q] = int64_t(ev[size_t(q)]);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_batch_end(tsc_rot_corr_batch *r, double *coords_out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && (coords_out || r->total_doubles == 0), "tsc_rot_corr_batch_end: null argument");
    HostCall h(r->ctx);
    if (r->total_doubles) TSC_TRY(h.fetch(coords_out, r->coords, size_t(r->total_doubles)));
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// moments of inertia and their pair search for many ensembles (moi.hpp)

namespace {

// the segment table of both MOI entry points: rows numbered through, coordinates and masses back to back
int moi_segments(const char *who, const int64_t *offsets, const int32_t *n_structs, const int32_t *n_atoms, const double *max_deviation,
                 int64_t n_segments, std::vector<MoiSegment> &segs, int64_t *total_rows, int64_t *total_masses) {
    segs.resize(size_t(n_segments));
    int64_t row0 = 0, mass0 = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        const int64_t N = n_structs[s];
        const int n = n_atoms ? n_atoms[s] : 0;
        TSC_REQUIRE(N >= 0 && (!n_atoms || n > 0), "%s: segment %lld: %lld structures of %d atoms", who, (long long)s, (long long)N, n);
        if (offsets)
            TSC_REQUIRE(offsets[s + 1] - offsets[s] == N * n * 3, "%s: segment %lld: offsets span %lld doubles, the segment is %lld x %d x 3", who,
                        (long long)s, (long long)(offsets[s + 1] - offsets[s]), (long long)N, n);
        MoiSegment &g = segs[size_t(s)];
        g.row0 = row0, g.coord0 = offsets ? offsets[s] : 0, g.mass0 = mass0, g.max_deviation = max_deviation ? max_deviation[s] : 0.0;
        g.N = int32_t(N), g.n = n;
        row0 += N, mass0 += n;
        TSC_REQUIRE(row0 < INT32_MAX, "%s: the batch passes %d rows", who, INT32_MAX - 1);
    }
    *total_rows = row0, *total_masses = mass0;
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_inertia_moments_batch(tsc_ctx *c, const double *structures, const int64_t *offsets,
                                                                                const int32_t *n_structs, const int32_t *n_atoms,
                                                                                const double *masses, int64_t n_segments, double *out) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_inertia_moments_batch";
    TSC_REQUIRE(c, "%s: null argument", who);
    TSC_REQUIRE(n_segments >= 0 && n_segments < INT_MAX, "%s: %lld segments", who, (long long)n_segments);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(offsets && n_structs && n_atoms && masses, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    std::vector<MoiSegment> segs{};   // (in front of the HostCall: it outlives the call's wait for the stream)
    int64_t total_rows = 0, total_masses = 0;
    TSC_TRY(moi_segments(who, offsets, n_structs, n_atoms, nullptr, n_segments, segs, &total_rows, &total_masses));
    if (total_rows == 0) return 0;
    TSC_REQUIRE(structures && out, "%s: null argument", who);
    HostCall h(c);
    const MoiSegment *d_segs;
    const double *d_s, *d_m;
    double *d_o;
    TSC_TRY(h.in(segs.data(), segs.size(), &d_segs));
    TSC_TRY(h.in(structures, size_t(offsets[n_segments]), &d_s));
    TSC_TRY(h.in(masses, size_t(total_masses), &d_m));
    TSC_TRY(h.out(out, size_t(total_rows) * 3, &d_o));
    hipLaunchKernelGGL(k_inertia_moments_seg, dim3(grid_for(total_rows, 256, 256 * 8)), dim3(256), 0, c->stream, d_s, d_m, d_segs, int(n_segments),
                       total_rows, d_o);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_moi_first_similar_batch(tsc_ctx *c, const double *moments, const int32_t *n_structs,
                                                                                  const double *max_deviation, int64_t n_segments, int32_t *first) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_moi_first_similar_batch";
    TSC_REQUIRE(c, "%s: null argument", who);
    TSC_REQUIRE(n_segments >= 0 && n_segments < INT_MAX, "%s: %lld segments", who, (long long)n_segments);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(n_structs && max_deviation, "%s: null argument", who);
    std::vector<MoiSegment> segs{};   // (in front of the HostCall)
    int64_t total_rows = 0, total_masses = 0;
    TSC_TRY(moi_segments(who, nullptr, n_structs, nullptr, max_deviation, n_segments, segs, &total_rows, &total_masses));
    if (total_rows == 0) return 0;
    TSC_REQUIRE(moments && first, "%s: null argument", who);
    HostCall h(c);
    const MoiSegment *d_segs;
    const double *d_m;
    int32_t *d_f;
    TSC_TRY(h.in(segs.data(), segs.size(), &d_segs));
    TSC_TRY(h.in(moments, size_t(total_rows) * 3, &d_m));
    TSC_TRY(h.out(first, size_t(total_rows), &d_f));
    hipLaunchKernelGGL(k_moi_first_similar_seg, dim3(grid_for(total_rows, 4, 256 * 16)), dim3(256), 0, c->stream, d_m, d_segs, int(n_segments), total_rows, d_f);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}
