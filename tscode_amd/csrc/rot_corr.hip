// rot_corr.hip -- launches and C ABI of the symmetry-corrected RMSD prune (rot_corr.hpp; tscode/torsion_module.py:953-1161).
// gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "rot_corr_kernels.hpp"

#include <algorithm>
#include <climits>
#include <memory>

// One run: the centred structures live on the device from tsc_rot_corr_begin to tsc_rot_corr_end and are turned in place by the
// passes, as the reference turns its array; the cache bitmap of dissimilar pairs (:1121-1123) lives beside them.
struct tsc_rot_corr : tsc::Owned {
    using Owned::Owned;
    int64_t N = 0, words = 0;
    tsc::RotCorrArgs a{};
    double *coords = nullptr;
    uint32_t *cache = nullptr;
    int32_t *first = nullptr;
    unsigned long long *evaluated = nullptr;
};

namespace {

using namespace tsc;

int upload_setup(HostCall &hc, RotCorrArgs &a, int n, const int32_t *heavy, int h, const int32_t *tors, int T, const double *angles,
                 const int32_t *n_angles, const uint8_t *mask, const int32_t *sub_ptr, const int32_t *sub_idx) {
    a.n = n, a.h = h, a.n_tors = T;
    TSC_TRY(hc.in(heavy, size_t(h), &a.heavy));
    TSC_TRY(hc.in(tors, size_t(T) * 4, &a.tors));
    TSC_TRY(hc.in(angles, size_t(T) * RC_MAX_ANGLES, &a.angles));
    TSC_TRY(hc.in(n_angles, size_t(T), &a.n_angles));
    TSC_TRY(hc.in(mask, size_t(T) * n, &a.masks));
    TSC_TRY(hc.in(sub_ptr, size_t(T) + 1, &a.sub_ptr));
    TSC_TRY(hc.in(sub_idx, size_t(sub_ptr[T]), &a.sub_idx));
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_destroy(tsc_rot_corr *r) {
    TSC_API_GUARD_BEGIN
    return destroy_owned(r);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_begin(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                         const int32_t *heavy, int n_heavy, const int32_t *torsions, int n_tors,
                                                                         const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                                                                         const int32_t *sub_ptr, const int32_t *sub_idx, tsc_rot_corr **out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && out && (coords || n_structs == 0), "tsc_rot_corr_begin: null argument");
    *out = nullptr;
    TSC_TRY(rot_corr_check_setup(n_structs, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    // the run's blocks are the call's until everything is in place: an error hands them back behind an idle stream
    HostCall h(c);
    std::unique_ptr<tsc_rot_corr> run(new tsc_rot_corr(c));
    run->N = n_structs;
    run->words = (n_structs + 31) / 32;
    TSC_TRY(upload_setup(h, run->a, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    TSC_TRY(h.in(coords, size_t(n_structs) * n_atoms * 3, &run->coords));
    TSC_TRY(h.scratch().get(size_t(n_structs) * run->words, &run->cache));
    TSC_TRY(h.scratch().get(size_t(n_structs), &run->first));
    TSC_TRY(h.scratch().get(1, &run->evaluated));
    if (n_structs) TSC_HIP(hipMemsetAsync(run->cache, 0, size_t(n_structs) * run->words * sizeof(uint32_t), c->stream));
    TSC_TRY(h.finish());
    run->take_blocks(h.scratch());
    c->owned.adopt(run.get());   // (listed once complete: destroyed with the context, tsc_ctx_destroy)
    *out = run.release();
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_pass(tsc_rot_corr *r, int64_t d, int64_t k, int64_t num_active, double max_rmsd,
                                                                        int32_t *first, int64_t *pairs_evaluated) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && first && pairs_evaluated, "tsc_rot_corr_pass: null argument");
    const int64_t N = r->N;
    TSC_REQUIRE(d > 0 && k > 0 && k < INT32_MAX && num_active >= 0 && num_active <= N && d * k <= N,
                "bad pass geometry (n = %lld, d = %lld, k = %lld, active = %lld)", (long long)N, (long long)d, (long long)k, (long long)num_active);
    TSC_REQUIRE(std::isfinite(max_rmsd), "tsc_rot_corr_pass: max_rmsd not finite");
    tsc_ctx *c = r->ctx;
    unsigned long long ev = 0;
    HostCall h(c);
    TSC_HIP(hipMemsetAsync(r->first, 0xff, size_t(N) * sizeof(int32_t), c->stream));
    TSC_HIP(hipMemsetAsync(r->evaluated, 0, sizeof(unsigned long long), c->stream));
    const size_t lds = rot_corr_lds_bytes(r->a.n_tors, r->a.n, RC_WAVES);
    TSC_TRY(lds_attribute(&k_rot_corr_pass, lds));
    hipLaunchKernelGGL(k_rot_corr_pass, dim3(unsigned(k)), dim3(64 * RC_WAVES), lds, c->stream, r->a, r->coords, d, k, num_active, max_rmsd, r->cache,
                       r->words, r->first, r->evaluated);
    TSC_HIP(hipGetLastError());
    TSC_TRY(h.fetch(first, r->first, size_t(N)));
    TSC_TRY(h.fetch(&ev, r->evaluated, 1));
    TSC_TRY(h.finish());
    *pairs_evaluated = int64_t(ev);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_end(tsc_rot_corr *r, double *coords_out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && (coords_out || r->N == 0), "tsc_rot_corr_end: null argument");
    tsc_ctx *c = r->ctx;
    HostCall h(c);
    TSC_TRY(h.fetch(coords_out, r->coords, size_t(r->N) * r->a.n * 3));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_pairs(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                         const int32_t *heavy, int n_heavy, const int32_t *torsions, int n_tors,
                                                                         const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                                                                         const int32_t *sub_ptr, const int32_t *sub_idx, const int32_t *pairs,
                                                                         int64_t n_pairs, double *rmsd, double *best_angle) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && (coords || n_structs == 0) && (n_pairs == 0 || (pairs && rmsd && (best_angle || n_tors == 0))),
                "tsc_rot_corr_pairs: null argument");
    TSC_REQUIRE(n_pairs >= 0, "tsc_rot_corr_pairs: negative pair count");
    TSC_TRY(rot_corr_check_setup(n_structs, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        TSC_REQUIRE(pairs[p] >= 0 && pairs[p] < n_structs, "tsc_rot_corr_pairs: pair %lld: structure index out of range", (long long)(p / 2));
    if (n_pairs == 0) return 0;
    HostCall h(c);
    RotCorrArgs a{};
    TSC_TRY(upload_setup(h, a, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    const double *d_coords;
    const int32_t *d_pairs;
    double *d_rmsd, *d_best;
    TSC_TRY(h.in(coords, size_t(n_structs) * n_atoms * 3, &d_coords));
    TSC_TRY(h.in(pairs, size_t(n_pairs) * 2, &d_pairs));
    TSC_TRY(h.out(rmsd, size_t(n_pairs), &d_rmsd));
    TSC_TRY(h.out(best_angle, size_t(n_pairs) * n_tors, &d_best));   // (null is allowed without torsions: nothing is written then)
    const size_t lds = rot_corr_lds_bytes(n_tors, n_atoms, RC_WAVES);
    TSC_TRY(lds_attribute(&k_rot_corr_pairs, lds));
    hipLaunchKernelGGL(k_rot_corr_pairs, dim3(grid_for(n_pairs, RC_WAVES, 256 * 4)), dim3(64 * RC_WAVES), lds, c->stream, a, d_coords, d_pairs,
                       n_pairs, d_rmsd, d_best);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}
