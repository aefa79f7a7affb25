// rot_corr.hip -- launches and C ABI of the symmetry-corrected RMSD prune (rot_corr.hpp; tscode/torsion_module.py:953-1161).
// gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "rot_corr.hpp"

#include <algorithm>
#include <climits>

// One run: the centred structures live on the device from tsc_rot_corr_begin to tsc_rot_corr_end and are turned in place by the
// passes, as the reference turns its array; the cache bitmap of dissimilar pairs (:1121-1123) lives beside them.
struct tsc_rot_corr {
    tsc_ctx *ctx = nullptr;
    int64_t N = 0, words = 0;
    tsc::RotCorrArgs a{};
    double *coords = nullptr;
    uint32_t *cache = nullptr;
    int32_t *first = nullptr;
    unsigned long long *evaluated = nullptr;
    std::vector<void *> blocks;
};

namespace {

using namespace tsc;

template <typename T>
int rc_get(tsc_rot_corr *r, size_t count, T **out) {
    void *p = nullptr;
    TSC_TRY(r->ctx->alloc((count ? count : 1) * sizeof(T), &p));
    r->blocks.push_back(p);
    *out = static_cast<T *>(p);
    return 0;
}

template <typename T>
int rc_put(tsc_rot_corr *r, const T *host, size_t count, const T **out) {
    T *d;
    TSC_TRY(rc_get(r, count, &d));
    if (count) TSC_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, r->ctx->stream));
    *out = d;
    return 0;
}

// the limits of the ABI (include/tscode_hip.h), checked on the host arrays before anything touches the device
int check_setup(int64_t N, int n, const int32_t *heavy, int h, const int32_t *tors, int T, const double *angles, const int32_t *n_angles,
                const uint8_t *mask, const int32_t *sub_ptr, const int32_t *sub_idx) {
    TSC_REQUIRE(heavy && (T == 0 || (tors && angles && n_angles && mask)) && sub_ptr && (T == 0 || sub_idx), "rot_corr: null argument");
    TSC_REQUIRE(N >= 0 && N < INT32_MAX, "rot_corr: %lld structures (at most %d)", (long long)N, INT32_MAX - 1);
    TSC_REQUIRE(n >= 1 && n <= RC_MAX_ATOMS, "rot_corr: %d atoms per structure (1 .. %d)", n, RC_MAX_ATOMS);
    TSC_REQUIRE(T >= 0 && T <= RC_MAX_TORS, "rot_corr: %d torsions (0 .. %d)", T, RC_MAX_TORS);
    TSC_REQUIRE(h >= 1 && h <= n, "rot_corr: %d heavy atoms of %d", h, n);
    for (int q = 0; q < h; ++q) TSC_REQUIRE(heavy[q] >= 0 && heavy[q] < n, "rot_corr: heavy atom index %d out of range", heavy[q]);
    TSC_REQUIRE(sub_ptr[0] == 0, "rot_corr: sub_ptr[0] must be 0");
    for (int t = 0; t < T; ++t) {
        for (int q = 0; q < 4; ++q) TSC_REQUIRE(tors[4 * t + q] >= 0 && tors[4 * t + q] < n, "rot_corr: torsion %d: atom index out of range", t);
        TSC_REQUIRE(n_angles[t] >= 1 && n_angles[t] <= RC_MAX_ANGLES, "rot_corr: torsion %d: %d angles (1 .. %d)", t, n_angles[t], RC_MAX_ANGLES);
        for (int q = 0; q < n_angles[t]; ++q) TSC_REQUIRE(std::isfinite(angles[RC_MAX_ANGLES * t + q]), "rot_corr: torsion %d: angle not finite", t);
        TSC_REQUIRE(sub_ptr[t + 1] > sub_ptr[t] && sub_ptr[t + 1] - sub_ptr[t] <= n, "rot_corr: torsion %d: local subgraph of %d atoms", t,
                    sub_ptr[t + 1] - sub_ptr[t]);
        for (int q = sub_ptr[t]; q < sub_ptr[t + 1]; ++q) TSC_REQUIRE(sub_idx[q] >= 0 && sub_idx[q] < n, "rot_corr: subgraph index out of range");
    }
    return 0;
}

int upload_setup(tsc_rot_corr *r, int n, const int32_t *heavy, int h, const int32_t *tors, int T, const double *angles,
                 const int32_t *n_angles, const uint8_t *mask, const int32_t *sub_ptr, const int32_t *sub_idx) {
    RotCorrArgs &a = r->a;
    a.n = n, a.h = h, a.n_tors = T;
    TSC_TRY(rc_put(r, heavy, size_t(h), &a.heavy));
    TSC_TRY(rc_put(r, tors, size_t(T) * 4, &a.tors));
    TSC_TRY(rc_put(r, angles, size_t(T) * RC_MAX_ANGLES, &a.angles));
    TSC_TRY(rc_put(r, n_angles, size_t(T), &a.n_angles));
    TSC_TRY(rc_put(r, mask, size_t(T) * n, &a.masks));
    TSC_TRY(rc_put(r, sub_ptr, size_t(T) + 1, &a.sub_ptr));
    TSC_TRY(rc_put(r, sub_idx, size_t(sub_ptr[T]), &a.sub_idx));
    return 0;
}

template <typename K>
int lds_attribute(K kernel, size_t lds) {
    if (lds > 64 * 1024) TSC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    return 0;
}

void free_run(tsc_rot_corr *r) {
    for (void *p : r->blocks) r->ctx->release(p);
    delete r;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_destroy(tsc_rot_corr *r) {
    TSC_API_GUARD_BEGIN
    if (!r) return 0;
    DeviceGuard guard(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    {
        std::lock_guard<std::mutex> lock(r->ctx->runs_mutex);
        auto &lr = r->ctx->live_rot_corr;
        lr.erase(std::remove(lr.begin(), lr.end(), r), lr.end());
    }
    free_run(r);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_begin(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                         const int32_t *heavy, int n_heavy, const int32_t *torsions, int n_tors,
                                                                         const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                                                                         const int32_t *sub_ptr, const int32_t *sub_idx, tsc_rot_corr **out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && out && (coords || n_structs == 0), "tsc_rot_corr_begin: null argument");
    *out = nullptr;
    TSC_TRY(check_setup(n_structs, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    DeviceGuard guard(c->device);
    tsc_rot_corr *r = new tsc_rot_corr;
    r->ctx = c;
    r->N = n_structs;
    r->words = (n_structs + 31) / 32;
    int rc = upload_setup(r, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx);
    const double *d_coords = nullptr;
    if (!rc) rc = rc_put(r, coords, size_t(n_structs) * n_atoms * 3, &d_coords);
    if (!rc) rc = rc_get(r, size_t(n_structs) * r->words, &r->cache);
    if (!rc) rc = rc_get(r, size_t(n_structs), &r->first);
    if (!rc) rc = rc_get(r, 1, &r->evaluated);
    if (!rc && n_structs) {
        hipError_t e = hipMemsetAsync(r->cache, 0, size_t(n_structs) * r->words * sizeof(uint32_t), c->stream);
        if (e != hipSuccess) rc = fail(TSC_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        free_run(r);
        return rc;
    }
    r->coords = const_cast<double *>(d_coords);
    {
        std::lock_guard<std::mutex> lock(c->runs_mutex);
        c->live_rot_corr.push_back(r);
    }
    *out = r;
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
    DeviceGuard guard(c->device);
    TSC_HIP(hipMemsetAsync(r->first, 0xff, size_t(N) * sizeof(int32_t), c->stream));
    TSC_HIP(hipMemsetAsync(r->evaluated, 0, sizeof(unsigned long long), c->stream));
    const size_t lds = rot_corr_lds_bytes(r->a.n_tors, r->a.n, RC_WAVES);
    TSC_TRY(lds_attribute(&k_rot_corr_pass, lds));
    hipLaunchKernelGGL(k_rot_corr_pass, dim3(unsigned(k)), dim3(64 * RC_WAVES), lds, c->stream, r->a, r->coords, d, k, num_active, max_rmsd, r->cache,
                       r->words, r->first, r->evaluated);
    TSC_HIP(hipGetLastError());
    unsigned long long ev = 0;
    TSC_HIP(hipMemcpyAsync(first, r->first, size_t(N) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipMemcpyAsync(&ev, r->evaluated, sizeof(ev), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    *pairs_evaluated = int64_t(ev);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rot_corr_end(tsc_rot_corr *r, double *coords_out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && (coords_out || r->N == 0), "tsc_rot_corr_end: null argument");
    tsc_ctx *c = r->ctx;
    DeviceGuard guard(c->device);
    TSC_HIP(hipMemcpyAsync(coords_out, r->coords, size_t(r->N) * r->a.n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    return 0;
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
    TSC_TRY(check_setup(n_structs, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        TSC_REQUIRE(pairs[p] >= 0 && pairs[p] < n_structs, "tsc_rot_corr_pairs: pair %lld: structure index out of range", (long long)(p / 2));
    if (n_pairs == 0) return 0;
    DeviceGuard guard(c->device);
    // a run object only as the owner of the uploaded set-up (never listed: it does not outlive this call)
    tsc_rot_corr tmp;
    tmp.ctx = c;
    struct Release {
        tsc_rot_corr *r;
        ~Release() {
            (void)hipStreamSynchronize(r->ctx->stream);
            for (void *p : r->blocks) r->ctx->release(p);
        }
    } release{&tmp};
    TSC_TRY(upload_setup(&tmp, n_atoms, heavy, n_heavy, torsions, n_tors, angles, n_angles, move_mask, sub_ptr, sub_idx));
    const double *d_coords;
    const int32_t *d_pairs;
    double *d_rmsd, *d_best;
    TSC_TRY(rc_put(&tmp, coords, size_t(n_structs) * n_atoms * 3, &d_coords));
    TSC_TRY(rc_put(&tmp, pairs, size_t(n_pairs) * 2, &d_pairs));
    TSC_TRY(rc_get(&tmp, size_t(n_pairs), &d_rmsd));
    TSC_TRY(rc_get(&tmp, size_t(n_pairs) * n_tors, &d_best));
    const size_t lds = rot_corr_lds_bytes(n_tors, n_atoms, RC_WAVES);
    TSC_TRY(lds_attribute(&k_rot_corr_pairs, lds));
    hipLaunchKernelGGL(k_rot_corr_pairs, dim3(grid_for(n_pairs, RC_WAVES, 256 * 4)), dim3(64 * RC_WAVES), lds, c->stream, tmp.a, d_coords, d_pairs,
                       n_pairs, d_rmsd, d_best);
    TSC_HIP(hipGetLastError());
    TSC_HIP(hipMemcpyAsync(rmsd, d_rmsd, size_t(n_pairs) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_tors) TSC_HIP(hipMemcpyAsync(best_angle, d_best, size_t(n_pairs) * n_tors * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    return 0;
    TSC_API_GUARD_END
}
