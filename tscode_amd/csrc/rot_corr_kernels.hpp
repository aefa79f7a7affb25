// rot_corr_kernels.hpp -- the pass and the value-level kernel of the symmetry-corrected RMSD prune for one ensemble (device
// functions: rot_corr.hpp).  Included only by rot_corr.hip, which launches them.
#pragma once
#include "rot_corr.hpp"

namespace tsc {

// One pass (:1080-1152 without the graph step): chunk blockIdx.x is [d*step, d*(step+1)), the last one [d*(k-1), num_active).
// first[i] = the first j of row i that is similar (rmsd < thr), or -1 (left as the caller set it for rows of empty chunks).
inline __global__ __launch_bounds__(64 * RC_WAVES) void k_rot_corr_pass(RotCorrArgs a, double *__restrict__ coords, int64_t d, int64_t k,
                                                                        int64_t num_active, double thr, uint32_t *__restrict__ cache,
                                                                        int64_t words, int32_t *__restrict__ first,
                                                                        unsigned long long *__restrict__ evaluated) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int64_t step = blockIdx.x;
    const int64_t lo = d * step, hi = step == k - 1 ? num_active : d * (step + 1);   // :1093-1096
    rot_corr_chunk(a, coords, cache, words, first, lo, hi, thr, s_raw, evaluated);
}

// The value-level form: one wavefront per pair, S[j] turned in LDS only (nothing is written back).
inline __global__ __launch_bounds__(64 * RC_WAVES) void k_rot_corr_pairs(RotCorrArgs a, const double *__restrict__ coords,
                                                                         const int32_t *__restrict__ pairs, int64_t n_pairs,
                                                                         double *__restrict__ rmsd, double *__restrict__ best_angle) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, n = a.n;
    const TorsionLists L = torsion_lists_at(s_raw, a.n_tors, n);
    build_torsion_lists(L, a.masks, a.tors, a.n_tors, n);
    double *c = reinterpret_cast<double *>(s_raw + torsion_lists_bytes(a.n_tors, n) + size_t(wid) * rot_corr_wave_bytes(n));
    double *best = c + size_t(n) * 3;
    for (int64_t p = int64_t(blockIdx.x) * nw + wid; p < n_pairs; p += int64_t(gridDim.x) * nw) {
        const double *src = coords + int64_t(pairs[2 * p + 1]) * n * 3;
        for (int e = lane; e < n * 3; e += 64) c[e] = src[e];
        __builtin_amdgcn_wave_barrier();
        const double r = rot_corr_pair(a, L, coords + int64_t(pairs[2 * p]) * n * 3, c, best, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) rmsd[p] = r;
        for (int t = lane; t < a.n_tors; t += 64) best_angle[p * a.n_tors + t] = best[t];
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace tsc
