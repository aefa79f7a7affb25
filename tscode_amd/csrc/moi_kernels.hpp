// moi_kernels.hpp -- the kernels of the moments of inertia, their pair search and the embed scores for one ensemble (device
// functions: moi.hpp).  Included only by adjacent.hip, which launches them.
#pragma once
#include "moi.hpp"

namespace tsc {

inline __global__ __launch_bounds__(256) void k_inertia_moments(const double *__restrict__ structures, int64_t N, int n, const double *__restrict__ masses,
                                                          double *__restrict__ out) {
    for (int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < N; s += int64_t(gridDim.x) * blockDim.x)
        inertia_moments_of(structures + s * n * 3, n, masses, out + 3 * s);
}

// algebra.py:188-205: first[i] = moi_first_similar_row of row i
inline __global__ __launch_bounds__(256) void k_moi_first_similar(const double *__restrict__ mo, int64_t N, double max_deviation, int32_t *__restrict__ first) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); i < N; i += int64_t(gridDim.x) * 4) {
        const int32_t found = moi_first_similar_row(mo, N, i, max_deviation, lane);
        if (lane == 0) first[i] = found;
    }
}

// numba_functions.py:273-288 _score_embed_poses (float32 accumulator, as the reference's array) and the signed error of
// fitness_check (optimization_methods.py:544-557; a NaN target stands for None and is skipped)
inline __global__ __launch_bounds__(256) void k_embed_scores(const double *__restrict__ structures, int64_t N, int n, const int32_t *__restrict__ indices,
                                                       const double *__restrict__ distances, int n_c, float *__restrict__ scores,
                                                       double *__restrict__ fitness_error) {
    for (int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < N; s += int64_t(gridDim.x) * blockDim.x) {
        const double *c = structures + s * n * 3;
        float sc = 0.0f;
        double err = 0.0;
        for (int i = 0; i < n_c; ++i) {
            const int a = indices[(s * n_c + i) * 2], b = indices[(s * n_c + i) * 2 + 1];
            const double dx = c[3 * a] - c[3 * b], dy = c[3 * a + 1] - c[3 * b + 1], dz = c[3 * a + 2] - c[3 * b + 2];
            const double dist = sqrt(dx * dx + dy * dy + dz * dz), target = distances[s * n_c + i];
            if (target == target) {
                sc = float(double(sc) + fabs(dist - target));
                err += dist - target;
            }
        }
        scores[s] = sc;
        fitness_error[s] = err;
    }
}

}  // namespace tsc
