// diverse_kernels.hpp -- the kernels of alignment, k-means and the diverse-conformer pick for one ensemble: one-line wrappers of the
// device functions of diverse.hpp on the problem's own grid.  Included only by diverse.hip, which launches them.
#pragma once
#include "diverse.hpp"
#include "diverse_align_kernel.hpp"

namespace tsc {

inline __global__ __launch_bounds__(256) void k_col_partial(const double *__restrict__ X, int64_t N, int D, int squares, double *__restrict__ part) {
    dv_col_partial(X, N, D, squares, part, blockIdx.x, blockIdx.y, gridDim.y);
}

inline __global__ __launch_bounds__(256) void k_col_finish(const double *__restrict__ part, int chunks, int D, double scale, double *__restrict__ out) {
    dv_col_finish(part, chunks, D, scale, out, blockIdx.x);
}

// X[i, d] += sign * v[d]
inline __global__ __launch_bounds__(256) void k_shift_cols(double *__restrict__ X, int64_t rows, int D, const double *__restrict__ v, double sign) {
    const int64_t total = rows * D;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) X[e] += sign * v[e % D];
}

inline __global__ __launch_bounds__(256) void k_gather_rows(const double *__restrict__ X, int D, const int32_t *__restrict__ rows, int k, double *__restrict__ out) {
    const int64_t total = int64_t(k) * D;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) out[e] = X[int64_t(rows[e / D]) * D + e % D];
}

inline __global__ __launch_bounds__(1024) void k_sum_fixed(const double *__restrict__ v, int64_t n, double scale, double *__restrict__ out) {
    dv_sum_fixed(v, n, scale, out);
}

inline __global__ __launch_bounds__(256) void k_row_norms(const double *__restrict__ X, int64_t rows, int D, double *__restrict__ out) {
    dv_row_norms(X, rows, D, out, blockIdx.x);
}

template <int NT>
__global__ __launch_bounds__(256) void k_kmeans_assign(const double *__restrict__ X, int64_t N, int D, const double *__restrict__ C, int k,
                                                       const double *__restrict__ xn, const double *__restrict__ cn, int32_t *__restrict__ labels,
                                                       double *__restrict__ own_d2, int *__restrict__ changed) {
    dv_kmeans_assign<NT>(X, N, D, C, k, xn, cn, labels, own_d2, changed, blockIdx.x);
}

inline __global__ __launch_bounds__(256) void k_own_d2(const double *__restrict__ X, int64_t N, int D, const double *__restrict__ C,
                                                       const int32_t *__restrict__ labels, const int32_t *__restrict__ counts, int k, int only_if_empty,
                                                       double *__restrict__ own_d2) {
    dv_own_d2(X, N, D, C, labels, counts, k, only_if_empty, own_d2, blockIdx.x);
}

inline __global__ __launch_bounds__(256) void k_label_count(const int32_t *__restrict__ labels, int64_t N, int32_t *__restrict__ counts) {
    dv_label_count(labels, N, counts, blockIdx.x);
}

inline __global__ __launch_bounds__(256) void k_label_bucket(const int32_t *__restrict__ labels, int64_t N, const int32_t *__restrict__ counts, int k,
                                                             int32_t *__restrict__ offs, int32_t *__restrict__ members) {
    dv_label_bucket(labels, N, counts, k, offs, members, blockIdx.x);
}

inline __global__ __launch_bounds__(256) void k_kmeans_relocate(const double *__restrict__ own_d2, int64_t N, const int32_t *__restrict__ labels,
                                                                const int32_t *__restrict__ counts, int k, KmControl *__restrict__ ctl) {
    dv_kmeans_relocate(own_d2, N, labels, counts, k, ctl);
}

inline __global__ __launch_bounds__(256) void k_kmeans_update(const double *__restrict__ X, int D, const int32_t *__restrict__ members,
                                                              const int32_t *__restrict__ offs, const int32_t *__restrict__ counts,
                                                              const KmControl *__restrict__ ctl, double *__restrict__ C, double *__restrict__ shift_part) {
    dv_kmeans_update(X, D, members, offs, counts, ctl, C, shift_part, blockIdx.x, blockIdx.y, gridDim.y);
}

inline __global__ __launch_bounds__(64) void k_kmeans_control(const double *__restrict__ shift_part, int n_part, const int *__restrict__ changed,
                                                              KmControl *__restrict__ ctl) {
    dv_kmeans_control(shift_part, n_part, changed, ctl);
}

inline __global__ __launch_bounds__(256) void k_diverse_pick(const double *__restrict__ X, int n, const int32_t *__restrict__ members,
                                                             const int32_t *__restrict__ offs, const int32_t *__restrict__ counts,
                                                             const double *__restrict__ C, int k, const double *__restrict__ energies,
                                                             int32_t *__restrict__ picked) {
    dv_diverse_pick(X, n, members, offs, counts, C, k, energies, picked, blockIdx.x);
}

inline __global__ __launch_bounds__(256) void k_kmeans_seed_update(const double *__restrict__ X, int64_t N, int D, const int32_t *__restrict__ rows, int j,
                                                                   double *__restrict__ min_d2) {
    dv_kmeans_seed_update(X, N, D, rows, j, min_d2, blockIdx.x);
}

inline __global__ __launch_bounds__(1024) void k_kmeans_seed_pick(const double *__restrict__ min_d2, int64_t N, const double *__restrict__ u, int j,
                                                                  int32_t *__restrict__ rows) {
    dv_kmeans_seed_pick(min_d2, N, u, j, rows);
}

}  // namespace tsc
