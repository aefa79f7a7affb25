// mm_kernels.hpp -- the non-template kernels of the matrix-core screen (mm.hpp): the records of a run that gets them outside
// k_open_rows, and the screen's values and verdicts for tests.  Included only by prune.hip, which launches them.
#pragma once
#include "mm.hpp"

namespace tsc {

// records of n structures from their descriptors (runs that get their records outside k_open_rows: the screen's self-test)
inline __global__ __launch_bounds__(256) void k_mm_records(const float *__restrict__ D, int64_t n, const unsigned *__restrict__ dmax_bits, _Float16 *__restrict__ col_rec) {
    const float sigma = mm_scale(*dmax_bits);
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        float d[DW];
#pragma unroll
        for (int q = 0; q < DW / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(D + i * DW + 4 * q);
            d[4 * q] = v.x, d[4 * q + 1] = v.y, d[4 * q + 2] = v.z, d[4 * q + 3] = v.w;
        }
        mm_write_record(d, sigma, col_rec + i * MM_REC_HALVES);
    }
}

// The screen's values themselves, for tests: S[fam][r][c] of rows [0, 64) against columns [0, n_cols) of the records (one wavefront
// per 16 columns), and the limit's bit pattern.
inline __global__ __launch_bounds__(64) void k_mm_screen_dump(const _Float16 *__restrict__ recs, int n_cols,
                                                        const unsigned *__restrict__ dmax_bits, double limit, float *__restrict__ S, int *__restrict__ limit_bits) {
    const int lane = threadIdx.x, g = lane >> 4, rc = lane & 15, c0 = blockIdx.x * MM_STEP;
    if (blockIdx.x == 0 && lane == 0) *limit_bits = __float_as_int(screen_limit_mm(*dmax_bits, limit));
    const int col = min(c0 + rc, n_cols - 1);
#pragma unroll
    for (int fam = 0; fam < NFAM; ++fam) {
        const f16x4 b = mm_load_B(recs + int64_t(col) * MM_REC_HALVES, fam, g);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            const int row = min(16 * rt + rc, n_cols - 1);
            const f16x4 a = mm_load_A(recs + int64_t(row) * MM_REC_HALVES, fam, g);
            const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, z, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + rc < n_cols) S[(size_t(fam) * MM_ROWS + 16 * rt + 4 * g + i) * n_cols + c0 + rc] = acc[i];
        }
    }
}

// The screen's verdicts themselves, for tests, in the form the pair kernels compute them: the operands of mm_load_A / mm_load_B2, every
// accumulator started at minus the limit, keep[r][c] = 1 where the sign bits of both families' results are set (rows [0, 64) against
// columns [0, n_cols); one wavefront per 16 columns).  With the limit among the summed terms the rounding is not that of k_mm_screen_dump's
// `S <= limit` on the host.
inline __global__ __launch_bounds__(64) void k_mm_screen_keeps(const _Float16 *__restrict__ recs, int n_cols, const unsigned *__restrict__ dmax_bits, double limit,
                                                         unsigned char *__restrict__ keep, int *__restrict__ limit_bits) {
    const int lane = threadIdx.x, g = lane >> 4, rc = lane & 15, c0 = blockIdx.x * MM_STEP;
    const float limit_mm = screen_limit_mm(*dmax_bits, limit);
    if (blockIdx.x == 0 && lane == 0) *limit_bits = __float_as_int(limit_mm);
    f16x4 B[NFAM];
    mm_load_B2(recs + int64_t(min(c0 + rc, n_cols - 1)) * MM_REC_HALVES, g, B);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int row = min(16 * rt + rc, n_cols - 1);
        const f16x4 a0 = mm_load_A(recs + int64_t(row) * MM_REC_HALVES, 0, g), a1 = mm_load_A(recs + int64_t(row) * MM_REC_HALVES, 1, g);
        const f32x4 z = {-limit_mm, -limit_mm, -limit_mm, -limit_mm};
        const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x16f16(a0, B[0], z, 0, 0, 0);
        const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x16f16(a1, B[1], z, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c0 + rc < n_cols) keep[size_t(16 * rt + 4 * g + i) * n_cols + c0 + rc] = (unsigned char)((__float_as_uint(s0[i]) & __float_as_uint(s1[i])) >> 31);
    }
}

}  // namespace tsc
