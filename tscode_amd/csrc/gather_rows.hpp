// gather_rows.hpp -- the ordered row gather behind a scan: k_gather_rows and its launcher.  Included only by the units that call
// launch_gather_rows: embed.hip, adjacent.hip.
#pragma once
#include "common.hpp"

namespace tsc {

// dst[r] = src[idx[r]] for rows of row_words 8-byte words; idx == nullptr means identity.
// sel (optional) picks words inside the row: dst[r][w] = src[idx[r]][sel[w]] for w < out_words
// (used for the heavy-atom gather, where a "word" is one coordinate triple = 3 doubles handled as 3 words).
inline __global__ __launch_bounds__(256) void k_gather_rows(const uint64_t *__restrict__ src, const int32_t *__restrict__ idx,
                                                      int64_t n_out, int row_words, const int32_t *__restrict__ sel,
                                                      int out_words, uint64_t *__restrict__ dst) {
    int64_t total = n_out * out_words;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        int64_t r = e / out_words;
        int w = int(e - r * out_words);
        int64_t s = idx ? idx[r] : r;
        int sw = sel ? sel[w] : w;
        dst[e] = src[s * row_words + sw];
    }
}

inline int launch_gather_rows(hipStream_t st, const void *src, const int32_t *idx, int64_t n_out, int row_words,
                              const int32_t *sel, int out_words, void *dst) {
    if (n_out <= 0) return 0;
    int64_t total = n_out * out_words;
    int blocks = int(std::min<int64_t>(ceil_div<int64_t>(total, 256), 256 * 16));
    hipLaunchKernelGGL(k_gather_rows, dim3(blocks), dim3(256), 0, st, static_cast<const uint64_t *>(src), idx, n_out,
                       row_words, sel, out_words, static_cast<uint64_t *>(dst));
    TSC_HIP(hipGetLastError());
    return 0;
}

}  // namespace tsc
