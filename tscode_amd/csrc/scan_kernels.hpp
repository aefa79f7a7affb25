// scan_kernels.hpp -- the two kernels of the ordered compaction's exclusive scan and scan_mask, which enqueues them (device functions
// and sizes: scan.hpp).  Included only by the units that call scan_mask: embed.hip, adjacent.hip, pipeline.hip.
#pragma once
#include "scan.hpp"

namespace tsc {

// pass 1: per-block count of non-zero mask bytes
// gate (optional): the kernels of a speculatively enqueued pass return at once when *gate == 0.
inline __global__ __launch_bounds__(SCAN_THREADS) void k_scan_block_sums(const uint8_t *__restrict__ mask, int64_t n,
                                                                   int32_t *__restrict__ bsum, const int *__restrict__ gate) {
    __shared__ int s_w[SCAN_THREADS / WAVE];
    if (gate && *gate == 0) return;
    int64_t base = (int64_t(blockIdx.x) * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    int c = (base < n) ? count_nonzero_bytes(load_mask8(mask, base, n)) : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

inline __global__ __launch_bounds__(SCAN_THREADS) void k_scan_write(const uint8_t *__restrict__ mask, int64_t n,
                                                              const int32_t *__restrict__ bsum, int32_t *__restrict__ pos,
                                                              int32_t *__restrict__ act_idx, uint8_t *__restrict__ mbit_bytes,
                                                              int32_t *__restrict__ total_out, const int *__restrict__ gate,
                                                              int32_t *total_host = nullptr) {
    __shared__ int s_w[SCAN_THREADS / WAVE];
    __shared__ int s_o[SCAN_THREADS / WAVE];
    if (gate && *gate == 0) return;
    scan_write_block(mask, n, bsum, pos, act_idx, mbit_bytes, total_out, s_w, s_o, total_host);
}

// Enqueue the two passes.  bsum must hold ceil(n / SCAN_TILE) + 1 ints.  pos may be null (then only
// act_idx / mbit are produced); total_dev (optional) receives count_nonzero(mask).
// bsum_current: the caller keeps bsum up to date itself (the prune run does, through k_apply_pass), so the
// counting pass is skipped.
inline int scan_mask(hipStream_t st, const uint8_t *mask, int64_t n, int32_t *bsum, int32_t *pos, int32_t *act_idx,
                     uint8_t *mbit_bytes, int32_t *total_dev, const int *gate = nullptr, bool bsum_current = false, int32_t *total_host = nullptr) {
    int nb = int(ceil_div<int64_t>(n + 1, SCAN_TILE));  // n + 1: some thread always owns index n (writes pos[n])
    if (!bsum_current) hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(SCAN_THREADS), 0, st, mask, n, bsum, gate);
    hipLaunchKernelGGL(k_scan_write, dim3(nb), dim3(SCAN_THREADS), 0, st, mask, n, (const int32_t *)bsum, pos, act_idx, mbit_bytes, total_dev, gate, total_host);
    TSC_HIP(hipGetLastError());
    return 0;
}

}  // namespace tsc
