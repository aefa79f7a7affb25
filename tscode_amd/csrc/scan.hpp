// scan.hpp -- ordered compaction primitives: exclusive scan of a byte mask, bit packing, row gathers.
// NumPy's structures[mask] keeps order, and the pruning result depends on that order, so every
// compaction here is a stable one driven by an exclusive prefix sum (no atomics).
// No kernel here: the device functions and sizes that other kernels use too (rmsd.hpp).  k_scan_block_sums, k_scan_write and
// scan_mask are in scan_kernels.hpp, k_gather_rows and its launcher in gather_rows.hpp.
#pragma once
#include "common.hpp"

namespace tsc {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;                             // bytes per thread: one 64-bit load
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;     // 2048 mask bytes per block

__device__ inline uint64_t load_mask8(const uint8_t *__restrict__ mask, int64_t base, int64_t n) {
    // 8 mask bytes starting at base (base % 8 == 0), zero beyond n; mask is hipMalloc-aligned.
    if (base + 8 <= n) return *reinterpret_cast<const uint64_t *>(mask + base);
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b)
        if (base + b < n) v |= uint64_t(mask[base + b]) << (8 * b);
    return v;
}

__device__ inline int count_nonzero_bytes(uint64_t v) {
    // number of non-zero bytes in v
    uint64_t t = v | (v >> 4);
    t |= t >> 2;
    t |= t >> 1;
    t &= 0x0101010101010101ull;
    return __popcll(t);
}

// pass 2: pos[i] = number of non-zero mask bytes before i (pos[n] = total); optionally the list of
// kept indices (act_idx[pos[i]] = i) and the mask as a bit array (bit i of mbit = mask[i] != 0).
// (the work of one block; s_w, s_o: SCAN_THREADS / WAVE ints of LDS each)
__device__ inline void scan_write_block(const uint8_t *__restrict__ mask, int64_t n, const int32_t *__restrict__ bsum,
                                        int32_t *__restrict__ pos, int32_t *__restrict__ act_idx, uint8_t *__restrict__ mbit_bytes,
                                        int32_t *__restrict__ total_out, int *s_w, int *s_o, volatile int32_t *total_host = nullptr) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // exclusive offset of this block = sum of the counts of the blocks before it (a few hundred values at most)
    int part = 0;
    for (int i = threadIdx.x; i < int(blockIdx.x); i += SCAN_THREADS) part += bsum[i];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) s_o[wid] = part;
    int64_t base = (int64_t(blockIdx.x) * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    uint64_t v = (base < n) ? load_mask8(mask, base, n) : 0;
    int c = count_nonzero_bytes(v);
    int incl = c;
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_w[wid] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += s_w[w];
    const int block_off = s_o[0] + s_o[1] + s_o[2] + s_o[3];
    int run = block_off + woff + incl - c;
    uint8_t bits = 0;
    for (int b = 0; b < SCAN_ITEMS; ++b) {
        int64_t i = base + b;
        if (i >= n) break;
        bool on = ((v >> (8 * b)) & 0xff) != 0;
        if (pos) pos[i] = run;
        if (on) {
            if (act_idx) act_idx[run] = int32_t(i);
            bits |= uint8_t(1u << b);
            ++run;
        }
    }
    if (mbit_bytes && base < n) mbit_bytes[base >> 3] = bits;
    if (base <= n && n < base + SCAN_ITEMS) {  // the thread owning the tail knows the total
        if (pos) pos[n] = run;
        if (total_out) *total_out = run;
        if (total_host) {  // (pinned host memory the host is looking at: no copy command, no event in the stream)
            *total_host = run;
            __threadfence_system();
        }
    }
}

inline int scan_grid_blocks(int64_t n) { return int(ceil_div<int64_t>(n + 1, SCAN_TILE)); }

inline size_t scan_bsum_count(int64_t n) { return size_t(ceil_div<int64_t>(n + 1, SCAN_TILE)) + 2; }

}  // namespace tsc
