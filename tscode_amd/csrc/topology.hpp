// topology.hpp -- bond graphs from distances and their difference to an expected graph, one wavefront per structure.
//
// What the reference does per structure in Python double loops: graphize (tscode/graph_manipulations.py:28-55: atoms i < j are
// bonded iff both are active and |r_i - r_j| < 1.2 (rcov_i + rcov_j)), then molecule_check / scramble_check (tscode/utils.py:341-387:
// the symmetric difference of the bond set with an expected one, bonds that touch an excluded atom dropped, compared with
// max_newbonds); get_double_bonds_indices (tscode/utils.py:293-314) is the same scan with another threshold table.
//
// The atoms of an ensemble share their elements, so a threshold depends on the pair of element CLASSES only: the host hands over
// class[n] (at most 16 classes) and the squared bounds bound[T][T] (clash_sq_bound of the reference's fp64 threshold, so that
// d2 < bound is the reference's sqrt-then-compare verdict; d2 itself is formed with the reference's roundings -- three products,
// two sums, no fused multiply-add -- as norm_of does, tscode/algebra.py:90-96).  Inactive atoms and the lanes behind the last atom
// belong to one more class whose bounds are 0: never bonded, no test in the loop.
//
// Shape: the structure is staged in LDS by coalesced loads; lane l keeps atoms l, l + 64, ... in registers; the row atom i is read
// from LDS at a wave-uniform address (a broadcast); every lane forms d2 to its atom of column tile tc and compares it with its
// class pair's bound; one __ballot gives the 64 columns of row i as a word, and everything behind it is wave-uniform integer
// work: xor with the expected row, and with the care word, population count.  Only column tiles at or right of the diagonal are
// visited.  Stores: one lane per element, no atomics.
#pragma once

#include "common.hpp"

namespace tsc {

constexpr int TP_MAX_ATOMS = 512;
constexpr int TP_MAX_W = TP_MAX_ATOMS / 64;
constexpr int TP_MAX_CLASSES = 16;
constexpr int TP_MAX_EXCL = 16;
constexpr int TP_TABLE = TP_MAX_CLASSES + 1;  // + the class of inactive atoms

struct TopoArgs {
    int64_t n_structs;
    int n;      // atoms per structure
    int n_tab;  // classes, the inactive one (n_tab - 1) included
    int n_excl; // slots per structure of the per-structure excluded list (0: none)
    long long max_newbonds;
    uint64_t excl_words[TP_MAX_W];            // atoms excluded in every structure, one bit each
    double bound[TP_TABLE * TP_TABLE];        // squared bounds by class pair
    uint8_t cls[TP_MAX_ATOMS];                // class of every atom (inactive atoms: n_tab - 1)
};

__host__ __device__ inline size_t topo_lds_bytes(int n) { return size_t(4) * 3 * n * sizeof(double); }

// W = ceil(n / 64) column tiles.  ref (optional) u64[n][W]: the expected bonds, strict upper triangle.  excl (optional)
// i32[n_structs][n_excl]: atoms excluded in that structure only (-1 or anything outside 0 .. n-1: an unused slot).
// adj (optional) u64[n_structs][n][W]: the bonds found, strict upper triangle.
template <int W>
inline __global__ __launch_bounds__(256) void k_bond_delta(TopoArgs a, const double *__restrict__ coords, const uint64_t *__restrict__ ref,
                                                     const int32_t *__restrict__ excl, uint8_t *__restrict__ mask,
                                                     int32_t *__restrict__ formed, int32_t *__restrict__ broken,
                                                     uint64_t *__restrict__ adj) {
    extern __shared__ __attribute__((aligned(16))) double s_xyz[];
    __shared__ double s_bound[TP_TABLE * TP_TABLE];
    __shared__ int s_cls[TP_MAX_ATOMS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = a.n, T = a.n_tab;
    for (int e = threadIdx.x; e < T * T; e += 256) s_bound[e] = a.bound[e];
    for (int e = threadIdx.x; e < TP_MAX_ATOMS; e += 256) s_cls[e] = e < n ? int(a.cls[e]) : T - 1;
    __syncthreads();
    int cl[W];
#pragma unroll
    for (int t = 0; t < W; ++t) cl[t] = s_cls[lane + 64 * t];
    double *w = s_xyz + size_t(wid) * 3 * n;
    const int64_t waves_total = int64_t(gridDim.x) * 4;
    for (int64_t s = int64_t(blockIdx.x) * 4 + wid; s < a.n_structs; s += waves_total) {
        const double *src = coords + s * n * 3;
        for (int e = lane; e < 3 * n; e += 64) w[e] = src[e];
        // the excluded atoms of this structure as one bit each (wave-uniform)
        uint64_t exc[W];
#pragma unroll
        for (int t = 0; t < W; ++t) exc[t] = a.excl_words[t];
        if (excl) {
            for (int q = 0; q < a.n_excl; ++q) {
                const int e = __builtin_amdgcn_readfirstlane(excl[s * a.n_excl + q]);  // (the same address in every lane)
#pragma unroll
                for (int t = 0; t < W; ++t)
                    if (e >= 64 * t && e < 64 * t + 64 && e < n) exc[t] |= 1ull << (e & 63);
            }
        }
        __builtin_amdgcn_wave_barrier();
        double x[W], y[W], z[W];
#pragma unroll
        for (int t = 0; t < W; ++t) {
            const int j = lane + 64 * t;
            const bool in = j < n;
            x[t] = in ? w[3 * j] : 0.0, y[t] = in ? w[3 * j + 1] : 0.0, z[t] = in ? w[3 * j + 2] : 0.0;
        }
        int nf = 0, nb = 0;
#pragma unroll
        for (int tr = 0; tr < W; ++tr) {
            const int rows = min(64, n - 64 * tr);
            uint64_t mine[W];  // row 64 tr + lane of the adjacency, gathered for one coalesced store per row tile
#pragma unroll
            for (int t = 0; t < W; ++t) mine[t] = 0;
            for (int r = 0; r < rows; ++r) {
                const int i = 64 * tr + r;
                const double xi = w[3 * i], yi = w[3 * i + 1], zi = w[3 * i + 2];
                const double *brow = s_bound + s_cls[i] * T;
                const uint64_t above = r == 63 ? 0ull : ~0ull << (r + 1);
                const bool row_cared = ((exc[tr] >> r) & 1ull) == 0;
#pragma unroll
                for (int tc = tr; tc < W; ++tc) {
                    double d2;
                    {
#pragma clang fp contract(off)
                        const double dx = xi - x[tc], dy = yi - y[tc], dz = zi - z[tc];
                        d2 = dx * dx + dy * dy + dz * dz;
                    }
                    uint64_t bits = __ballot(d2 < brow[cl[tc]]);
                    if (tc == tr) bits &= above;
                    const uint64_t rf = ref ? ref[size_t(i) * W + tc] : 0ull;
                    const uint64_t care = row_cared ? ~exc[tc] : 0ull;
                    nf += __popcll(bits & ~rf & care);
                    nb += __popcll(~bits & rf & care);
                    if (adj && lane == r) mine[tc] = bits;
                }
            }
            if (adj && lane < rows) {
                uint64_t *dst = adj + (size_t(s) * n + 64 * tr + lane) * W;
#pragma unroll
                for (int t = 0; t < W; ++t) dst[t] = mine[t];
            }
        }
        if (lane == 0) {
            mask[s] = uint8_t((long long)nf + nb <= a.max_newbonds ? 1 : 0);
            if (formed) formed[s] = nf;
            if (broken) broken[s] = nb;
        }
        __builtin_amdgcn_wave_barrier();  // the next structure overwrites this wavefront's LDS rows
    }
}

}  // namespace tsc
