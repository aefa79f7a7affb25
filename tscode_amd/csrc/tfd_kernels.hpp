// tfd_kernels.hpp -- the kernels of prune_conformers_tfd for one ensemble, of the greedy TFD filter and the two list helpers beside
// them (device functions: tfd.hpp).  Included only by adjacent.hip, which launches them.
#pragma once
#include "tfd.hpp"

namespace tsc {

// _get_tf_mat (:233-240): out f32[N][T]
inline __global__ __launch_bounds__(256) void k_torsion_fingerprints(const double *__restrict__ coords, int64_t N, int n, const int32_t *__restrict__ quads,
                                                               int T, float *__restrict__ out) {
    const int64_t total = N * T;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const int64_t s = e / T;
        out[e] = tfd_fingerprint_element(coords + s * n * 3, quads, int(e - s * T));
    }
}

// One pass of the pair search (:171-199): first[i] = tfd_first_similar_row of row i
inline __global__ __launch_bounds__(256) void k_tfd_first_similar(const float *__restrict__ tf, int64_t N, int T, int64_t d, int64_t k, int64_t num_active,
                                                            double thresh, int32_t *__restrict__ first) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); i < N; i += int64_t(gridDim.x) * 4) {
        const int32_t found = tfd_first_similar_row(tf, T, i, d, k, num_active, thresh, lane);
        if (lane == 0) first[i] = found;
    }
}

// blockIdx.x: 256 candidates, one per thread; blockIdx.y: a slice of the kept list.  The kept fingerprints are read from `kept_fp`, the
// compact copy k_tfd_greedy_replay keeps ([n_kept][T], in the order they were kept): the address is the same for every lane, so the
// loads are scalar loads and the comparison's operands sit in scalar registers -- no LDS, no barrier, no indirection through kept_list
// in front of every comparison (the first version walked kept_list -> tf per comparison: 207 us per super-block, an LDS-tiled one 153)
inline __global__ __launch_bounds__(256) void k_tfd_greedy_prior(const float *__restrict__ tf, int64_t base, int n_cand, int T, double thresh,
                                                           const float *__restrict__ kept_fp, const int32_t *__restrict__ n_kept,
                                                           uint8_t *__restrict__ dead) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int nk = *n_kept;
    const int per = (nk + int(gridDim.y) - 1) / int(gridDim.y);
    const int k0 = min(nk, int(blockIdx.y) * per), k1 = min(nk, k0 + per);
    const float *a = tf + (base + min(c, n_cand - 1)) * T;
    float ar[TG_REG_T];
    tfd_load_reg(a, T, ar);
    const TfdScreen sc = tfd_screen(T, thresh);
    bool live = c < n_cand;
    int k = k0;
    for (; k + 4 <= k1; k += 4) {  // four kept fingerprints at a time: their (scalar) loads are in flight together
        if (((k - k0) & 31) == 0) {
            if (live && dead[c]) live = false;  // another slice has settled this candidate (a hint: a stale read only costs work)
            if (!__any(live)) return;
        }
        const float *b = kept_fp + size_t(k) * T;
        const bool s0 = tfd_similar_reg(a, ar, b, T, thresh, sc), s1 = tfd_similar_reg(a, ar, b + T, T, thresh, sc);
        const bool s2 = tfd_similar_reg(a, ar, b + 2 * T, T, thresh, sc), s3 = tfd_similar_reg(a, ar, b + 3 * T, T, thresh, sc);
        if (live && (s0 || s1 || s2 || s3)) {
            dead[c] = 1;
            live = false;
        }
    }
    for (; k < k1; ++k)
        if (live && tfd_similar_reg(a, ar, kept_fp + size_t(k) * T, T, thresh, sc)) {
            dead[c] = 1;
            live = false;
        }
}

// sim[c][w] bit j: candidate c of the super-block is similar to its candidate 64 w + j, for 64 w + j < c (zero elsewhere: every
// word is written); nz[c / 64] bit c % 64: row c has a bit set at all (zeroed by the caller).  blockIdx.x = w (its 64 fingerprints
// in LDS), blockIdx.y * 256 + threadIdx.x = c.
inline __global__ __launch_bounds__(256) void k_tfd_greedy_pairs(const float *__restrict__ tf, int64_t base, int n_cand, int T, double thresh,
                                                           unsigned long long *__restrict__ sim, unsigned long long *__restrict__ nz) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tfd_raw[];
    float *s_tile = reinterpret_cast<float *>(s_tfd_raw);
    const int w = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    const int ncol = max(0, min(64, n_cand - 64 * w));
    const bool staged = 64 * T <= 12288;
    if (staged) {
        for (int e = threadIdx.x; e < ncol * T; e += 256) s_tile[e] = tf[(base + 64 * w) * T + e];
        __syncthreads();
    }
    if (c >= TG_SUPER) return;
    unsigned long long bits = 0ull;
    if (c < n_cand && 64 * w < c) {
        const float *a = tf + (base + c) * T;
        float ar[TG_REG_T];
        tfd_load_reg(a, T, ar);
        const TfdScreen sc = tfd_screen(T, thresh);
        const int jn = min(64, c - 64 * w);
        for (int j = 0; j < jn; ++j) {
            const float *b = staged ? s_tile + j * T : tf + (base + 64 * w + j) * T;
            if (tfd_similar_reg(a, ar, b, T, thresh, sc)) bits |= 1ull << j;
        }
    }
    sim[size_t(c) * TG_WORDS + w] = bits;
    if (bits) atomicOr(&nz[c >> 6], 1ull << (c & 63));
}

inline __global__ __launch_bounds__(64) void k_tfd_greedy_replay(const unsigned long long *__restrict__ sim, const unsigned long long *__restrict__ nz,
                                                           int64_t base, int n_cand, const uint8_t *__restrict__ dead_in,
                                                           uint8_t *__restrict__ accepted, int32_t *__restrict__ kept_list, int32_t *__restrict__ n_kept,
                                                           int32_t *__restrict__ n_kept_before) {
    const int lane = threadIdx.x;
    const int n_blocks = (n_cand + 63) / 64;
    // dead bits of block `lane` (candidates past the end count as dead) and which of its rows have any bit set
    unsigned long long D = 0ull;
    for (int i = 0; i < 64; ++i) {
        const int c = 64 * lane + i;
        if (c >= n_cand || dead_in[c]) D |= 1ull << i;
    }
    const unsigned long long NZ = nz[lane];
    unsigned long long W = 0ull;  // kept bits of block `lane`
    unsigned long long row[2][64], corner[2];
#pragma unroll
    for (int i = 0; i < 64; ++i) row[0][i] = sim[size_t(i) * TG_WORDS + lane];
    corner[0] = sim[size_t(lane) * TG_WORDS + 0];
    int nk = *n_kept;
    if (lane == 0) *n_kept_before = nk;  // (k_tfd_greedy_keep copies the fingerprints of what this super-block adds)
    auto block = [&](const int B, const unsigned long long(&cur)[64], unsigned long long(&nxt)[64], const unsigned long long cw,
                     unsigned long long &cw_next) __attribute__((always_inline)) {
        if (B + 1 < n_blocks) {
#pragma unroll
            for (int i = 0; i < 64; ++i) nxt[i] = sim[(size_t(B + 1) * 64 + i) * TG_WORDS + lane];
            cw_next = sim[(size_t(B + 1) * 64 + lane) * TG_WORDS + (B + 1)];  // row 64 (B + 1) + lane, the word of its own block
        }
        const unsigned long long dead = readlane64(D, B);
        const unsigned long long need = readlane64(NZ, B) & ~dead;  // alive rows that are similar to anything before them
        // against the blocks before this one: W of lane B is still zero, so the block's own corner does not take part
        unsigned long long blocked = dead;
#pragma unroll
        for (int i = 0; i < 64; ++i)
            if ((need >> i) & 1ull)
                if (__any((cur[i] & W) != 0ull)) blocked |= 1ull << i;
        // the block's own corner, in order: rows without a bit are kept as they are; a row's bits only name rows before it
        unsigned long long acc = ~dead & ~need;
        for (unsigned long long todo = need & ~blocked; todo; todo &= todo - 1ull) {
            const int i = __ffsll((long long)todo) - 1;
            if ((readlane64(cw, i) & acc) == 0ull) acc |= 1ull << i;
        }
        if (lane == B) W = acc;
        const int c = 64 * B + lane;
        if (c < n_cand) {
            const bool ok = (acc >> lane) & 1ull;
            accepted[base + c] = ok ? 1 : 0;
            if (ok) kept_list[nk + __popcll(acc & ((1ull << lane) - 1ull))] = int32_t(base + c);
        }
        nk += __popcll(acc);
    };
    for (int B = 0; B < n_blocks; B += 2) {
        block(B, row[0], row[1], corner[0], corner[1]);
        if (B + 1 < n_blocks) block(B + 1, row[1], row[0], corner[1], corner[0]);
    }
    if (lane == 0) *n_kept = nk;
}

// the fingerprints of the structures the last super-block kept, appended to the compact copy k_tfd_greedy_prior reads (one workgroup: a few
// hundred fingerprints; inside the one-wavefront replay kernel the same copy cost 20 us per super-block)
inline __global__ __launch_bounds__(256) void k_tfd_greedy_keep(const float *__restrict__ tf, int T, const int32_t *__restrict__ kept_list,
                                                          const int32_t *__restrict__ n_kept_before, const int32_t *__restrict__ n_kept,
                                                          float *__restrict__ kept_fp) {
    const int s0 = *n_kept_before, total = (*n_kept - s0) * T;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int slot = s0 + e / T, t = e - (e / T) * T;
        kept_fp[size_t(slot) * T + t] = tf[int64_t(kept_list[slot]) * T + t];
    }
}

// flags of a compacted list back onto the full index space: full[idx[r]] = part[r] (full is zeroed by the caller)
inline __global__ __launch_bounds__(256) void k_scatter_flags(const uint8_t *__restrict__ part, const int32_t *__restrict__ idx, const int32_t *__restrict__ n_dev,
                                                        uint8_t *__restrict__ full) {
    const int n = *n_dev;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) full[idx[r]] = part[r];
}

// offsets of candidate groups in the list of the candidates that passed a filter: out[g] = pos[group_off[g]] (pos = exclusive
// scan of the filter's mask), out[n_groups] = total
inline __global__ __launch_bounds__(256) void k_group_offsets_after_filter(const int32_t *__restrict__ group_off, int n_groups, const int32_t *__restrict__ pos,
                                                                     int64_t n, const int32_t *__restrict__ total, int32_t *__restrict__ out) {
    for (int g = blockIdx.x * 256 + threadIdx.x; g <= n_groups; g += gridDim.x * 256) out[g] = (g == n_groups || group_off[g] >= n) ? *total : pos[group_off[g]];
}

}  // namespace tsc
