// cull_layout.hpp -- what lays a culled pass out in front of its pair kernel (cull.hpp): the once-per-run Morton sort, the verdict
// culled-or-walked, the ordered partition by chunk and the tiles' bounding boxes.  Included only by prune.hip, which launches them.
#pragma once
#include "cull.hpp"

namespace tsc {

// ---- once per run: the structures in (coarse) Morton order of their descriptors ---------------------------------------------
__device__ inline unsigned morton_cell(const float *__restrict__ d, float inv_dmax) {
    unsigned code = 0;
#pragma unroll
    for (int k = 0; k < CULL_MORTON_DIMS; ++k) {
        const float x = d[2 * k] * inv_dmax * 0.5f + 0.5f;  // component k of family 0 (families interleaved), mapped to [0, 1]
        int q = int(x * float(1 << CULL_MORTON_BITS));
        q = q < 0 ? 0 : (q >= (1 << CULL_MORTON_BITS) ? (1 << CULL_MORTON_BITS) - 1 : q);   // (a NaN component lands in cell 0)
#pragma unroll
        for (int b = 0; b < CULL_MORTON_BITS; ++b) code |= ((unsigned(q) >> b) & 1u) << (b * CULL_MORTON_DIMS + k);
    }
    return code;
}
// The order has to come out THE SAME on every rank of a sharded run (the ranks deal the row tiles of the sorted layout among
// themselves: with layouts of their own they would miss pairs), so it is a STABLE sort by cell, ties in index order: two passes of
// a least-significant-digit radix sort over 8 bits, each an ordered partition into 256 buckets -- per block of 2048 entries the
// number of entries per bucket; their exclusive prefix over blocks and buckets; a scatter that ranks the entries of a wavefront by
// ballots (entry order kept).
constexpr int RADIX_BUCKETS = 256;
__device__ inline int radix_digit(const float *__restrict__ D, const int32_t *__restrict__ in, int64_t m, int64_t n, float inv, int shift, int &id) {
    id = 0;
    if (m >= n) return -1;
    id = in ? in[m] : int(m);
    return int((morton_cell(D + int64_t(id) * DW, inv) >> shift) & (RADIX_BUCKETS - 1));
}
inline __global__ __launch_bounds__(256) void k_radix_count(const float *__restrict__ D, const int32_t *__restrict__ in, int64_t n, const unsigned *__restrict__ dmax_bits,
                                                      int shift, int32_t *__restrict__ blk_cnt) {
    __shared__ int s_cnt[RADIX_BUCKETS];
    const float dmax = __uint_as_float(*dmax_bits);
    const float inv = (dmax > 0.0f && dmax < 3.0e38f) ? 1.0f / dmax : 0.0f;
    const int tid = threadIdx.x;
    s_cnt[tid] = 0;
    __syncthreads();
    const int64_t m0 = int64_t(blockIdx.x) * 2048;
    for (int u = 0; u < 8; ++u) {
        int id;
        const int d = radix_digit(D, in, m0 + u * 256 + tid, n, inv, shift, id);
        if (d >= 0) atomicAdd(&s_cnt[d], 1);
    }
    __syncthreads();
    blk_cnt[int64_t(blockIdx.x) * RADIX_BUCKETS + tid] = s_cnt[tid];
}
// blk_cnt[b][d] -> entries with digit d in the blocks before b (one wavefront per digit), tot[d] = entries with digit d
inline __global__ __launch_bounds__(64) void k_radix_scan(int n_blocks, int32_t *__restrict__ blk_cnt, int32_t *__restrict__ tot) {
    const int d = blockIdx.x, lane = threadIdx.x & 63;
    int run = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < n_blocks ? blk_cnt[int64_t(b) * RADIX_BUCKETS + d] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (b < n_blocks) blk_cnt[int64_t(b) * RADIX_BUCKETS + d] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) tot[d] = run;
}
// tot[d] -> first output slot of digit d (exclusive prefix over the 256 digits; one block)
inline __global__ __launch_bounds__(256) void k_radix_base(int32_t *__restrict__ tot) {
    __shared__ int s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int v = tot[tid];
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_part[wv] = incl;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < wv; ++q) base += s_part[q];
    tot[tid] = base + incl - v;
}
inline __global__ __launch_bounds__(256) void k_radix_scatter(const float *__restrict__ D, const int32_t *__restrict__ in, int64_t n, const unsigned *__restrict__ dmax_bits,
                                                        int shift, const int32_t *__restrict__ blk_base, const int32_t *__restrict__ digit_base,
                                                        int32_t *__restrict__ out) {
    __shared__ int s_cnt[32][RADIX_BUCKETS];
    const float dmax = __uint_as_float(*dmax_bits);
    const float inv = (dmax > 0.0f && dmax < 3.0e38f) ? 1.0f / dmax : 0.0f;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    for (int e = tid; e < 32 * RADIX_BUCKETS; e += 256) (&s_cnt[0][0])[e] = 0;
    __syncthreads();
    const int64_t m0 = int64_t(blockIdx.x) * 2048;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int my_d[8], my_id[8], my_rank[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        my_d[u] = radix_digit(D, in, m0 + u * 256 + tid, n, inv, shift, my_id[u]);
        my_rank[u] = 0;
        for (unsigned long long left = __ballot(my_d[u] >= 0); left;) {   // the lanes of a wavefront that share a digit, in lane order
            const int dd = __shfl(my_d[u], __ffsll((long long)left) - 1);
            const unsigned long long same = __ballot(my_d[u] == dd);
            if (my_d[u] == dd) my_rank[u] = __popcll(same & lt);
            if (lane == 0) s_cnt[u * 4 + wv][dd] = __popcll(same);
            left &= ~same;
        }
    }
    __syncthreads();
    {   // exclusive prefix over the block's 32 (round, wavefront) slots per digit, on top of the digit's base and the block's offset in it
        int run = digit_base[tid] + blk_base[int64_t(blockIdx.x) * RADIX_BUCKETS + tid];
        for (int sl = 0; sl < 32; ++sl) {
            const int v = s_cnt[sl][tid];
            s_cnt[sl][tid] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (my_d[u] >= 0) out[s_cnt[u * 4 + wv][my_d[u]] + my_rank[u]] = my_id[u];
}

// ---- once per culled pass ----------------------------------------------------------------------------------------------
// cbase[c] = active structures before chunk c of the open pass (c = 0 .. k; cbase[k] = A): chunk c takes the positions
// [cbase[c], cbase[c + 1]) of the sorted layout -- the rank range of the chunk, in another order.  Also clears the fill counters.
inline __global__ __launch_bounds__(64) void k_chunk_bases(PassGeom g, const PruneState *__restrict__ st, const int32_t *__restrict__ boff,
                                                     const unsigned long long *__restrict__ bits, int bit_words, int n_blocks, int32_t *__restrict__ cbase,
                                                     int32_t *__restrict__ cfill) {
    const unsigned long long *X = bits + size_t(st->bitsel) * bit_words;
    const int n_all = st->n_active;
    const int c = blockIdx.x;  // one wavefront per chunk boundary (grid = k + 1)
    const int64_t pos = c < g.k ? int64_t(c) * g.cs : int64_t(g.n);
    // (a pass partitioned over ranks runs on the LOCAL rows 0 .. A - 1 of this rank's chunks: ranks relative to row_lo, clamped to them)
    const int r = rank_below_wave(boff, X, n_blocks, n_all, pos) - st->row_lo;
    if ((threadIdx.x & 63) == 0) cbase[c] = r < 0 ? 0 : (r > st->A ? st->A : r), cfill[c] = 0;
}

// Culled or walked?  The ordered walk looks at the pairs inside the rows' ranges (r, cend[r]) -- W of them, summed by k_open_rows;
// the culled kernel at the tile pairs whose boxes lie within the limit, whatever the ranges are: a share f of ALL pairs of the
// chunks that falls with the chunk length (measured at 1M x 50: 0.27 at 22 000 active structures per chunk, 0.19 at 62 000,
// 0.13 at 206 000: about 0.27 (22 000 / len)^(1/3)) at two thirds of the walk's rate per pair (what the boxes leave are the near
// tiles, dense in candidates).  Where the reference's cache ends most rows early (W a few per cent of all pairs: C4's k = 5 and
// k = 1 passes) the walk has little to do and keeps the pass.  One wavefront; the verdict goes to pinned host memory, the host
// waits for it (a pass that large takes a millisecond or more; enqueueing both kernels and letting the loser's 10^5 workgroups
// start and leave cost 0.1-0.2 ms a pass) and launches one flow or the other.
inline __global__ __launch_bounds__(64) void k_cull_decide(PruneState *__restrict__ st, const PassCounters *__restrict__ cnt, const int32_t *__restrict__ cbase, int k,
                                                     int force, int *__restrict__ flag_host) {
    const int lane = threadIdx.x & 63;
    unsigned long long w = __hip_atomic_load(&cnt->w[lane][CNT_WALK], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
    double all = 0.0, longest = 0.0;
    if (lane < k) {
        const double len = double(cbase[lane + 1] - cbase[lane]);
        all = 0.5 * len * len, longest = len;
    }
    for (int off = 32; off > 0; off >>= 1) all += __shfl_xor(all, off), longest = fmax(longest, __shfl_xor(longest, off));
    if (lane == 0) {
        const double f = 0.27 * cbrt(22000.0 / fmax(longest, 1.0));
        const int on = (w > 0 && (force || double(w) > 1.5 * f * all)) ? 1 : 0;  // (force: option "cull" = 2, tests; w = 0: a pass that is gated off, or whose rows have no columns left)
        st->cull_on = on;
        flag_host[1] = st->A;   // (the rows of the pass: a pass that is WALKED is launched for these, not for the ensemble the run began with)
        *flag_host = on;
        __threadfence_system();
    }
}

// The active structures of the pass, chunk by chunk, each chunk in the run's Morton order -- an ORDERED partition of that order by
// chunk, so that 128 consecutive positions of a chunk are 128 neighbours on the curve (a layout that only kept a block's structures
// together gave column tiles that mixed two distant places of the curve, and the boxes culled a quarter of the tiles instead of
// three quarters).  Three launches: per block of 2048 entries the number of active structures per chunk; their exclusive prefix
// over the blocks (one wavefront per chunk); the scatter, which ranks every structure inside its block by ballots -- entry order
// is kept inside a block as well -- and moves what the pair kernel reads BY POSITION: the descriptor and the structure's active
// rank (crank: what the verdicts are expressed in).
constexpr int CULL_LAYOUT_ITEMS = 2048;
constexpr int CULL_LAYOUT_SLOTS = CULL_LAYOUT_ITEMS / 64;   // (round, wavefront) slots of a block: 64 consecutive entries each

// chunk of entry m of the Morton order if that structure is active, else -1
struct LayoutRange {
    int s_lo, s_hi;   // structures [s_lo, s_hi) take part (a pass partitioned over ranks: this rank's chunks; else all n)
};
__device__ inline int layout_chunk(const PassGeom &g, const LayoutRange lr, const int32_t *__restrict__ order, const unsigned long long *__restrict__ X, int64_t m, int &i) {
    i = 0;
    if (m >= g.n) return -1;
    i = order[m];
    if (i < lr.s_lo || i >= lr.s_hi || !((X[i >> 6] >> (i & 63)) & 1ull)) return -1;
    const int c = i / g.cs;
    return c >= g.k ? g.k - 1 : c;
}
// s_cnt[slot][chunk] = active structures of chunk `chunk` among the 64 entries of slot `slot`; mine = this lane's chunk (-1: none);
// returns the lane's rank among the lanes of its wavefront with the same chunk
__device__ inline int layout_wave_rank(int mine, int *s_cnt_slot) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int rank = 0;
    for (unsigned long long left = __ballot(mine >= 0); left;) {
        const int c = __shfl(mine, __ffsll((long long)left) - 1);
        const unsigned long long same = __ballot(mine == c);
        if (mine == c) rank = __popcll(same & lt);
        if (lane == 0 && s_cnt_slot) s_cnt_slot[c] = __popcll(same);
        left &= ~same;
    }
    return rank;
}
inline __global__ __launch_bounds__(256) void k_layout_count(PassGeom g, LayoutRange lr, const PruneState *__restrict__ st, const int32_t *__restrict__ order,
                                                      const unsigned long long *__restrict__ bits, int bit_words, int32_t *__restrict__ blk_cnt) {
    __shared__ int s_cnt[CULL_MAX_CHUNKS];
    if (st->pass_on == 0) return;
    const unsigned long long *X = bits + size_t(st->bitsel) * bit_words;
    const int tid = threadIdx.x;
    if (tid < CULL_MAX_CHUNKS) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t m0 = int64_t(blockIdx.x) * CULL_LAYOUT_ITEMS;
    for (int u = 0; u < CULL_LAYOUT_ITEMS / 256; ++u) {
        int i;
        const int c = layout_chunk(g, lr, order, X, m0 + u * 256 + tid, i);
        for (unsigned long long left = __ballot(c >= 0); left;) {   // one LDS atomic per (wavefront, chunk present)
            const int cc = __shfl(c, __ffsll((long long)left) - 1);
            const unsigned long long same = __ballot(c == cc);
            if ((tid & 63) == 0) atomicAdd(&s_cnt[cc], __popcll(same));
            left &= ~same;
        }
    }
    __syncthreads();
    if (tid < g.k) blk_cnt[int64_t(blockIdx.x) * CULL_MAX_CHUNKS + tid] = s_cnt[tid];
}
// blk_cnt[b][c] -> first position of block b's structures of chunk c: cbase[c] + structures of chunk c in the blocks before b
inline __global__ __launch_bounds__(64) void k_layout_scan(const PruneState *__restrict__ st, int n_layout_blocks, const int32_t *__restrict__ cbase,
                                                     int32_t *__restrict__ blk_cnt) {
    if (st->pass_on == 0) return;
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    int run = cbase[c];
    for (int b0 = 0; b0 < n_layout_blocks; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < n_layout_blocks ? blk_cnt[int64_t(b) * CULL_MAX_CHUNKS + c] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (b < n_layout_blocks) blk_cnt[int64_t(b) * CULL_MAX_CHUNKS + c] = run + incl - v;
        run += __shfl(incl, 63);
    }
}
inline __global__ __launch_bounds__(256) void k_layout_scatter(PassGeom g, LayoutRange lr, const PruneState *__restrict__ st, const int32_t *__restrict__ order,
                                                        const unsigned long long *__restrict__ bits, int bit_words, const int32_t *__restrict__ rank_of,
                                                        const float *__restrict__ Dc, const int32_t *__restrict__ blk_base, float *__restrict__ Ds,
                                                        int32_t *__restrict__ crank, const _Float16 *__restrict__ Dh = nullptr,
                                                        _Float16 *__restrict__ Dhs = nullptr, int32_t *__restrict__ cstruct = nullptr) {
    // cstruct (optional): the structure at every sorted position (= act[crank[pos]]: cull_mm.hpp reads a candidate's coordinates one
    // round trip earlier with it)
    // Dh -> Dhs (optional): the float16 records of the matrix-core screen (mm_record.hpp) move along with the descriptors
    __shared__ int s_cnt[CULL_LAYOUT_SLOTS][CULL_MAX_CHUNKS];
    if (st->pass_on == 0) return;
    const unsigned long long *X = bits + size_t(st->bitsel) * bit_words;
    const int tid = threadIdx.x, wv = tid >> 6;
    for (int e = tid; e < CULL_LAYOUT_SLOTS * CULL_MAX_CHUNKS; e += 256) (&s_cnt[0][0])[e] = 0;
    __syncthreads();
    const int64_t m0 = int64_t(blockIdx.x) * CULL_LAYOUT_ITEMS;
    int my_c[CULL_LAYOUT_ITEMS / 256], my_i[CULL_LAYOUT_ITEMS / 256], my_rank[CULL_LAYOUT_ITEMS / 256];
#pragma unroll
    for (int u = 0; u < CULL_LAYOUT_ITEMS / 256; ++u) {
        my_c[u] = layout_chunk(g, lr, order, X, m0 + u * 256 + tid, my_i[u]);
        my_rank[u] = layout_wave_rank(my_c[u], s_cnt[u * 4 + wv]);
    }
    __syncthreads();
    // exclusive prefix over the block's 32 slots, per chunk, on top of the block's base
    if (tid < g.k) {
        int run = blk_base[int64_t(blockIdx.x) * CULL_MAX_CHUNKS + tid];
        for (int sl = 0; sl < CULL_LAYOUT_SLOTS; ++sl) {
            const int v = s_cnt[sl][tid];
            s_cnt[sl][tid] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < CULL_LAYOUT_ITEMS / 256; ++u) {
        if (my_c[u] < 0) continue;
        const int pos = s_cnt[u * 4 + wv][my_c[u]] + my_rank[u];
        const int r = rank_of[my_i[u]];
        crank[pos] = r;
        if (cstruct) cstruct[pos] = my_i[u];
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Dc + int64_t(r) * DW);
        f32x4 *dst = reinterpret_cast<f32x4 *>(Ds + int64_t(pos) * DW);
#pragma unroll
        for (int q = 0; q < DW / 4; ++q) dst[q] = src[q];
        if (Dhs) {
            const f32x4 *hs = reinterpret_cast<const f32x4 *>(Dh + int64_t(r) * MM_REC_HALVES);
            f32x4 *hd = reinterpret_cast<f32x4 *>(Dhs + int64_t(pos) * MM_REC_HALVES);
#pragma unroll
            for (int q = 0; q < MM_REC_HALVES / 8; ++q) hd[q] = hs[q];
        }
    }
}

// Bounding boxes of the sorted layout: per 128 positions one column box and eight row boxes (16 positions each), lo[16] then
// hi[16].  Positions beyond the active count do not exist: an empty box (lo = +inf, hi = -inf) is infinitely far from everything.
inline __global__ __launch_bounds__(128) void k_tile_boxes(const PruneState *__restrict__ st, const float *__restrict__ Ds, float *__restrict__ cbox,
                                                     float *__restrict__ rbox) {
    __shared__ float s_d[CULL_COLS][DW + 1];
    const int A = st->pass_on ? st->A : 0;
    const int64_t p0 = int64_t(blockIdx.x) * CULL_COLS;
    const int tid = threadIdx.x;
    for (int e = tid; e < CULL_COLS * DW; e += 128) {
        const int p = e / DW, k = e - p * DW;
        s_d[p][k] = (p0 + p < A) ? Ds[(p0 + p) * DW + k] : __builtin_nanf("");
    }
    __syncthreads();
    const int t = tid / DW, k = tid - t * DW;  // row tile t of this block, component k
    float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float v = s_d[16 * t + q][k];
        lo = fminf(lo, v), hi = fmaxf(hi, v);  // (fminf / fmaxf ignore the NaN of an absent position)
    }
    float *rb = rbox + (int64_t(blockIdx.x) * 8 + t) * CULL_BOX;
    rb[k] = lo, rb[DW + k] = hi;
    __syncthreads();
    s_d[t][k] = lo, s_d[8 + t][k] = hi;
    __syncthreads();
    if (tid < DW) {
        float clo = __builtin_inff(), chi = -__builtin_inff();
#pragma unroll
        for (int q = 0; q < 8; ++q) clo = fminf(clo, s_d[q][tid]), chi = fmaxf(chi, s_d[8 + q][tid]);
        float *cb = cbox + int64_t(blockIdx.x) * CULL_BOX;
        cb[tid] = clo, cb[DW + tid] = chi;
    }
}

}  // namespace tsc
