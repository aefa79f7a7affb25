// prune_batch.hpp -- prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on MANY small ensembles in one launch, and the statement of a
// pass that the team route (prune_team.hpp) shares with it: the pb_* device functions below.
//
// A pass only compares structures inside one chunk of one ensemble (:136-157), its rows are independent (:92, :101-113) and the
// cache is private to a run (:183): one workgroup owns one ensemble ("segment") for its whole pass schedule.  The workgroups of a
// launch share nothing and wait for nothing: no flags, no tickets, any order.
//
// Per segment s with N structures of h heavy atoms:
//   schedule  k over :186-188; a pass runs iff k == 1 or 20 k < active (:192), active counted from the mask at that moment;
//             chunks of N // k structures, the last one runs to N (:136-144) -- prune_schedule.hpp;
//   row       the active row i of chunk [f, l) walks the active j in (i, l) in increasing order: a cached key (f, f + (j - i)) -- j - i
//             counts all structures (:65) -- ends the row and keeps it (:66-67); else the first j with rmsd < thr and maxdev < 2 thr
//             (:75) removes row i and appends that key (:76) -- pb_walk_row;
//   pass      every row reads the mask and the cache as they were when the pass began; the keys are added after it (:204).
// The cache view of a pass is one bit per structure: bit b is set for a key (a, b) iff a is a chunk start of this pass and b lies in
// that chunk -- then exactly the pairs (i, j) of that chunk with a + (j - i) == b hit it (pb_scatter_view).  It is rebuilt in LDS at the
// start of every pass from the segment's key list (device scratch; a row is removed once, so the list holds at most N keys).
//
// Shape: a wavefront per row, 64 columns per step, lane = column (as k_tfd_first_similar); the cached keys of the step are found
// first and only the columns in front of the first one are evaluated; a ballot finds the first similar column.  Verdicts come from
// the device functions of the single-ensemble path (pair_stages.hpp: pair_H, pair_math.hpp: pair_verdict, exact_rmsd_maxdev).
#pragma once
#include "prune_batch_plan.hpp"
#include "pair_math.hpp"
#include "pair_stages.hpp"

namespace tsc {

constexpr int PB_MAX_N = TSC_PRUNE_BATCH_MAX_N;  // (8192) structures of one segment at most: three bit arrays of it live in LDS (3 KB)
constexpr int PB_WAVES = 4;
constexpr int PB_THREADS = PB_WAVES * 64;
constexpr int PB_WORDS = PB_MAX_N / 64;

__device__ inline bool pb_bit(const unsigned long long *bits, int t) { return (bits[t >> 6] >> (t & 63)) & 1ull; }

// false for a NaN, an infinity and a sum that overflowed: what a squared norm, or the sum of two, is when a coordinate is not finite
__device__ inline bool pb_finite(double g) { return g < 1.7976931348623157e308; }

// the squared norm of a structure's h heavy atoms
__device__ inline double pb_sqnorm(const double *x, int h) {
    double g = 0.0;
    for (int a = 0; a < h; ++a) g += x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1] + x[3 * a + 2] * x[3 * a + 2];
    return g;
}

// The cache view of a pass of k chunks of cs structures: key (a, b) sets bit b iff a is a chunk start of this pass and b lies in that
// chunk.  Thread `tid` of `stride`; `view` (LDS or device memory) is empty and visible to all of them before the call.
__device__ inline void pb_scatter_view(const int2 *__restrict__ keys, int n_keys, int N, int k, int cs, int tid, int stride, unsigned long long *view) {
    for (int q = tid; q < n_keys; q += stride) {
        const int2 key = keys[q];
        const int c = key.x / cs;
        if (key.x - c * cs != 0 || c >= k) continue;
        const int last = (c == k - 1) ? N : cs * (c + 1);
        if (key.y < last) atomicOr(&view[key.y >> 6], 1ull << (key.y & 63));
    }
}

// the record of a pass that ran (:204, :196); `pairs`: the columns the sequential scan reached in it
__device__ inline void pb_write_stats(tsc_batch_pass_stats *__restrict__ stats, int seg, int n_pass, int k, int active, int removed, unsigned long long pairs) {
    tsc_batch_pass_stats &o = stats[(long long)seg * TSC_MAX_PASSES + n_pass];
    o.k = k, o.n_active_before = active, o.n_active_after = active - removed;
    o.pairs_evaluated = (long long)pairs, o.new_keys = removed;
}

struct PbStep {
    unsigned long long vm, hm;  // of the 64 columns from j0 on: the active ones below l (:60); of those, the ones a cached key ends the row at (:65-66)
};

// One wavefront walks the active row i of chunk [f, l) (the caller has checked :101, :118-119), 64 columns per step, lane = column.
// step(j0) gives the PbStep of the columns j0 .. j0 + 63, the same in every lane (hm is not read where vm is 0; it is 0 in the cache-free
// mode).  Returns the first similar column -- row i goes, with the key (f, f + (j - i)), :75-77 -- or -1: the row stays.  `pairs` grows by
// the columns the sequential scan reached.  heavy, G: the segment's structures and their squared norms.
template <typename Step>
__device__ inline int pb_walk_row(const PbSegment &sg, const double *__restrict__ heavy, const double *__restrict__ G, int i, int l, int lane, Step &&step,
                                  unsigned long long &pairs) {
    const int h = sg.h, h3 = 3 * sg.h;
    const double *__restrict__ p = heavy + (long long)i * h3;
    const double Gi = G[i];
    int found = -1;
    for (int j0 = i + 1; j0 < l; j0 += 64) {
        const int j = j0 + lane;
        const PbStep s = step(j0);
        if (!s.vm) continue;
        // the columns the sequential scan reaches in this step: the active ones in front of the first cached key
        const unsigned long long em = s.hm ? (s.vm & ((1ull << (__ffsll((long long)s.hm) - 1)) - 1ull)) : s.vm;
        bool sim = false;
        if ((em >> lane) & 1ull) {
            const double Gj = G[j];
            // a structure with a NaN or infinite coordinate is similar to nothing (every comparison of :75 is false)
            if (pb_finite(Gi + Gj)) {
                const double *__restrict__ q = heavy + (long long)j * h3;
                double H[9];
                pair_H(p, q, h, 0, 1, H);  // :15, p the lower index
                const int verdict = pair_verdict(H, 0.5 * (Gi + Gj), sg.half_h_thr2, sg.two_thr2, h);
                if (verdict == PAIR_UNDECIDED) {
                    double rm, md;
                    exact_rmsd_maxdev(p, q, h, H, Gi, Gj, rm, md);
                    sim = rm < sg.thr && md < sg.maxdev_thr;  // :75
                } else {
                    sim = verdict == PAIR_SIMILAR;
                }
            }
        }
        const unsigned long long sm = __builtin_amdgcn_ballot_w64(sim);
        if (sm) {
            const int ls = __ffsll((long long)sm) - 1;
            pairs += (unsigned long long)__popcll(em & ((2ull << ls) - 1ull));
            found = j0 + ls;
            break;
        }
        pairs += (unsigned long long)__popcll(em);
        if (s.hm) break;  // :66-67
    }
    return found;
}

// segs: one per workgroup, in launch order
inline __global__ __launch_bounds__(PB_THREADS) void k_prune_batch(const PbSegment *__restrict__ segs, const double *__restrict__ heavy_all, int use_cache,
                                                                   double *__restrict__ G_all, int2 *__restrict__ keys_all, uint8_t *__restrict__ mask_all,
                                                                   tsc_batch_pass_stats *__restrict__ stats, int32_t *__restrict__ n_passes,
                                                                   uint8_t *__restrict__ nonfinite) {
    __shared__ unsigned long long s_in[PB_WORDS], s_out[PB_WORDS], s_view[PB_WORDS];
    __shared__ unsigned long long s_ev;
    __shared__ int s_nkeys, s_nonfinite;

    const PbSegment sg = segs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = sg.n, h3 = 3 * sg.h;
    const double *__restrict__ heavy = heavy_all + sg.off;
    double *__restrict__ G = G_all + sg.moff;
    int2 *__restrict__ keys = keys_all + sg.moff;
    const int nw = (N + 63) >> 6;

    // the mask of :182 as bits, and the squared norm of every structure (a sum that is not finite marks a NaN or infinite coordinate)
    for (int w = tid; w < nw; w += PB_THREADS) {
        const int rem = N - 64 * w;
        s_in[w] = s_out[w] = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    }
    if (tid == 0) s_ev = 0, s_nkeys = 0, s_nonfinite = 0;
    __syncthreads();
    for (int t = tid; t < N; t += PB_THREADS) {
        const double g = G[t] = pb_sqnorm(heavy + (long long)t * h3, sg.h);
        if (!pb_finite(g)) atomicOr(&s_nonfinite, 1);
    }
    __syncthreads();

    int active = N, n_pass = 0;
    for (int ks = 0; ks < TSC_MAX_PASSES && N > 0; ++ks) {
        const int k = KS[ks];
        if (!pass_gate(k, active)) continue;
        const int cs = N / k;  // :136  (>= 20 where k > 1)
        const int keys_before = s_nkeys;
        // ---- the cache view of this pass
        for (int w = tid; w < nw; w += PB_THREADS) s_view[w] = 0ull;
        __syncthreads();
        if (use_cache) pb_scatter_view(keys, keys_before, N, k, cs, tid, PB_THREADS, s_view);
        __syncthreads();
        // ---- rows, dealt round-robin to the wavefronts (early rows of a chunk have the long ranges)
        unsigned long long ev = 0;
        for (int i = wid; i < N; i += PB_WAVES) {
            if (!pb_bit(s_in, i)) continue;  // :101, :118-119
            int f, l;
            chunk_of_row(i, N, k, cs, f, l);
            const int j = pb_walk_row(sg, heavy, G, i, l, lane, [&](int j0) {
                const int jl = j0 + lane;
                const bool valid = jl < l && pb_bit(s_in, jl);
                PbStep s{__builtin_amdgcn_ballot_w64(valid), 0ull};
                if (s.vm) s.hm = __builtin_amdgcn_ballot_w64(valid && pb_bit(s_view, f + (jl - i)));  // (the view is empty in the cache-free mode)
                return s;
            }, ev);
            if (j >= 0 && lane == 0) {
                atomicAnd(&s_out[i >> 6], ~(1ull << (i & 63)));
                keys[atomicAdd(&s_nkeys, 1)] = make_int2(f, f + (j - i));
            }
        }
        if (lane == 0 && ev) atomicAdd(&s_ev, ev);
        __syncthreads();
        // ---- :204, :196: the keys join the cache, the mask of the next pass
        const int removed = s_nkeys - keys_before;
        if (tid == 0 && stats) pb_write_stats(stats, sg.seg, n_pass, k, active, removed, s_ev);
        for (int w = tid; w < nw; w += PB_THREADS) s_in[w] = s_out[w];
        __syncthreads();
        if (tid == 0) s_ev = 0;
        active -= removed;
        ++n_pass;
    }
    for (int t = tid; t < N; t += PB_THREADS) mask_all[sg.moff + t] = pb_bit(s_in, t) ? 1 : 0;
    if (tid == 0) {
        if (n_passes) n_passes[sg.seg] = n_pass;
        if (nonfinite) nonfinite[sg.seg] = s_nonfinite ? 1 : 0;
    }
}

}  // namespace tsc
