// prune_batch.hpp -- prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on MANY small ensembles in one launch.
//
// A pass only compares structures inside one chunk of one ensemble (:136-157), its rows are independent (:92, :101-113) and the
// cache is private to a run (:183): one workgroup owns one ensemble ("segment") for its whole pass schedule.  The workgroups of a
// launch share nothing and wait for nothing: no flags, no tickets, any order.
//
// Per segment s with N structures of h heavy atoms:
//   schedule  k over :186-188; a pass runs iff k == 1 or 20 k < active (:192), active counted from the mask at that moment;
//             chunks of N // k structures, the last one runs to N (:136-144);
//   row       the active row i of chunk [f, l) walks the active j in (i, l) in increasing order: a cached key (f, f + (j - i)) -- j - i
//             counts all structures (:65) -- ends the row and keeps it (:66-67); else the first j with rmsd < thr and maxdev < 2 thr
//             (:75) removes row i and appends that key (:76);
//   pass      every row reads the mask and the cache as they were when the pass began; the keys are added after it (:204).
// The cache view of a pass is one bit per structure: bit b is set for a key (a, b) iff a is a chunk start of this pass and b lies in
// that chunk -- then exactly the pairs (i, j) of that chunk with a + (j - i) == b hit it.  It is rebuilt in LDS at the start of every
// pass from the segment's key list (device scratch; a row is removed once, so the list holds at most N keys).
//
// Shape: a wavefront per row, 64 columns per step, lane = column (as k_tfd_first_similar); the cached keys of the step are found
// first and only the columns in front of the first one are evaluated; a ballot finds the first similar column.  Verdicts come from
// the device functions of the single-ensemble path (sieve.hpp: pair_H, rmsd.hpp: pair_verdict, exact_rmsd_maxdev).
#pragma once
#include "rmsd.hpp"
#include "sieve.hpp"

namespace tsc {

constexpr int PB_MAX_N = TSC_PRUNE_BATCH_MAX_N;  // (8192) structures of one segment at most: three bit arrays of it live in LDS (3 KB)
constexpr int PB_WAVES = 4;
constexpr int PB_THREADS = PB_WAVES * 64;
constexpr int PB_WORDS = PB_MAX_N / 64;

struct PbSegment {  // one per workgroup, in launch order
    long long off;   // first double of the segment's [n, h, 3] block in `heavy`
    long long moff;  // first structure of the segment in the batch (mask, squared norms, key list)
    int n, h;
    int seg;         // the segment's index in the caller's arrays (stats, n_passes, nonfinite)
    int pad;
    double thr, maxdev_thr, half_h_thr2, two_thr2;  // pass_plan.hpp: thresholds()
};

__device__ inline bool pb_bit(const unsigned long long *bits, int t) { return (bits[t >> 6] >> (t & 63)) & 1ull; }

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
    const int N = sg.n, h = sg.h, h3 = 3 * sg.h;
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
        const double *x = heavy + (long long)t * h3;
        double g = 0.0;
        for (int a = 0; a < h; ++a) g += x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1] + x[3 * a + 2] * x[3 * a + 2];
        G[t] = g;
        if (!(g < 1.7976931348623157e308)) atomicOr(&s_nonfinite, 1);
    }
    __syncthreads();

    constexpr int KS[18] = {500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1};  // :186-188
    int active = N, n_pass = 0;
    for (int ks = 0; ks < 18 && N > 0; ++ks) {
        const int k = KS[ks];
        if (!(k == 1 || 20ll * k < active)) continue;  // :192
        const int cs = N / k;                            // :136  (>= 20 where k > 1)
        const int keys_before = s_nkeys;
        // ---- the cache view of this pass
        for (int w = tid; w < nw; w += PB_THREADS) s_view[w] = 0ull;
        __syncthreads();
        if (use_cache)
            for (int q = tid; q < keys_before; q += PB_THREADS) {
                const int2 key = keys[q];
                const int c = key.x / cs;
                if (key.x - c * cs != 0 || c >= k) continue;
                const int last = (c == k - 1) ? N : cs * (c + 1);
                if (key.y < last) atomicOr(&s_view[key.y >> 6], 1ull << (key.y & 63));
            }
        __syncthreads();
        // ---- rows, dealt round-robin to the wavefronts (early rows of a chunk have the long ranges)
        unsigned long long ev = 0;
        for (int i = wid; i < N; i += PB_WAVES) {
            if (!pb_bit(s_in, i)) continue;  // :101, :118-119
            const int c = min(i / cs, k - 1);
            const int f = c * cs;                           // :140
            const int l = (c == k - 1) ? N : f + cs;        // :141-144
            const double *__restrict__ p = heavy + (long long)i * h3;
            const double Gi = G[i];
            for (int j0 = i + 1; j0 < l; j0 += 64) {
                const int j = j0 + lane;
                const bool valid = j < l && pb_bit(s_in, j);  // :60
                const unsigned long long vm = __builtin_amdgcn_ballot_w64(valid);
                if (!vm) continue;
                const bool hit = valid && pb_bit(s_view, f + (j - i));  // :65-66 (the view is empty in the cache-free mode)
                const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
                // the columns the sequential scan reaches in this step: the active ones in front of the first cached key
                const unsigned long long em = hm ? (vm & ((1ull << (__ffsll((long long)hm) - 1)) - 1ull)) : vm;
                bool sim = false;
                if ((em >> lane) & 1ull) {
                    const double Gj = G[j];
                    // a structure with a NaN or infinite coordinate is similar to nothing (every comparison of :75 is false)
                    if (Gi + Gj < 1.7976931348623157e308) {
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
                if (sm) {  // :75-77: row i goes, with the key of its first similar column
                    const int ls = __ffsll((long long)sm) - 1;
                    ev += (unsigned long long)__popcll(em & ((2ull << ls) - 1ull));
                    if (lane == 0) {
                        atomicAnd(&s_out[i >> 6], ~(1ull << (i & 63)));
                        keys[atomicAdd(&s_nkeys, 1)] = make_int2(f, f + (j0 + ls - i));
                    }
                    break;
                }
                ev += (unsigned long long)__popcll(em);
                if (hm) break;  // :66-67
            }
        }
        if (lane == 0 && ev) atomicAdd(&s_ev, ev);
        __syncthreads();
        // ---- :204, :196: the keys join the cache, the mask of the next pass
        const int removed = s_nkeys - keys_before;
        if (tid == 0 && stats) {
            tsc_batch_pass_stats &o = stats[(long long)sg.seg * TSC_MAX_PASSES + n_pass];
            o.k = k, o.n_active_before = active, o.n_active_after = active - removed;
            o.pairs_evaluated = (long long)s_ev, o.new_keys = removed;
        }
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
