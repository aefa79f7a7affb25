// prune_team.hpp -- prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on MANY mid-size ensembles per call: a TEAM of workgroups
// per ensemble ("segment") and one set of launches per schedule slot for all segments together.
//
// The semantics are those stated at the top of prune_batch.hpp, per segment s with N structures of h heavy atoms:
//   schedule  k over :186-188; a pass runs iff k == 1 or 20 k < active (:192), active counted from the mask at that moment;
//             chunks of N // k structures, the last one runs to N (:136-144);
//   row       the active row i of chunk [f, l) walks the active j in (i, l) in increasing order: a cached key (f, f + (j - i)) ends the
//             row and keeps it (:66-67); else the first j with rmsd < thr and maxdev < 2 thr (:75) removes row i and appends that key (:76);
//   pass      every row reads the mask and the cache as they were when the pass began; the keys are added after it (:204);
//   mode 1    has no cache.
// Verdicts come from the device functions k_prune_batch uses, in its argument order (sieve.hpp: pair_H with p the lower index, rmsd.hpp:
// pair_verdict, exact_rmsd_maxdev), and so does the non-finite rule: the masks are bit for bit those of the other routes.
//
// Where k_prune_batch keeps a segment's state in LDS, this route keeps it in device memory (PtState): three bit arrays per segment -- the
// mask the pass reads, the mask it writes, the cache view -- each segment starting on a 64-bit word of its own with the bits past N zero,
// the squared norms, the key list int2[N] and one record (PtRecord).  All of it is initialised by k_team_init / k_team_prologue: scratch
// is recycled memory.
//
// Launches: k_team_init, k_team_prologue, then per schedule slot that some segment can take by its N alone k_team_turn (a workgroup per
// segment: closes the segment's previous pass, decides the gate of this one from its own `active`, builds the cache view) and
// k_team_rows (a static table of (segment, tile of PT_ROWS rows); the items of a segment whose gate is closed return at once), a last
// k_team_turn that only closes, and k_team_finish.  The count depends on the slot list, never on the number of segments.  The workgroups
// of a launch wait for nothing from one another: what one launch writes the next one reads, and that is all the ordering there is.
#pragma once
#include "prune_batch.hpp"

namespace tsc {

constexpr int PT_MAX_N = TSC_PRUNE_TEAM_MAX_N;  // structures of one segment at most
constexpr int PT_ROWS = 16;                     // rows of a work item: four per wavefront.  A lone ensemble of 4096 structures makes 256
                                                // items of them, 1024 wavefronts; with 64 rows it was one wavefront per compute unit
constexpr int PT_WAVES = 4;
constexpr int PT_THREADS = PT_WAVES * 64;
constexpr int PT_PER_WORD = 64 / PT_ROWS;       // items that share a word of the segment's bit arrays
static_assert(PT_ROWS * PT_PER_WORD == 64 && PT_ROWS <= 64, "the rows of an item lie in one mask word");

struct PtSegment {  // one per segment, in the caller's order
    long long off;   // first double of the segment's [n, h, 3] block in `heavy`
    long long moff;  // first structure of the segment in the batch (mask, squared norms, key list)
    long long woff;  // first 64-bit word of the segment in the bit arrays
    int n, h;
    double thr, maxdev_thr, half_h_thr2, two_thr2;  // pass_plan.hpp: thresholds()
};

struct PtRecord {  // one per segment
    int n_keys;       // keys in the segment's list (one per removed row)
    int keys_before;  // ... when the open pass began
    int active;       // count_nonzero(mask) entering the open pass (:192)
    int n_pass;       // passes closed so far
    int run;          // the open slot's gate: 1 = k_team_rows works on this segment
    int cs, k;        // the open pass: chunk length N // k, chunks
    int nonfinite;
    unsigned long long pairs;  // columns the sequential scan reached in the open pass
};

struct PtState {
    unsigned long long *in, *out, *view;  // [sum of ceil(n / 64)]
    double *G;                            // [sum n]
    int2 *keys;                           // [sum n]
    PtRecord *rec;                        // [S]
};

// 64 bits of a segment's bit array from bit t on (words at nw and beyond read as zero)
__device__ inline unsigned long long pt_bits(const unsigned long long *__restrict__ bits, int nw, int t) {
    const int w = t >> 6, s = t & 63;
    unsigned long long v = w < nw ? bits[w] >> s : 0ull;
    if (s && w + 1 < nw) v |= bits[w + 1] << (64 - s);
    return v;
}

inline __global__ __launch_bounds__(PT_THREADS) void k_team_init(PtState st, const PtSegment *__restrict__ segs, int n_segs) {
    const int s = blockIdx.x * PT_THREADS + threadIdx.x;
    if (s >= n_segs) return;
    PtRecord r;
    r.n_keys = r.keys_before = r.n_pass = r.run = r.cs = r.k = r.nonfinite = 0;
    r.active = segs[s].n;
    r.pairs = 0ull;
    st.rec[s] = r;
}

// the mask of :182 as bits, an empty view, and the squared norm of every structure (a sum that is not finite marks a NaN or infinite coordinate)
inline __global__ __launch_bounds__(PT_ROWS) void k_team_prologue(PtState st, const PtSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                                  const double *__restrict__ heavy_all) {
    const int2 it = items[blockIdx.x];
    const PtSegment sg = segs[it.x];
    const int tid = threadIdx.x;
    const int N = sg.n, h = sg.h, h3 = 3 * sg.h;
    const int r0 = it.y * PT_ROWS;
    if (tid == 0 && it.y % PT_PER_WORD == 0) {  // (the first item of a word writes it)
        const int w = it.y / PT_PER_WORD, rem = N - r0;
        const unsigned long long full = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
        st.in[sg.woff + w] = full, st.out[sg.woff + w] = full, st.view[sg.woff + w] = 0ull;
    }
    const int t = r0 + tid;
    if (t < N) {
        const double *x = heavy_all + sg.off + (long long)t * h3;
        double g = 0.0;
        for (int a = 0; a < h; ++a) g += x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1] + x[3 * a + 2] * x[3 * a + 2];
        st.G[sg.moff + t] = g;
        if (!(g < 1.7976931348623157e308)) atomicOr(&st.rec[it.x].nonfinite, 1);
    }
}

// One workgroup per segment.  Closes the pass the segment had open (:204, :196: the statistics, the mask of the next pass, an empty
// view), then opens slot k (k = 0: none -- the call's last turn, which also writes n_passes and nonfinite): the gate of :192 from the
// segment's own count, and the cache view of the pass from the key list (prune_batch.hpp: key (a, b) sets bit b iff a is a chunk start
// of this pass and b lies in that chunk).
inline __global__ __launch_bounds__(PT_THREADS) void k_team_turn(PtState st, const PtSegment *__restrict__ segs, int k, int use_cache,
                                                                 tsc_batch_pass_stats *__restrict__ stats, int32_t *__restrict__ n_passes,
                                                                 uint8_t *__restrict__ nonfinite) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int N = segs[s].n;
    const long long woff = segs[s].woff, moff = segs[s].moff;
    const int nw = (N + 63) >> 6;
    PtRecord r = st.rec[s];  // (every thread its own copy; thread 0 writes the record back at the end)
    __syncthreads();         // ... which no wavefront may still have to read then
    unsigned long long *__restrict__ view = st.view + woff;
    if (r.run) {
        const int removed = r.n_keys - r.keys_before;
        if (tid == 0 && stats) {
            tsc_batch_pass_stats &o = stats[(long long)s * TSC_MAX_PASSES + r.n_pass];
            o.k = r.k, o.n_active_before = r.active, o.n_active_after = r.active - removed;
            o.pairs_evaluated = (long long)r.pairs, o.new_keys = removed;
        }
        for (int w = tid; w < nw; w += PT_THREADS) st.in[woff + w] = st.out[woff + w], view[w] = 0ull;
        r.active -= removed, r.n_pass += 1, r.pairs = 0ull, r.run = 0;
    }
    if (k > 0 && N > 0 && (k == 1 || 20ll * k < r.active)) {  // :192
        const int cs = N / k;                                  // :136  (>= 20 where k > 1)
        r.run = 1, r.k = k, r.cs = cs, r.keys_before = r.n_keys;
        if (use_cache && r.n_keys > 0) {
            __syncthreads();  // (the view is empty before the keys of this pass set bits in it)
            const int2 *__restrict__ keys = st.keys + moff;
            for (int q = tid; q < r.n_keys; q += PT_THREADS) {
                const int2 key = keys[q];
                const int c = key.x / cs;
                if (key.x - c * cs != 0 || c >= k) continue;
                const int last = (c == k - 1) ? N : cs * (c + 1);
                if (key.y < last) atomicOr(&view[key.y >> 6], 1ull << (key.y & 63));
            }
        }
    }
    if (tid == 0) {
        st.rec[s] = r;
        if (k == 0) {
            if (n_passes) n_passes[s] = r.n_pass;
            if (nonfinite) nonfinite[s] = r.nonfinite ? 1 : 0;
        }
    }
}

// A work item: PT_ROWS consecutive rows of one segment, dealt round-robin to the wavefronts (early rows of a chunk have the long ranges).
// A wavefront per row, 64 columns per step, lane = column, as k_prune_batch; the active columns and the cached keys of a step come as
// 64-bit words straight from the bit arrays, so the ballots of prune_batch.hpp:106-110 are shifts here.
inline __global__ __launch_bounds__(PT_THREADS) void k_team_rows(PtState st, const PtSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                                 const double *__restrict__ heavy_all) {
    __shared__ unsigned long long s_ev;
    const int2 it = items[blockIdx.x];
    const PtRecord r = st.rec[it.x];
    if (!r.run) return;
    const PtSegment sg = segs[it.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = sg.n, h = sg.h, h3 = 3 * sg.h, k = r.k, cs = r.cs;
    const int nw = (N + 63) >> 6;
    const double *__restrict__ heavy = heavy_all + sg.off;
    const double *__restrict__ G = st.G + sg.moff;
    const unsigned long long *__restrict__ in = st.in + sg.woff;
    const unsigned long long *__restrict__ view = st.view + sg.woff;
    if (tid == 0) s_ev = 0ull;
    __syncthreads();

    const int r0 = it.y * PT_ROWS;
    const unsigned rows = unsigned(in[r0 >> 6] >> (r0 & 63)) & ((1u << PT_ROWS) - 1u);  // the item's rows: bits past N are zero
    unsigned long long ev = 0;
    for (int i = r0 + wid; i < r0 + PT_ROWS; i += PT_WAVES) {
        if (!((rows >> (i - r0)) & 1u)) continue;  // :101, :118-119
        const int c = min(i / cs, k - 1);
        const int f = c * cs;                           // :140
        const int l = (c == k - 1) ? N : f + cs;        // :141-144
        const double *__restrict__ p = heavy + (long long)i * h3;
        const double Gi = G[i];
        for (int j0 = i + 1; j0 < l; j0 += 64) {
            const int j = j0 + lane;
            const int left = l - j0;
            unsigned long long vm = pt_bits(in, nw, j0);  // :60
            if (left < 64) vm &= (1ull << left) - 1ull;
            if (!vm) continue;
            const unsigned long long hm = vm & pt_bits(view, nw, f + (j0 - i));  // :65-66 (the view is empty in the cache-free mode)
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
                    atomicAnd(&st.out[sg.woff + (i >> 6)], ~(1ull << (i & 63)));
                    st.keys[sg.moff + atomicAdd(&st.rec[it.x].n_keys, 1)] = make_int2(f, f + (j0 + ls - i));
                }
                break;
            }
            ev += (unsigned long long)__popcll(em);
            if (hm) break;  // :66-67
        }
    }
    if (lane == 0 && ev) atomicAdd(&s_ev, ev);
    __syncthreads();
    if (tid == 0 && s_ev) atomicAdd(&st.rec[it.x].pairs, s_ev);
}

// the verdicts as bytes: an item writes those of its rows
inline __global__ __launch_bounds__(PT_ROWS) void k_team_finish(PtState st, const PtSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                           uint8_t *__restrict__ mask_all) {
    const int2 it = items[blockIdx.x];
    const long long moff = segs[it.x].moff, woff = segs[it.x].woff;
    const int t = it.y * PT_ROWS + threadIdx.x;
    if (t < segs[it.x].n) mask_all[moff + t] = (st.in[woff + (t >> 6)] >> (t & 63)) & 1ull ? 1 : 0;
}

}  // namespace tsc
