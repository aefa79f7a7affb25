// prune_team.hpp -- prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on MANY mid-size ensembles per call: a TEAM of workgroups
// per ensemble ("segment") and one set of launches per schedule slot for all segments together.
//
// The semantics are those stated at the top of prune_batch.hpp (schedule, row, pass; mode 1 has no cache), and so is their text: the gate
// and the chunk of a row are those of prune_schedule.hpp, and a row is walked, the cache view built, the squared norms and the non-finite
// rule taken and a pass recorded by the pb_* functions k_prune_batch calls.  The masks are bit for bit those of the other routes.
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
constexpr int PT_WAVES = 4;                     // (PT_ROWS, the rows of a work item, and PT_PER_WORD: prune_batch_plan.hpp)
constexpr int PT_THREADS = PT_WAVES * 64;

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

// (segs: in the caller's order throughout)
inline __global__ __launch_bounds__(PT_THREADS) void k_team_init(PtState st, const PbSegment *__restrict__ segs, int n_segs) {
    const int s = blockIdx.x * PT_THREADS + threadIdx.x;
    if (s >= n_segs) return;
    PtRecord r;
    r.n_keys = r.keys_before = r.n_pass = r.run = r.cs = r.k = r.nonfinite = 0;
    r.active = segs[s].n;
    r.pairs = 0ull;
    st.rec[s] = r;
}

// the mask of :182 as bits, an empty view, and the squared norm of every structure (a sum that is not finite marks a NaN or infinite coordinate)
inline __global__ __launch_bounds__(PT_ROWS) void k_team_prologue(PtState st, const PbSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                                  const double *__restrict__ heavy_all) {
    const int2 it = items[blockIdx.x];
    const PbSegment sg = segs[it.x];
    const int tid = threadIdx.x;
    const int N = sg.n;
    const int r0 = it.y * PT_ROWS;
    if (tid == 0 && it.y % PT_PER_WORD == 0) {  // (the first item of a word writes it)
        const int w = it.y / PT_PER_WORD, rem = N - r0;
        const unsigned long long full = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
        st.in[sg.woff + w] = full, st.out[sg.woff + w] = full, st.view[sg.woff + w] = 0ull;
    }
    const int t = r0 + tid;
    if (t < N) {
        const double g = st.G[sg.moff + t] = pb_sqnorm(heavy_all + sg.off + (long long)t * (3 * sg.h), sg.h);
        if (!pb_finite(g)) atomicOr(&st.rec[it.x].nonfinite, 1);
    }
}

// One workgroup per segment.  Closes the pass the segment had open (:204, :196: the statistics, the mask of the next pass, an empty
// view), then opens slot k (k = 0: none -- the call's last turn, which also writes n_passes and nonfinite): the gate of :192 from the
// segment's own count, and the cache view of the pass from the key list (pb_scatter_view).
inline __global__ __launch_bounds__(PT_THREADS) void k_team_turn(PtState st, const PbSegment *__restrict__ segs, int k, int use_cache,
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
        if (tid == 0 && stats) pb_write_stats(stats, s, r.n_pass, r.k, r.active, removed, r.pairs);
        for (int w = tid; w < nw; w += PT_THREADS) st.in[woff + w] = st.out[woff + w], view[w] = 0ull;
        r.active -= removed, r.n_pass += 1, r.pairs = 0ull, r.run = 0;
    }
    if (k > 0 && N > 0 && pass_gate(k, r.active)) {
        const int cs = N / k;  // :136  (>= 20 where k > 1)
        r.run = 1, r.k = k, r.cs = cs, r.keys_before = r.n_keys;
        if (use_cache && r.n_keys > 0) {
            __syncthreads();  // (the view is empty before the keys of this pass set bits in it)
            pb_scatter_view(st.keys + moff, r.n_keys, N, k, cs, tid, PT_THREADS, view);
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
// 64-bit words straight from the bit arrays, so the ballots of k_prune_batch's step are shifts here.
inline __global__ __launch_bounds__(PT_THREADS) void k_team_rows(PtState st, const PbSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                                 const double *__restrict__ heavy_all) {
    __shared__ unsigned long long s_ev;
    const int2 it = items[blockIdx.x];
    const PtRecord r = st.rec[it.x];
    if (!r.run) return;
    const PbSegment sg = segs[it.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = sg.n;
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
        int f, l;
        chunk_of_row(i, N, r.k, r.cs, f, l);
        const int j = pb_walk_row(sg, heavy, G, i, l, lane, [&](int j0) {
            const int left = l - j0;
            PbStep s{pt_bits(in, nw, j0), 0ull};
            if (left < 64) s.vm &= (1ull << left) - 1ull;
            if (s.vm) s.hm = s.vm & pt_bits(view, nw, f + (j0 - i));  // (the view is empty in the cache-free mode)
            return s;
        }, ev);
        if (j >= 0 && lane == 0) {
            atomicAnd(&st.out[sg.woff + (i >> 6)], ~(1ull << (i & 63)));
            st.keys[sg.moff + atomicAdd(&st.rec[it.x].n_keys, 1)] = make_int2(f, f + (j - i));
        }
    }
    if (lane == 0 && ev) atomicAdd(&s_ev, ev);
    __syncthreads();
    if (tid == 0 && s_ev) atomicAdd(&st.rec[it.x].pairs, s_ev);
}

// the verdicts as bytes: an item writes those of its rows
inline __global__ __launch_bounds__(PT_ROWS) void k_team_finish(PtState st, const PbSegment *__restrict__ segs, const int2 *__restrict__ items,
                                                           uint8_t *__restrict__ mask_all) {
    const int2 it = items[blockIdx.x];
    const long long moff = segs[it.x].moff, woff = segs[it.x].woff;
    const int t = it.y * PT_ROWS + threadIdx.x;
    if (t < segs[it.x].n) mask_all[moff + t] = (st.in[woff + (t >> 6)] >> (t & 63)) & 1ull ? 1 : 0;
}

}  // namespace tsc
