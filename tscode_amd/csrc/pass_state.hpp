// pass_state.hpp -- the state of a run of prune_conformers_rmsd on the device and the device functions that step it: the counters, state
// blocks, records and tickets of a pass, the cache views, closing one pass and opening the next (pass_step_wave, pass_derive), the geometry
// of a pass (PassGeom, chunk_of) and applying the verdicts of a wavefront's rows (apply_wave_rows).  No kernel: every pair kernel includes
// this (a pass can be closed by whichever kernel finishes it); the kernels made of nothing else are in rmsd.hpp.
#pragma once
#include "common.hpp"

namespace tsc {

// Statistics counters of a pass (one set per schedule slot).  Thousands of wavefronts report at the end of a kernel; same-address atomics
// serialise at ~12 ns each (MI355X_MICROARCH.md, "fanin"), which for 10^4 reports is longer than the kernels
// themselves, so the counters are spread over 64 buckets on separate 128-byte lines and summed on the host.
constexpr int CNT_BUCKETS = 64;
enum { CNT_FORMED = 0, CNT_EXACT = 1, CNT_SCREENED = 2, CNT_EVALUATED = 3, CNT_REMOVED = 4, CNT_WALK = 5 /* pairs inside the rows' ranges (k_open_rows, for k_cull_decide) */,
       CNT_KNOWN = 6 /* pairs of the rows' ranges that the pair kernel leaves out: found dissimilar by an earlier pass (k_open_rows, known[]) */, CNT_WORDS = 16 };
struct PassCounters {
    unsigned long long w[CNT_BUCKETS][CNT_WORDS];
};
__device__ inline void count_add(PassCounters *c, unsigned bucket, int what, unsigned long long v) {
    if (v) atomicAdd(&c->w[bucket & (CNT_BUCKETS - 1)][what], v);
}

// Device-resident control block of a prune run, one per schedule slot: written by whoever opens the slot's pass, read by its kernels, so
// that nothing a pass reads changes while it is in flight.  The host enqueues every pass that COULD run (20 k < N) without
// waiting for counts; the kernel that closes a pass evaluates the reference's gate `k == 1 or 20*k < count_nonzero(mask)`
// (rmsd_pruning.py:192) for the next one on the device, and the kernels of a pass that is gated off return immediately.
struct PruneState {
    int n_active;  // count_nonzero(mask) after the last finished pass
    int pass_on;   // gate of the pass in flight
    int A;         // active structures entering the pass in flight (== n_active at its start)
    unsigned ticket;  // blocks of k_apply_pass that have finished (the last one closes the pass)
    int bitsel;    // which of the two bit copies of the mask the pass in flight READS (it clears the rows it removes in the other)
    int cull_on;   // a pass that MAY be culled (cull.hpp): 1 = the sorted layout + bounding boxes run it, 0 = the ordered walk does
                   // (k_cull_decide, from the rows' ranges: a cache that ends most rows early leaves the walk little to do)
    int row_lo;    // rank-partitioned pass (tsc_prune_pass_range): active rank of this rank's local row 0; 0 in every other pass.
                   // In such a pass A counts only the active structures of this rank's chunks and act / cend / best / Dc are
                   // indexed by LOCAL row (global active rank - row_lo): the pair kernel sees an ensemble of A rows
};
struct PassRecord {  // one per schedule slot, read back once at the end of the run
    long long k, n_before, n_after, formed, exact, screened, evaluated, removed;
    long long known;  // of `screened`: pairs the pair kernel did not look at again (CNT_KNOWN)
    int on, algo;
};

// "Every unit of this pass has finished": two-level arrival counter (same-address atomics serialise at ~12 ns each, so
// thousands of arrivals go to PT_GROUPS counters on separate 128-byte lines and only the last of a group to the top).
constexpr int PT_GROUPS = 64;
struct PassTickets {  // zeroed by k_init_run and again by the wavefront that closes a pass
    unsigned group[PT_GROUPS][32];
    unsigned top;
    unsigned pad[31];
};
// one lane calls this for unit `unit` of `n_units`; true for the arrival that completes the pass
__device__ inline bool tickets_arrive(PassTickets *tk, unsigned unit, unsigned n_units, unsigned n_groups) {
    const unsigned grp = unit % n_groups;
    const unsigned in_group = (n_units - grp + n_groups - 1) / n_groups;
    if (atomicAdd(&tk->group[grp][0], 1u) != in_group - 1) return false;
    const unsigned groups = n_units < n_groups ? n_units : n_groups;
    return atomicAdd(&tk->top, 1u) == groups - 1;
}

// The similarity cache of the reference (rmsd_pruning.py:65-76, :204) as one bitmap PER FUTURE PASS.  A row removed in a
// pass leaves the key (a, b) = (first, first + (j - i)); a later pass hits that key only where `a` is the start of one of
// ITS chunks and `b` lies inside that chunk -- and then exactly for the pairs with first + (j - i) == b.  The schedule of
// a run is known when it starts, so the kernel that removes a row sets bit b in the view of every later pass the key
// applies to (a handful of integer divisions per removed row; few keys apply anywhere) and no pass has to walk the key
// list before it can start.  Behind the n-bit view of a pass sits its summary, one bit per 1024 view bits: the stop-column
// search walks only non-empty blocks.
constexpr int MAX_SLOTS = 18;
struct ViewPass {  // one view's pass: k chunks of cs = n // k structures; a / cs == (a * magic) >> shift for every a < 2^31
    int k, cs;
    unsigned magic;
    int shift;
};
struct CacheViews {
    unsigned long long *views;  // [count][stride] words
    long long stride;           // words per view: bit_words + summary words
    int bit_words;
    int n;                      // structures of the run
    int first, count;           // views first .. count - 1 belong to the passes after the one in flight
    const ViewPass *pass;       // [count]
};
// Division by an invariant: m = floor(2^(31+L) / d) + 1 with L = ceil(log2 d) divides every 31-bit dividend exactly
// (Granlund & Montgomery 1994, theorem 4.2 with N = 31); m < 2^32.
inline ViewPass view_pass(int n, int k) {
    ViewPass v;
    v.k = k, v.cs = n / k;
    int L = 0;
    while ((1ll << L) < (long long)v.cs) ++L;
    v.magic = unsigned(((1ull << (31 + L)) / (unsigned long long)v.cs) + 1ull);
    v.shift = 31 + L;
    return v;
}
// A whole wavefront calls this with one removed row per lane (or none): key (a, b) of lane `removed`.  The loop over the later
// passes is wave-uniform (their parameters come by scalar loads); the summary words, which every key of a chunk shares, take
// one atomic per wavefront and word instead of one per key (same-address atomics serialise at ~12 ns each).
__device__ inline void views_insert_wave(const CacheViews &cv, bool removed, int a, int b) {
    if (__ballot(removed) == 0) return;
    const int lane = threadIdx.x & 63;
    for (int j = cv.first; j < cv.count; ++j) {
        const ViewPass vp = cv.pass[j];
        bool ok = false;
        if (removed) {
            const int c = int(((unsigned long long)unsigned(a) * vp.magic) >> vp.shift);
            if (c * vp.cs == a && c < vp.k) ok = b < ((c == vp.k - 1) ? cv.n : vp.cs * (c + 1));
        }
        unsigned long long left = __ballot(ok);
        if (!left) continue;
        unsigned long long *v = cv.views + int64_t(j) * cv.stride;
        if (ok) atomicOr(&v[b >> 6], 1ull << (b & 63));
        while (left) {
            const int leader = __ffsll((long long)left) - 1;
            const int word = __shfl(b >> 16, leader);
            const bool same = ok && (b >> 16) == word;
            unsigned long long sb = same ? 1ull << ((b >> 10) & 63) : 0ull;
            for (int off = 32; off > 0; off >>= 1) sb |= __shfl_xor(sb, off);
            if (lane == leader) {
                unsigned long long *ds = v + cv.bit_words + word;
                if ((__hip_atomic_load(ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & sb) != sb) atomicOr(ds, sb);
            }
            left &= ~__ballot(same);
        }
    }
}

// Closes the pass in slot `prev` (sums its counters, updates n_active, re-ranks the scan blocks, flips the bit copy) and
// opens the pass in slot `cur` (gate, A: the state block of that slot; its counters were zeroed by k_init_run).  prev / cur = -1: nothing to close / open.  Runs in ONE
// WAVEFRONT: of the last unit of the closing pass to finish -- a row tile of the pair kernel, a block of k_apply_pass or of
// k_pass_chunks -- or, where no pass precedes, of k_pass_step.
struct StepArgs {
    int prev, cur;
    long long k_cur;
    int algo_cur;
    int prev_algo;  // >= 0: the kernel that really ran the closing pass (recorded in its PassRecord), -1: as opened
};
struct StepCtx {
    PruneState *st;       // state block of the slot being closed (StepArgs::prev; of the slot being opened where there is none)
    PruneState *st_next;  // state block of the slot being opened (StepArgs::cur), null where there is none
    PassCounters *cnt;    // counters of the slot being closed
    PassRecord *rec;
    int32_t *bsum, *boff;
    int n_blocks;
    unsigned *tickets;  // every arrival counter of the run (PassTickets and the chunk-local kernel's: one per 128-byte line), zeroed on the way out
    int ticket_lines;
    unsigned long long *exch_tail;  // rank-partitioned pass only (else null): the last unit of this rank's share does not close the
                                    // pass -- it leaves this rank's five statistics here, behind the removed-row bits of the exchange
                                    // buffer, and k_pass_merge closes the pass after the ranks' buffers have been summed
};

__device__ inline void pass_step_wave(const StepCtx &sc, const StepArgs &sa) {
    PruneState *st = sc.st;
    const int lane = threadIdx.x & 63;
    static_assert(CNT_BUCKETS == 64 && CNT_REMOVED == 4, "one bucket per lane, five statistics");
    // the buckets and block counts were written by other CUs' atomics: read at the L2, not through this CU's cache.  All
    // loads of the step are issued before the first is used (one memory round trip, not seven)
    const int pass_on = st->pass_on, n_before = st->n_active, bitsel = st->bitsel;
    unsigned long long v0 = __hip_atomic_load(&sc.cnt->w[lane][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long v1 = __hip_atomic_load(&sc.cnt->w[lane][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long v2 = __hip_atomic_load(&sc.cnt->w[lane][2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long v3 = __hip_atomic_load(&sc.cnt->w[lane][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long v4 = __hip_atomic_load(&sc.cnt->w[lane][4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long kn = __hip_atomic_load(&sc.cnt->w[lane][CNT_KNOWN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int c_first = lane < sc.n_blocks ? __hip_atomic_load(&sc.bsum[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const bool closing = sa.prev >= 0 && pass_on != 0;
    unsigned long long sum[CNT_REMOVED + 1] = {v0, v1, v2, v3, v4};
    if (sc.exch_tail) {  // this rank's share of a rank-partitioned pass is done: statistics into the exchange buffer
#pragma unroll
        for (int w = 0; w <= CNT_REMOVED; ++w)
            for (int off = 32; off > 0; off >>= 1) sum[w] += __shfl_xor(sum[w], off);
        if (lane == 0 && pass_on != 0) {
#pragma unroll
            for (int w = 0; w <= CNT_REMOVED; ++w) sc.exch_tail[w] = sum[w];
        }
        for (int e = lane; e < sc.ticket_lines; e += 64) sc.tickets[32 * e] = 0;
        return;
    }
    if (closing) {
#pragma unroll
        for (int w = 0; w <= CNT_REMOVED; ++w)
            for (int off = 32; off > 0; off >>= 1) sum[w] += __shfl_xor(sum[w], off);
        for (int off = 32; off > 0; off >>= 1) kn += __shfl_xor(kn, off);
    }
    if (sa.prev >= 0) {
        // (also behind a pass that was gated off: a chunk-local pass further back that was left open removed rows and wrote no prefix)
        int run = 0;
        for (int b0 = 0; b0 < sc.n_blocks; b0 += 64) {
            const int b = b0 + lane;
            const int c = b0 == 0 ? c_first : (b < sc.n_blocks ? __hip_atomic_load(&sc.bsum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
            int incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (b < sc.n_blocks) sc.boff[b] = run + incl - c;
            run += __shfl(incl, 63);
        }
        if (lane == 0) sc.boff[sc.n_blocks] = run;
    }
    if (lane == 0) {
        int n_active = n_before, sel = bitsel;
        if (closing) {
            PassRecord &r = sc.rec[sa.prev];
            r.formed = (long long)sum[CNT_FORMED], r.exact = (long long)sum[CNT_EXACT], r.screened = (long long)sum[CNT_SCREENED];
            r.evaluated = (long long)sum[CNT_EVALUATED], r.removed = (long long)sum[CNT_REMOVED];
            r.screened += (long long)kn, r.known = (long long)kn;  // (the known prefix counts as inside the rows' ranges: looked at by an earlier pass)
            n_active -= int(sum[CNT_REMOVED]);
            r.n_after = n_active;
            if (sa.prev_algo >= 0) r.algo = sa.prev_algo;
            sel ^= 1;  // the copy the closing pass cleared its removed rows in is the current one now
        }
        int on = 0;
        if (sa.cur >= 0) {
            on = (sa.k_cur == 1 || 20 * sa.k_cur < (long long)n_active) ? 1 : 0;  // rmsd_pruning.py:192
            PassRecord &r = sc.rec[sa.cur];
            r.k = sa.k_cur, r.n_before = n_active, r.n_after = n_active, r.on = on, r.algo = sa.algo_cur;
            r.formed = r.exact = r.screened = r.evaluated = r.removed = r.known = 0;
        }
        // (the state block of the next slot is written whole: nothing of the closing slot's is touched, so a wavefront of the closing
        // pass that is still on its way reads what its siblings read)
        if (PruneState *sn = sc.st_next)
            sn->n_active = n_active, sn->A = n_active, sn->bitsel = sel, sn->row_lo = 0, sn->pass_on = on, sn->ticket = 0, sn->cull_on = 0;
    }
    // the counters belong to their slot and stay; the arrival counters are shared: the first word of every 128-byte line back to zero
    for (int e = lane; e < sc.ticket_lines; e += 64) sc.tickets[32 * e] = 0;
}

// The same step without a closing wavefront: the pass in slot `prev` was LEFT OPEN by its last kernel (its tails end after they have
// applied their rows and added to their counters), and the kernel boundary behind it makes its counters and the scan blocks' counts
// final.  The first kernel of the pass in slot `cur` -- k_open_rows, k_pass_chunks -- derives what pass_step_wave would have written, in
// every workgroup for itself, in the round trip it spends on the state block anyway; workgroup 0 also writes it down (state block of
// `cur`, the records of both slots, the prefix of the scan blocks) for the kernels behind the next kernel boundary.  No workgroup reads
// what workgroup 0 writes in the same launch.  prev_st = null: nothing to derive, the state block of `cur` has been written already.
struct DeriveArgs {
    const PruneState *prev_st;
    const PassCounters *prev_cnt;
    PassRecord *rec;
    int prev, cur;
    long long k_cur;
    int algo_cur, prev_algo;  // (as in StepArgs)
};
struct Derived {
    int n_active, pass_on, bitsel;
};
// One wavefront calls this.  bsum (optional): the scan blocks' counts, whose exclusive prefix goes to s_boff[0 .. n_blocks] (LDS) and,
// from the writer, to boff.  st_cur: written by the writer only.
__device__ inline Derived pass_derive(const DeriveArgs &d, PruneState *st_cur, bool writer, const int32_t *bsum, int n_blocks, int *s_boff, int32_t *boff) {
    const int lane = threadIdx.x & 63;
    const PruneState *sp = d.prev_st;
    // one round trip: the state block, the removed-row buckets (all five statistics in the writer) and the first 64 block counts
    const int prev_on = sp->pass_on, n_before = sp->n_active, sel_before = sp->bitsel;
    unsigned long long sum[CNT_REMOVED + 1] = {0ull, 0ull, 0ull, 0ull, 0ull};
    sum[CNT_REMOVED] = __hip_atomic_load(&d.prev_cnt->w[lane][CNT_REMOVED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (writer) {
#pragma unroll
        for (int w = 0; w < CNT_REMOVED; ++w) sum[w] = __hip_atomic_load(&d.prev_cnt->w[lane][w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long kn = writer ? __hip_atomic_load(&d.prev_cnt->w[lane][CNT_KNOWN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    const int c_first = (bsum && lane < n_blocks) ? __hip_atomic_load(&bsum[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    for (int off = 32; off > 0; off >>= 1) sum[CNT_REMOVED] += __shfl_xor(sum[CNT_REMOVED], off);
    if (writer) {
#pragma unroll
        for (int w = 0; w < CNT_REMOVED; ++w)
            for (int off = 32; off > 0; off >>= 1) sum[w] += __shfl_xor(sum[w], off);
        for (int off = 32; off > 0; off >>= 1) kn += __shfl_xor(kn, off);
    }
    if (bsum) {
        int run = 0;
        for (int b0 = 0; b0 < n_blocks; b0 += 64) {
            const int b = b0 + lane;
            const int c = b0 == 0 ? c_first : (b < n_blocks ? __hip_atomic_load(&bsum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
            int incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (b < n_blocks) {
                s_boff[b] = run + incl - c;
                if (writer) boff[b] = run + incl - c;
            }
            run += __shfl(incl, 63);
        }
        if (lane == 0) {
            s_boff[n_blocks] = run;
            if (writer) boff[n_blocks] = run;
        }
    }
    Derived out;
    const bool closing = prev_on != 0;
    out.n_active = closing ? n_before - int(sum[CNT_REMOVED]) : n_before;
    out.bitsel = closing ? sel_before ^ 1 : sel_before;  // (a pass that was gated off hands both on unchanged)
    out.pass_on = (d.k_cur == 1 || 20 * d.k_cur < (long long)out.n_active) ? 1 : 0;  // rmsd_pruning.py:192
    if (writer && lane == 0) {
        if (closing) {
            PassRecord &r = d.rec[d.prev];
            r.formed = (long long)sum[CNT_FORMED], r.exact = (long long)sum[CNT_EXACT], r.screened = (long long)sum[CNT_SCREENED];
            r.evaluated = (long long)sum[CNT_EVALUATED], r.removed = (long long)sum[CNT_REMOVED];
            r.screened += (long long)kn, r.known = (long long)kn;
            r.n_after = out.n_active;
            if (d.prev_algo >= 0) r.algo = d.prev_algo;
        }
        PassRecord &r = d.rec[d.cur];
        r.k = d.k_cur, r.n_before = out.n_active, r.n_after = out.n_active, r.on = out.pass_on, r.algo = d.algo_cur;
        r.formed = r.exact = r.screened = r.evaluated = r.removed = r.known = 0;
        st_cur->n_active = out.n_active, st_cur->A = out.n_active, st_cur->bitsel = out.bitsel, st_cur->row_lo = 0, st_cur->pass_on = out.pass_on;
        st_cur->ticket = 0, st_cur->cull_on = 0;
    }
    return out;
}

struct PassGeom {
    int n;   // structures (< 2^31)
    int k;   // chunks in this pass
    int cs;  // chunk size n // k (rmsd_pruning.py:136)
};

__device__ inline void chunk_of(const PassGeom &g, int64_t i, int64_t &first, int64_t &last) {
    int c = int(i) / g.cs;  // 32-bit division: n < 2^31
    if (c >= g.k) c = g.k - 1;
    first = int64_t(c) * g.cs;                        // :140
    last = (c == g.k - 1) ? g.n : first + g.cs;       // :141-144
}

__device__ inline unsigned long long extract64(const unsigned long long *__restrict__ bits, int64_t start) {
    int64_t w = start >> 6;
    int sh = int(start & 63);
    unsigned long long lo = bits[w] >> sh;
    unsigned long long hi = sh ? (bits[w + 1] << (64 - sh)) : 0ull;
    return lo | hi;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int SCAN_BLOCK_WORDS = 32;  // a scan block (scan.hpp: SCAN_TILE = 2048 structures) as 64-bit words of the mask's bit copy
constexpr int DESC_WORDS = 16;        // floats per descriptor (descriptor.hpp: DW)

// position of the k-th (0-based) set bit of w (k < popcount(w))
__device__ inline int select64(unsigned long long w, int k) {
    int p = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int c = __popcll((w >> p) & ((1ull << s) - 1ull));
        if (k >= c) k -= c, p += s;
    }
    return p;
}

// The verdicts of up to 64 rows of a finished pass, one row per lane (a whole wavefront calls this): rows with a similar
// column are removed (:113) -- mask byte, the bit in the copy the NEXT pass reads, the count of their scan block -- and
// leave one cache key each (:76, appended after the pass at :204), entered into the views of the later passes; counts what
// the reference's sequential scan would have evaluated.  best[] was written by other CUs' atomics: read at the L2.
struct ApplyArgs {
    PassGeom g;
    const int32_t *act, *cend;
    const int32_t *best;
    uint8_t *mask;
    unsigned long long *bits;
    int bit_words;
    int32_t *bsum;
    int block_items;
    CacheViews cv;
    unsigned long long *exch;  // rank-partitioned pass (else null): removed rows are only NOTED here, one bit each; mask, bit copy and
                               // block counts follow in k_pass_merge, from the sum of every rank's notes
};
__device__ inline void apply_wave_rows(const ApplyArgs &a, int sel, int r, bool valid, unsigned long long &ev_total, unsigned long long &rm_total) {
    const int lane = threadIdx.x & 63;
    unsigned long long ev = 0;
    bool removed = false;
    int my_block = -1;
    int64_t first = 0, delta = 0;
    if (valid) {
        const int b = __hip_atomic_load(&a.best[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b != INT_MAX) {
            const int64_t i = a.act[r], j = a.act[b];
            int64_t last;
            chunk_of(a.g, i, first, last);
            if (a.exch) {
                atomicOr(&a.exch[i >> 6], 1ull << (i & 63));
            } else {
                a.mask[i] = 0;
                atomicAnd(&a.bits[size_t(sel ^ 1) * a.bit_words + (i >> 6)], ~(1ull << (i & 63)));
                my_block = int(i / a.block_items);
            }
            delta = j - i;
            removed = true;
            ev = (unsigned long long)(b - r);  // columns r+1 .. b were evaluated
        } else {
            ev = (unsigned long long)(a.cend[r] - r - 1);  // every active column before the stop column
        }
    }
    // the per-block counts follow the mask: one atomic per (wavefront, scan block) -- the removed rows of a wavefront fall
    // into one or two blocks, and thousands of single decrements of two cache lines would serialise
    for (unsigned long long left = __ballot(removed && my_block >= 0); left;) {
        const int l = __ffsll((long long)left) - 1;
        const int blk = __shfl(my_block, l);
        const unsigned long long same = __ballot(removed && my_block == blk);
        if (lane == l) atomicSub(&a.bsum[blk], __popcll(same));
        left &= ~same;
    }
    views_insert_wave(a.cv, removed, int(first), int(first + delta));
    const int n_rm = __popcll(__ballot(removed));
    for (int off = 32; off > 0; off >>= 1) ev += __shfl_down(ev, off);
    ev_total += ev, rm_total += (unsigned long long)n_rm;
}

// Active structures before position pos (0 <= pos <= n) in the bit copy X: the prefix of its scan block + the set bits of
// the block below it.  One wavefront calls this.
__device__ inline int rank_below_wave(const int32_t *__restrict__ boff, const unsigned long long *__restrict__ X, int n_blocks, int n_active, int64_t pos) {
    const int lane = threadIdx.x & 63;
    const int bf = int(pos / (64 * SCAN_BLOCK_WORDS)), off = int(pos - int64_t(bf) * (64 * SCAN_BLOCK_WORDS));
    int cnt = 0;
    if (bf < n_blocks && lane < SCAN_BLOCK_WORDS) {
        const int below = off - 64 * lane;
        const unsigned long long m = below >= 64 ? ~0ull : (below > 0 ? (1ull << below) - 1ull : 0ull);
        cnt = m ? __popcll(X[size_t(bf) * SCAN_BLOCK_WORDS + lane] & m) : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    return (bf < n_blocks ? boff[bf] : n_active) + cnt;
}

}  // namespace tsc
