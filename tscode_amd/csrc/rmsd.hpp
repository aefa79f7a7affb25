// rmsd.hpp -- K3: the per-pass kernels of prune_conformers_rmsd around its pair kernels, all launched by prune.hip alone (no other unit includes
// this): the start of a run (k_init_run), a pass step of its own (k_pass_step), the rows of a pass (k_open_rows), the coordinate layouts of the
// register-tiled kernel (k_compact_coords), apply and merge of a finished pass (k_apply_pass, k_range_open, k_pass_merge, k_views_summaries) and
// the end of a run (k_export_run).  The arithmetic of a pair is in pair_math.hpp, the state of a run and the device functions that step it in
// pass_state.hpp, the register-tiled pair kernel in rmsd_tile.hpp.
#pragma once
#include "mm_record.hpp"
#include "pass_state.hpp"
#include "scan.hpp"

namespace tsc {

// Initial state of a run: out_mask = ones (rmsd_pruning.py:182), empty cache (:183), zeroed records, counters, tickets.
struct InitArgs {
    int64_t n;
    uint8_t *mask;
    unsigned long long *bits;  // two copies of the mask as bits, bit_words each
    int bit_words;
    unsigned long long *views;  // cache views of every pass of the schedule + their summaries
    int64_t view_words;
    ViewPass *view_pass;        // device copy of the schedule
    int n_views;
    ViewPass sched[MAX_SLOTS];
    PruneState *st;
    PassRecord *rec;
    int n_rec;
    PassCounters *cnt;
    int32_t *bsum, *boff;       // per scan block: active structures in it / before it
    int n_blocks, block_items;
    unsigned *dmax_bits;
    unsigned *zero_words;       // arrival counters of the kernels that close a pass
    int64_t n_zero_words;
    int32_t *tile_done;         // arrivals per row tile of the fused pair kernel
    int64_t n_tile_done;
    int32_t *act;
    int32_t *known;             // known[i]: every still-active column at a position in (i, known[i]) has been found dissimilar to i (k_open_rows); i + 1 here
    int first_slot;
    long long first_k;
    int first_algo;
    const float *Dall;          // with mm_rec: the descriptors by structure, FINAL (with *rec_dmax_bits) before this launch -- runs that build their own
    const unsigned *rec_dmax_bits;  // behind it get their records from k_mm_records instead (prune.hip)
    _Float16 *mm_rec;           // the float16 records by structure index the chunk-local pass screens with ("sieve_mm16"; local_pass.hpp), or null
};
inline __global__ __launch_bounds__(256) void k_init_run(InitArgs a) {
    // first_slot >= 0: the first pass of the schedule is opened here as well (gate of rmsd_pruning.py:192 on the full count,
    // its record), which is all a k_pass_step launch would do at this point
    const int64_t n = a.n;
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long *m8 = reinterpret_cast<unsigned long long *>(a.mask);  // scratch blocks are 256-byte aligned
    for (int64_t e = tid; e < n / 8; e += stride) m8[e] = 0x0101010101010101ull;
    for (int64_t e = (n / 8) * 8 + tid; e < n; e += stride) a.mask[e] = 1;
    // every entry of the active list is a valid structure index from the start: the pair kernel gathers through
    // act[x] for x up to n without knowing the active count
    for (int64_t e = tid; e < n; e += stride) a.act[e] = int32_t(e), a.known[e] = int32_t(e + 1);
    if (a.mm_rec) {  // (once per run: the records by position are k_open_rows', every pass)
        const float sigma = mm_scale(*a.rec_dmax_bits);
        for (int64_t e = tid; e < n; e += stride) {
            float d[2 * MM_KD];
#pragma unroll
            for (int q = 0; q < MM_KD / 2; ++q) {
                const float4 v = *reinterpret_cast<const float4 *>(a.Dall + e * (2 * MM_KD) + 4 * q);
                d[4 * q] = v.x, d[4 * q + 1] = v.y, d[4 * q + 2] = v.z, d[4 * q + 3] = v.w;
            }
            mm_write_record(d, sigma, a.mm_rec + e * MM_REC_HALVES);
        }
    }
    for (int64_t e = tid; e < a.bit_words; e += stride) {  // n ones, zeros behind them, in both copies
        const int64_t lo = e * 64;
        const unsigned long long w = lo + 64 <= n ? ~0ull : (lo >= n ? 0ull : ((1ull << (n - lo)) - 1ull));
        a.bits[e] = w, a.bits[a.bit_words + e] = w;
    }
    for (int64_t e = tid; e < a.view_words; e += stride) a.views[e] = 0;
    unsigned long long *c = &a.cnt->w[0][0];  // the counters of every slot: zeroed here, once per run, and by nothing else
    for (int64_t e = tid; e < int64_t(MAX_SLOTS) * CNT_BUCKETS * CNT_WORDS; e += stride) c[e] = 0;
    for (int64_t e = tid; e < a.n_zero_words; e += stride) a.zero_words[e] = 0;
    for (int64_t e = tid; e < a.n_tile_done; e += stride) a.tile_done[e] = 0;
    char *r = reinterpret_cast<char *>(a.rec);
    for (int64_t e = tid; e < int64_t(a.n_rec) * int64_t(sizeof(PassRecord)); e += stride)
        if (int(e / int64_t(sizeof(PassRecord))) != a.first_slot) r[e] = 0;  // (the first pass's record is written whole below)
    // per-block counts of the mask and their exclusive prefix: what ranks an active structure (k_open_rows); the kernels
    // that remove rows keep the counts current, the one that closes a pass the prefix
    for (int64_t e = tid; e <= a.n_blocks; e += stride) {
        const int64_t lo = e * a.block_items;
        if (e < a.n_blocks) a.bsum[e] = int32_t(lo >= n ? 0 : (n - lo < a.block_items ? n - lo : a.block_items));
        a.boff[e] = int32_t(lo >= n ? n : lo);
    }
    if (tid < a.n_views) a.view_pass[tid] = a.sched[tid];
    if (tid == 0) {
        if (a.dmax_bits) *a.dmax_bits = 0;  // running maximum of the descriptor build (describe.hpp)
        // the state block of every slot starts as that of the untouched ensemble, gated off; a slot's own is written by whoever opens it
        for (int s = 0; s < MAX_SLOTS; ++s) {
            PruneState *ss = a.st + s;
            ss->n_active = int(n), ss->pass_on = 0, ss->A = int(n), ss->ticket = 0, ss->bitsel = 0, ss->row_lo = 0, ss->cull_on = 0;
        }
        PruneState *st = a.st + (a.first_slot >= 0 ? a.first_slot : 0);
        if (a.first_slot >= 0) {
            const int on = (a.first_k == 1 || 20 * a.first_k < (long long)n) ? 1 : 0;
            PassRecord &fr = a.rec[a.first_slot];
            fr.k = a.first_k, fr.n_before = fr.n_after = (long long)n, fr.on = on, fr.algo = a.first_algo;
            fr.formed = fr.exact = fr.screened = fr.evaluated = fr.removed = fr.known = 0;
            st->pass_on = on;
        }
    }
}

inline __global__ __launch_bounds__(64) void k_pass_step(StepCtx sc, StepArgs sa) { pass_step_wave(sc, sa); }

// ---------------------------------------------------------------------------------------------------
// per-pass helper kernels (the pass sequence is in prune.hip, tsc_prune_pass_local / tsc_prune_pass_finish)

// Everything a pass needs per ROW, in one launch with no kernel in front of it: ONE LANE per active row r, one wavefront per 64 rows
// = four row tiles of the pair kernel, four wavefronts per block.
//   * which structure is the r-th active one: the scan block from the prefix of the block counts (boff, kept current by
//     the kernel that closed the previous pass), the bit inside the block from the 32 words of the mask's bit copy --
//     an ordered compaction without a scan pass over the whole mask.  The 64 rows of a wavefront are consecutive ranks, so they lie
//     in one or two scan blocks: the wavefront stages a block's 32 words and their running popcounts in LDS ONCE (stage_block) and
//     every row of that block finds its word by search and its bit by select;
//   * cend[r] = rank of the first active column j in (i, last) with (first + (j - i)) in the cache view of this pass (the
//     row returns "not similar" there, :66-67), else rank of `last`.  Columns of compacted rank in (r, cend[r]) are the
//     ones the reference may still evaluate for row r.  Ranks of positions come from staged blocks too: the rows of a wavefront
//     share their chunk's end (one or two distinct targets), a cache hit lies a few positions behind its row;
//   * act[r], best[r] = none, the row's descriptor copied to position r of Dc (the pair kernel reads rows and columns by
//     position), the largest stop column of every tile;
//   * the other bit copy of the mask brought up to date (the rows this pass removes are cleared THERE, so that every row of
//     the pass sees the mask as it was when the pass began, rmsd_pruning.py:151-157, whatever order the tiles finish in).
// fused != 0: the pair kernel applies the verdicts of a row tile itself when the tile's last work item finishes, and the
// last tile closes the pass.  A tile without work (no row with columns to look at; beyond the active count; the pass gated
// off) has nothing to apply and arrives here.
// (Rounds 2 - 4 gave a row 16, then 4 lanes: at a million structures 30 000 wavefronts each waited out the same memory round trips and
// the kernel was bound by instruction issue -- 45 us per pass at C4, 12 at C3.  A lane per row is a quarter of the wavefronts and of
// the wave-instructions per row.)
constexpr int OPEN_LDS_BLOCKS = 2048;  // scan blocks whose prefix is staged in LDS (4 M structures); beyond: read from memory
constexpr int OPEN_ROWS = 64;          // rows per wavefront
constexpr int OPEN_LIST_CAP = 64 + 1024;  // a refill stops once it holds 64 entries; the block that takes it there adds 1024 at most
struct OpenArgs {
    int use_cache, fused, lds_cap;
    const unsigned long long *view;  // cache view of this pass and its summary (bit_words behind it)
    unsigned long long *bits;        // the two bit copies of the mask
    int bit_words;
    const int32_t *boff;
    int n_blocks, block_items;
    unsigned n_tiles;                // row tiles of the pass (arrival count of a fused pass that closes itself)
    PassTickets *tickets;
    DeriveArgs dv;                   // dv.prev_st != null: the pass before this one was left open and is closed here (pass_derive) ...
    const int32_t *bsum;             // ... from the scan blocks' counts; the prefix goes to LDS (the host sees to n_blocks <= lds_cap) and,
    int32_t *boff_out;               // from workgroup 0, to memory, for the kernels behind this one
    int32_t *rank_of;                // (optional) rank_of[structure] = its active rank: what a culled pass (cull.hpp) lays its sorted order out from
    _Float16 *Dh;                    // (optional) the float16 records of the matrix-core screen (mm.hpp), by position like Dc
    const unsigned *dmax_bits;       // ... and the largest |descriptor component| of the run that scales them
    // What earlier passes of the run know about a row (null: nothing is read or kept).  A row i that SURVIVES a pass had every column that was
    // active between it and its stop position found dissimilar; a pair's verdict depends on its two structures alone and the mask only
    // shrinks, so no later pass needs to look at the active columns before known[i] = the furthest such stop position again.  cbeg[r] = the
    // rank of the first active position >= known[i] (>= r + 1), written beside cend[r]; the smallest cbeg of a tile's rows that have columns
    // left goes beside the tile's largest stop column (tile_cmax[2 t + 1]).  Without `skip`: r + 1 and 0.  A hint: too small a known[] costs work, never a verdict -- too large a one would.
    int32_t *known;
    int32_t *cbeg;
    int skip;                        // the pair kernel behind this launch starts its rows at cbeg and applies its own tiles: a tile whose rows all have
                                     // cbeg >= cend is dead HERE (tile_cmax = 0) and its rows' cend - r - 1 pairs go to CNT_EVALUATED here; the pairs
                                     // before cbeg are summed into CNT_KNOWN
    unsigned long long *dbg;         // -DTSC_DBG_STAMPS builds only: 8 time stamps per wavefront (tools/stamps.py), else null
};
#ifdef TSC_DBG_STAMPS
#define TSC_OPEN_STAMP(i)                                                                                                     \
    do {                                                                                                                      \
        if (oa.dbg) {                                                                                                         \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                       \
            if ((threadIdx.x & 63) == 0) oa.dbg[size_t(blockIdx.x) * 32 + (threadIdx.x >> 6) * 8 + (i)] = wall_clock64();       \
        }                                                                                                                     \
    } while (0)
#else
#define TSC_OPEN_STAMP(i) do { } while (0)
#endif
inline __global__ __launch_bounds__(256) void k_open_rows(PassGeom g, OpenArgs oa, StepCtx sc, StepArgs next, int32_t *__restrict__ act,
                                                    int32_t *__restrict__ cend, int32_t *__restrict__ best, int32_t *__restrict__ tile_cmax,
                                                    const float *__restrict__ D, float *__restrict__ Dc) {
    static_assert(SCAN_BLOCK_WORDS == 32 && OPEN_ROWS == 64 && DESC_WORDS == 16, "one wavefront = 64 rows = four row tiles; a block's 32 words on 32 lanes");
    __shared__ int s_boff[OPEN_LDS_BLOCKS + 1];
    __shared__ unsigned long long s_w[4][SCAN_BLOCK_WORDS];   // per wavefront: the words of the scan block staged last ...
    __shared__ int s_pre[4][SCAN_BLOCK_WORDS];                // ... and the set bits below each of them
    __shared__ int s_list[4][OPEN_LIST_CAP];                  // per wavefront: deltas of the cache view's set bits inside its chunk, ascending
    const PruneState *st = sc.st;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (the first 256 entries of the prefix are requested together with the state block: one round trip for both)
    const bool in_lds = oa.n_blocks <= oa.lds_cap;
    const bool derive = oa.dv.prev_st != nullptr;   // (the prefix of a derived pass comes from bsum, below; memory holds the one before it)
    const int boff_mine = (!derive && in_lds && int(threadIdx.x) <= oa.n_blocks) ? oa.boff[threadIdx.x] : 0;
    TSC_OPEN_STAMP(0);  // started (and the first loads have come back)
    // (row_lo / n_all differ from 0 / A only in a rank-partitioned pass: rows and ranks below are LOCAL except where the mask's
    // own ranking -- the prefix of the scan blocks -- is consulted)
    // One read of the state per WORKGROUP (a barrier below is conditional on it).  The pass before this one was either closed by its
    // own last unit, which wrote this slot's state block, or left open: then the first wavefront works the block out (pass_derive)
    __shared__ int s_state[5];
    if (derive) {
        if (wid == 0) {
            const Derived d = pass_derive(oa.dv, sc.st, blockIdx.x == 0, oa.bsum, oa.n_blocks, s_boff, oa.boff_out);
            if (lane == 0) s_state[0] = d.pass_on, s_state[1] = d.n_active, s_state[2] = d.bitsel, s_state[3] = 0, s_state[4] = d.n_active;
        }
    } else if (threadIdx.x == 0) {
        s_state[0] = st->pass_on, s_state[1] = st->A, s_state[2] = st->bitsel, s_state[3] = st->row_lo, s_state[4] = st->n_active;
    }
    __syncthreads();
    const int pass_on = s_state[0], A = s_state[1], sel = s_state[2], row_lo = s_state[3], n_all = s_state[4];
    const unsigned long long *X = oa.bits + size_t(sel) * oa.bit_words;
    const unsigned wave = blockIdx.x * 4 + wid;          // rows 64 wave .. 64 wave + 63, tiles 4 wave .. 4 wave + 3
    const int R0 = int(wave) * OPEN_ROWS;
    const unsigned tile = wave * 4 + unsigned(lane >> 4);
    if (pass_on) {
        unsigned long long *Xo = oa.bits + size_t(sel ^ 1) * oa.bit_words;
        for (int w = blockIdx.x * 256 + threadIdx.x; w < oa.bit_words; w += gridDim.x * 256) Xo[w] = X[w];
    }
    if (!derive && pass_on && in_lds && int(blockIdx.x) * 4 * OPEN_ROWS < A) {  // (block-uniform)
        if (int(threadIdx.x) <= oa.n_blocks) s_boff[threadIdx.x] = boff_mine;
        for (int e = threadIdx.x + 256; e <= oa.n_blocks; e += 256) s_boff[e] = oa.boff[e];
        __syncthreads();
    }
    if (wave * 4 >= oa.n_tiles) return;  // (padding of the last block)
    TSC_OPEN_STAMP(1);  // bit copy made, prefix staged
    int my_c = 0;        // stop column of this lane's row (0 for lanes without one: the tile maxima below)
    int my_cb = 0;       // ... and its first column
    if (pass_on && R0 < A) {
        // The kernel is a chain of dependent memory round trips (a light pass is bound by it, not by work): loads that do not depend on
        // each other are issued TOGETHER -- (1) state + prefix, above; (2) the words of the rows' scan blocks; (3) descriptors, the cache
        // view's summary and the words of the stop positions' scan block; then the stores.
        auto before = [&](int b) { return in_lds ? s_boff[b] : oa.boff[b]; };
        unsigned long long *sw = s_w[wid];
        int *sp = s_pre[wid];
        auto load_block = [&](int b) -> unsigned long long {   // word `lane` of scan block b (zeros beyond the last block)
            return (lane < SCAN_BLOCK_WORDS && b < oa.n_blocks) ? X[size_t(b) * SCAN_BLOCK_WORDS + lane] : 0ull;
        };
        // a block's 32 words and the set bits below each of them -> this wavefront's LDS area
        auto stage_words = [&](unsigned long long w) {
            __builtin_amdgcn_wave_barrier();   // (everybody has finished with the block staged before)
            const int c = __popcll(w);
            int incl = c;
#pragma unroll
            for (int off = 1; off < SCAN_BLOCK_WORDS; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (lane < SCAN_BLOCK_WORDS) sw[lane] = w, sp[lane] = incl - c;
            __builtin_amdgcn_wave_barrier();
        };
        const int r_true = R0 + lane;
        const bool mine = r_true < A;
        const int r = mine ? r_true : A - 1;  // (idle lanes walk along with the last row: the loops below stay convergent)
        const int rg = r + row_lo;            // its rank among ALL active structures
        // scan block of rank rg: the last b with boff[b] <= rg  (boff[0] = 0, boff[n_blocks] = n_all > rg).  The wavefront's rows are
        // consecutive ranks: the block of its FIRST row by a 64-way search (the lanes test 64 boundaries at once, coarse then fine --
        // three trips to LDS for up to 262 144 blocks instead of one per halving), the others a boundary or two further on
        int lo;
        {
            const int rg0 = __builtin_amdgcn_readfirstlane(rg);
            int base = 0, span = oa.n_blocks;   // invariant: boff[base] <= rg0 < boff[base + span]
            while (span > 1) {
                const int step = (span + 63) >> 6;
                const int b = base + lane * step;
                const unsigned long long le = __ballot(b < base + span && before(b) <= rg0);   // lane 0 always (the invariant)
                const int q = __popcll(le) - 1;           // boundaries are ascending: the set lanes are 0 .. q
                base += q * step;
                span = min(step, oa.n_blocks - base);
            }
            lo = base;
            while (__ballot(lo + 1 < oa.n_blocks && before(lo + 1) <= rg))
                if (lo + 1 < oa.n_blocks && before(lo + 1) <= rg) ++lo;
        }
        const int rem = rg - before(lo);      // the row is the rem-th active structure of its scan block
        int pos = 0;
        {
            // the (one or two, on sparse masks more) distinct scan blocks of this wavefront's rows: the first and the last are requested
            // together
            const int b_first = __builtin_amdgcn_readfirstlane(lo), b_last = __builtin_amdgcn_readlane(lo, 63);
            const unsigned long long w_first = load_block(b_first);
            const unsigned long long w_last = b_last != b_first ? load_block(b_last) : 0ull;
            for (unsigned long long pending = __ballot(true); pending;) {
                const int b = __builtin_amdgcn_readlane(lo, __ffsll((long long)pending) - 1);
                stage_words(b == b_first ? w_first : (b == b_last ? w_last : load_block(b)));
                if (lo == b) {
                    int u = 0;                     // the last word with sp[u] <= rem
#pragma unroll
                    for (int s2 = SCAN_BLOCK_WORDS / 2; s2 > 0; s2 >>= 1)
                        if (sp[u + s2] <= rem) u += s2;
                    pos = 64 * u + select64(sw[u], rem - sp[u]);
                }
                pending &= ~__ballot(lo == b);
            }
        }
        const int64_t i = int64_t(lo) * oa.block_items + pos;
        int64_t first, last;
        chunk_of(g, i, first, last);
        TSC_OPEN_STAMP(2);  // the row's structure found
        // candidate deltas d = 1 .. len, i.e. cache-view positions P = first + d in [p_lo, p_hi]; the view is sparse (a
        // key applies to a pass only when its chunk start is one of this pass's), so the row walks the NON-EMPTY 1024-bit
        // blocks of it, found through the summary bitmap, instead of every block of its chunk
        const unsigned long long *dbit = oa.view, *dsum = oa.view + oa.bit_words;
        const int64_t len = mine ? last - i - 1 : 0;
        const int64_t p_lo = first + 1, p_hi = first + len, shift = i - first;  // mask position of P is P + shift
        const bool walk = oa.use_cache != 0 && len > 0;
        // one batch of requests: the descriptor, the first summary word of the cache view, the scan block of the chunk's end
        f32x4 dval[4];
        if (D) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dval[q] = *reinterpret_cast<const f32x4 *>(D + i * 16 + 4 * q);
        }
        const unsigned long long sum_first = walk ? dsum[(p_lo >> 10) >> 6] : 0ull;
        const int bl_first = __builtin_amdgcn_readfirstlane(int(last / oa.block_items));
        const unsigned long long wl_first = load_block(bl_first);
        const int64_t known_i = oa.known ? int64_t(oa.known[i]) : i + 1;   // (i + 1 <= known_i <= n)
        // The stop column is the end of the chunk unless the cache view has a hit: the first delta d >= 1 whose key (first, first + d) is in the
        // view AND whose column i + d is active (rmsd_pruning.py:65-67).
        // Rows of ONE chunk (every wavefront of a late pass) look at the same view bits, shifted against the mask by their own position: the
        // wavefront lists the view's set bits once (in LDS, ascending, 64 or more at a time, walking the non-empty 1024-bit blocks through the
        // summary) and every row tests ITS mask bit behind each of them, eight at a time.  A hit comes after a few tests -- a row's
        // column is active more often than not -- where a walk word by word and row by row was as long as the unluckiest of the 64 rows
        // (the k = 1 pass of C3: 68 us for 21 000 rows).  Wavefronts whose rows lie in several chunks (early passes: short chunks, nearly empty
        // views) walk lane by lane, below.
        const bool one_chunk = __ballot(first != __shfl(first, 0)) == 0;
        // (the scan block that ranks known_i: requested with the cache view's loads.  The rows of a wavefront mostly share an earlier chunk's end.
        // Only where the pass's pair kernel starts its rows there, oa.skip: any other tracked pass -- the 64-row and packed-fp32 kernels, a
        // candidate for culling, k_apply_pass behind the pair kernel -- only RAISES known[], for a later pass of the run that may skip)
        const int bk = int(known_i / oa.block_items), bk_first = __builtin_amdgcn_readfirstlane(bk);
        const unsigned long long wk_first = (oa.skip && bk_first != bl_first) ? load_block(bk_first) : 0ull;
        int64_t found = last;
        if (oa.use_cache != 0 && one_chunk) {
            int *list = s_list[wid];
            const int64_t dmax = __shfl(len, 0);              // rows ascend: lane 0 has the longest range (and is always a row of the pass)
            const unsigned long long sum0 = (unsigned long long)__shfl((long long)sum_first, 0);   // (lanes without a range of their own loaded none)
            int64_t Bc = (first + 1) >> 10;
            const int64_t Bh = (first + dmax) >> 10;
            bool scanning = len > 0;
            while (__ballot(scanning)) {
                int n_list = 0;
                while (n_list < 64 && Bc <= Bh) {             // (wave-uniform: every lane holds the same first, dmax, Bc, n_list)
                    // up to 16 of the next non-empty blocks at once, four lanes per block and four words per lane: a sparse view (C3's
                    // last pass: 96 keys over 30 blocks) is listed in one round trip, not one per block
                    const unsigned long long sb = ((Bc >> 6) == ((p_lo >> 10) >> 6) ? sum0 : dsum[Bc >> 6]) >> (Bc & 63);   // bit t: block Bc + t
                    if (!sb) {
                        Bc = ((Bc >> 6) + 1) << 6;
                        continue;
                    }
                    const int j = lane >> 2, q = lane & 3;
                    int64_t Bj = -1;
                    if (j < __popcll(sb)) {
                        Bj = Bc + select64(sb, j);
                        if (Bj > Bh) Bj = -1;
                    }
                    unsigned long long w4[4] = {0ull, 0ull, 0ull, 0ull};
                    int c = 0;
                    if (Bj >= 0) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int64_t p0 = (Bj * 16 + 4 * q + u) * 64;
                            unsigned long long w = 0ull;
                            if (p0 <= first + dmax && p0 + 63 >= first + 1) {
                                w = dbit[p0 >> 6];
                                if (p0 < first + 1) w &= (first + 1 - p0 < 64) ? (~0ull << (first + 1 - p0)) : 0ull;
                                if (first + dmax - p0 < 63) w &= (2ull << (first + dmax - p0)) - 1ull;
                            }
                            w4[u] = w;
                            c += __popcll(w);
                        }
                    }
                    int incl = c;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const int t = __shfl_up(incl, off);
                        if (lane >= off) incl += t;
                    }
                    // whole blocks, in order, as long as the list has room (the first always fits: a block holds 1024 keys at most)
                    const bool fits = Bj >= 0 && __shfl(incl, lane | 3) <= OPEN_LIST_CAP - n_list;
                    const int n_valid = __popcll(__ballot(Bj >= 0 && q == 3)), n_fit = __popcll(__ballot(fits && q == 3));
                    if (fits) {
                        int kk = n_list + incl - c;
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int64_t p0 = (Bj * 16 + 4 * q + u) * 64;
                            for (unsigned long long w = w4[u]; w; w &= w - 1) list[kk++] = int(p0 + (__ffsll((long long)w) - 1) - first);
                        }
                    }
                    if (n_valid == 0) {
                        Bc = Bh + 1;                            // the summary's next blocks lie beyond the chunk
                    } else {
                        n_list += __shfl(incl, 4 * n_fit - 1);
                        Bc = __shfl(Bj, 4 * n_fit - 1) + 1;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                TSC_OPEN_STAMP(6);  // (the list refilled)
                if (n_list == 0) break;                        // the view has no further key inside the chunk: no row stops early
                int kidx = 0;
                while (__ballot(scanning && kidx < n_list)) {
                    if (scanning && kidx < n_list) {
                        int dd[8];
                        unsigned long long mw[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) dd[t] = kidx + t < n_list ? list[kidx + t] : INT_MAX;
#pragma unroll
                        for (int t = 0; t < 8; ++t) mw[t] = int64_t(dd[t]) <= len ? X[(i + dd[t]) >> 6] : 0ull;
                        int hit = -1;
#pragma unroll
                        for (int t = 7; t >= 0; --t)
                            if (int64_t(dd[t]) <= len && ((mw[t] >> ((i + dd[t]) & 63)) & 1ull)) hit = dd[t];
                        bool beyond = false;                   // the (ascending) list has left this row's range
#pragma unroll
                        for (int t = 0; t < 8; ++t) beyond = beyond || (dd[t] != INT_MAX && int64_t(dd[t]) > len);
                        if (hit >= 0) found = i + hit, scanning = false;
                        else if (beyond) scanning = false;
                        kidx += 8;
                    }
                }
                __builtin_amdgcn_wave_barrier();               // (before the list is refilled)
                TSC_OPEN_STAMP(7);  // (the list tested)
                // a row still scanning here has used up this list: on to the next non-empty blocks (none left: n_list = 0 above)
                if (Bc > Bh) {
                    // (the range is exhausted: rows that have not hit anything keep found = last)
                    break;
                }
            }
        }
        if (walk && !one_chunk) {
            int64_t B = p_lo >> 10;
            const int64_t B_hi = p_hi >> 10, S_first = (p_lo >> 10) >> 6;
            bool scanning = true;
            while (scanning) {
                bool any = false;            // next non-empty block at or after B
                while (B <= B_hi) {
                    const unsigned long long sb = ((B >> 6) == S_first ? sum_first : dsum[B >> 6]) >> (B & 63);
                    if (sb) {
                        B += __ffsll((long long)sb) - 1;
                        any = B <= B_hi;
                        break;
                    }
                    B = ((B >> 6) + 1) << 6;
                }
                if (!any) break;
                // the 16 words of the block: requested together (one round trip, not one per word), then the mask words behind the
                // non-empty ones; in ascending order the first cached column (mask position) ends the walk
                unsigned long long vw[16], xw[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int64_t p0 = (B * 16 + u) * 64;  // first position of this word
                    unsigned long long w = (p0 <= p_hi && p0 + 63 >= p_lo) ? dbit[p0 >> 6] : 0ull;
                    if (p0 < p_lo) w &= (p_lo - p0 < 64) ? (~0ull << (p_lo - p0)) : 0ull;
                    if (p_hi - p0 < 63) w &= p_hi >= p0 ? ((2ull << (p_hi - p0)) - 1ull) : 0ull;
                    vw[u] = w;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) xw[u] = vw[u] ? extract64(X, (B * 16 + u) * 64 + shift) : 0ull;
#pragma unroll
                for (int u = 15; u >= 0; --u) {
                    const unsigned long long w = vw[u] & xw[u];
                    if (w) found = (B * 16 + u) * 64 + (__ffsll((long long)w) - 1) + shift, scanning = false;
                }
                ++B;
                if (B > B_hi) scanning = false;
            }
        }
        TSC_OPEN_STAMP(3);  // the cache view walked
        // rank of the stop position = active structures before it: the prefix of its scan block + the set bits of the block below it.
        // The rows of a wavefront share their targets' scan blocks (the chunk's end; a hit a few positions behind its row): one staging
        // per distinct block
        int my_b = 0;        // first column this row still has to look at (the rank of known_i; r + 1 where nothing is known)
        {
            const int bf = int(found / oa.block_items), off = int(found - int64_t(bf) * oa.block_items);
            const int offk = int(known_i - int64_t(bk) * oa.block_items);
            auto rank_in = [&](int b, int o) {   // active structures before offset o of the staged block b
                const int u = o >> 6, below = o & 63;
                return (b < oa.n_blocks ? before(b) : n_all) + sp[u] + __popcll(sw[u] & (below ? (~0ull >> (64 - below)) : 0ull)) - row_lo;
            };
            unsigned long long pend_k = oa.skip ? __ballot(true) : 0ull;
            for (unsigned long long pending = __ballot(true); pending | pend_k;) {
                const int b = pending ? __builtin_amdgcn_readlane(bf, __ffsll((long long)pending) - 1) : __builtin_amdgcn_readlane(bk, __ffsll((long long)pend_k) - 1);
                stage_words(b == bl_first ? wl_first : ((oa.skip && b == bk_first) ? wk_first : load_block(b)));
                if (bf == b) my_c = rank_in(b, off);
                if (oa.skip && bk == b) my_b = rank_in(b, offk);
                pending &= ~__ballot(bf == b);
                pend_k &= ~__ballot(bk == b);
            }
            if (!oa.skip) my_b = r + 1;
        }
        TSC_OPEN_STAMP(4);  // stop column's rank
        if (mine) {
            if (D) {
                if (Dc)   // (null where nothing reads the fp32 rows by position: the 16-row matrix-core kernel of a pass that cannot be culled)
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4 *>(Dc + int64_t(r) * 16 + 4 * q) = dval[q];
                if (oa.Dh) {   // (made here every pass; copying them from records made once per run was measured: no faster, 80 B more per structure)
                    float dv[16];
#pragma unroll
                    for (int q = 0; q < 4; ++q) dv[4 * q] = dval[q].x, dv[4 * q + 1] = dval[q].y, dv[4 * q + 2] = dval[q].z, dv[4 * q + 3] = dval[q].w;
                    mm_write_record(dv, mm_scale(*oa.dmax_bits), oa.Dh + int64_t(r) * MM_REC_HALVES);
                }
            }
            act[r] = int32_t(i);
            cend[r] = my_c;
            oa.cbeg[r] = my_b;
            if (oa.known && found > known_i) oa.known[i] = int32_t(found);   // (a row this pass removes is never a row again: its entry is never read)
            best[r] = INT_MAX;  // atomicMin target of the pair kernel: no similar column found yet
            if (oa.rank_of) oa.rank_of[i] = r;
        }
        if (oa.rank_of) {  // a pass that may be culled: how many pairs lie inside the rows' ranges (what the ordered walk would look at)
            long long w = mine ? (long long)max(0, my_c - r - 1) : 0ll;
            for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
            if (lane == 0) count_add(sc.cnt, wave, CNT_WALK, (unsigned long long)w);
        }
        if (!mine) my_c = 0, my_b = 0;
        my_cb = my_b;
        TSC_OPEN_STAMP(5);  // everything written
    }
    // largest stop column of the 16 rows of every tile: lets a work item of the pair kernel whose column segment lies
    // beyond it leave after one scalar load (0: every work item of the tile leaves at its first test -- also for a pass that is
    // gated off and for tiles beyond the active count)
    // ... and the smallest first column of the rows that have columns left (INT_MAX: none has -- under oa.skip the tile is dead, cmax = 0, and
    // what its rows' verdicts would have counted as evaluated, cend - r - 1 each, is counted here: nobody applies a dead tile)
    int cmax = my_c, cmin = my_cb < my_c ? my_cb : INT_MAX;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off)), cmin = min(cmin, __shfl_xor(cmin, off));
    if (oa.skip) {
        const int r_lane = int(wave) * OPEN_ROWS + lane;
        const bool owes = cmin == INT_MAX && my_c > r_lane + 1;               // (my_c = 0 for lanes without a row)
        unsigned long long ev = owes ? (unsigned long long)(my_c - r_lane - 1) : 0ull;
        unsigned long long kn = my_c > 0 ? (unsigned long long)max(0, min(my_cb, my_c) - r_lane - 1) : 0ull;
        if (__ballot(ev != 0ull || kn != 0ull)) {
            for (int off = 32; off > 0; off >>= 1) ev += __shfl_xor(ev, off), kn += __shfl_xor(kn, off);
            if (lane == 0) count_add(sc.cnt, wave, CNT_EVALUATED, ev), count_add(sc.cnt, wave, CNT_KNOWN, kn);
        }
        if (cmin == INT_MAX) cmax = 0;
    }
    const bool tile_lane = (lane & 15) == 0 && tile < oa.n_tiles;
    if (tile_lane) tile_cmax[2 * tile] = cmax, tile_cmax[2 * tile + 1] = oa.skip ? cmin : 0;
    // no work item of the pair kernel will find a column for this tile: it has nothing to apply and arrives here
    const bool dead = tile_lane && cmax <= ((int(tile) * 16 + 1) & ~63);
    if (!oa.fused || !__ballot(dead)) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool fin = dead && tickets_arrive(oa.tickets, tile, oa.n_tiles, PT_GROUPS);
    if (__ballot(fin)) pass_step_wave(sc, next);
}

// Gather the active structures into the two layouts the tile kernel reads:
//   Xr[r][HP3]   row-major, zero-padded to HP atoms  (row structures: wavefront-uniform scalar reads)
//   Xc[d][ld]    coordinate-major                    (column structures: lane = column, coalesced)
//   G[r] = sum |x|^2
// One block moves 64 structures through an LDS tile so that both global sides are coalesced.
inline __global__ __launch_bounds__(256) void k_compact_coords(const double *__restrict__ heavy, int h, int hp3,
                                                         const int32_t *__restrict__ act_idx, const PruneState *__restrict__ st,
                                                         double *__restrict__ Xr, double *__restrict__ Xc, int64_t ld,
                                                         double *__restrict__ G) {
    extern __shared__ __attribute__((aligned(16))) double s_tile[];  // [64][hp3 + 1]
    if (st->pass_on == 0) return;
    const int n_active = st->A;
    const int h3 = h * 3, pitch = hp3 + 1;
    const int r0 = blockIdx.x * 64;
    if (r0 >= n_active) return;
    const int nr = min(64, n_active - r0);
    for (int e = threadIdx.x; e < 64 * hp3; e += 256) {
        int rr = e / hp3, d = e - rr * hp3;
        double v = 0.0;
        if (rr < nr && d < h3) v = heavy[int64_t(act_idx[r0 + rr]) * h3 + d];
        s_tile[rr * pitch + d] = v;
        if (rr < nr) Xr[int64_t(r0 + rr) * hp3 + d] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * hp3; e += 256) {
        int d = e >> 6, rr = e & 63;
        Xc[int64_t(d) * ld + r0 + rr] = s_tile[rr * pitch + d];  // rows >= nr are zeros
    }
    if (threadIdx.x < 64) {
        double g = 0.0;
        for (int d = 0; d < h3; ++d) {
            double v = s_tile[threadIdx.x * pitch + d];
            g += v * v;
        }
        G[r0 + threadIdx.x] = g;
    }
}

// Apply a finished pass as a launch of its own (the register-tiled kernel's passes, and passes whose rows were searched by
// several ranks: best[] is complete only after the exchange).  The sieve kernel of a single-rank run does this itself, tile
// by tile (sieve.hpp).
inline __global__ __launch_bounds__(256) void k_apply_pass(ApplyArgs a, StepCtx sc, StepArgs next) {
    __shared__ int s_last;
    PruneState *st = sc.st;
    const bool pass_on = st->pass_on != 0;
    const int n_active = pass_on ? st->A : 0;  // a pass that is gated off has no rows; its blocks still take a ticket
    const int sel = st->bitsel;
    const int lane = threadIdx.x & 63;
    unsigned long long ev_total = 0, rm_total = 0;
    // a capped grid walks the rows tile by tile (block-uniform bounds: every wavefront keeps all its lanes for the ballots)
    for (int row0 = blockIdx.x * 256; row0 < n_active; row0 += gridDim.x * 256) {
        const int r = row0 + threadIdx.x;
        apply_wave_rows(a, sel, r, r < n_active, ev_total, rm_total);
    }
    if (lane == 0) {
        const unsigned bucket = blockIdx.x * 4 + (threadIdx.x >> 6);
        count_add(sc.cnt, bucket, CNT_EVALUATED, ev_total);
        count_add(sc.cnt, bucket, CNT_REMOVED, rm_total);
    }
    // The last block to get here closes this pass and opens the next one (what a separate one-block launch would do).
    // The only data handed from block to block are the statistics buckets and block counts, and those are written by
    // agent-scope atomics and read with agent-scope (sc1) loads -- so no cache fence is needed (a __threadfence() per block
    // costs an L2 write-back each: measured 14 us per pass): every wave drains its atomics, the block's barrier, ONE lane's
    // ticket add, and the block whose add came last reads (MI355X_MICROARCH.md, inter-workgroup visibility, valid forms).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = atomicAdd(&st->ticket, 1u);
        s_last = (t == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (s_last && threadIdx.x < 64) pass_step_wave(sc, next);
}

// ---------------------------------------------------------------------------------------------------
// Rank-partitioned passes (one process per GPU, tscode_amd/pipeline.py).  The chunks of a pass are independent
// (rmsd_pruning.py:139-157: every chunk reads the same input mask and the same cache), so while a pass has several chunks
// per rank each rank takes the chunks that START inside its block [n r / W, n (r + 1) / W) of the structure axis and runs
// the whole pass flow on them alone -- k_open_rows over its rows only, the pair kernel, the tile-wise apply.  What it learns
// is which rows it removed: one bit each in an exchange buffer (n / 64 words + the pass's five statistics).  The host sums
// the ranks' buffers (the bits are disjoint, so the sum is their union; NCCL / RCCL have no bitwise reduction) and
// k_pass_merge makes the pass's outcome the state of every rank: mask bytes, the bit copy the next pass reads, the scan
// blocks' counts and prefix, the record, the gate of rmsd_pruning.py:192 for the next pass and -- when that one is
// rank-partitioned too -- which of the active structures are this rank's rows in it.
// The cache keys of the removed rows stay with the rank that removed them: a key (a, b) can only be hit by a later pass in
// the chunk that starts at a (pass_state.hpp, CacheViews), and the chunk that starts at a belongs to the same rank in every
// rank-partitioned pass.  Before the first pass that is NOT partitioned this way the host sums the cache views of the
// remaining passes over the ranks once (disjoint bits again) and k_views_summaries rebuilds their summary words.

// The rows of this rank in the OPEN pass: the active structures of [s_lo, s_hi) (whole chunks of that pass).  Needed as a
// launch of its own only where no k_pass_merge precedes the pass (the first pass of a run).
inline __global__ __launch_bounds__(64) void k_range_open(PruneState *__restrict__ st, const int32_t *__restrict__ boff, const unsigned long long *__restrict__ bits,
                                                    int bit_words, int n_blocks, int s_lo, int s_hi) {
    const unsigned long long *X = bits + size_t(st->bitsel) * bit_words;
    const int n_all = st->n_active;
    const int lo = rank_below_wave(boff, X, n_blocks, n_all, s_lo), hi = rank_below_wave(boff, X, n_blocks, n_all, s_hi);
    if ((threadIdx.x & 63) == 0) st->row_lo = lo, st->A = hi - lo;
}

struct MergeArgs {
    int n, bit_words, n_blocks;
    unsigned long long *bits;   // the two bit copies of the mask
    unsigned long long *exch;   // bit_words words of removed rows, then the five statistics: summed over the ranks by the host
    uint8_t *mask;
    int next_s_lo, next_s_hi;   // the next pass is rank-partitioned: this rank's structures [s_lo, s_hi) in it; -1: it is not
};
constexpr int MERGE_LDS_BLOCKS = 8192;  // scan blocks counted in LDS (16.7 M structures); beyond: every thread counts whole blocks from memory
inline __global__ __launch_bounds__(1024) void k_pass_merge(MergeArgs a, StepCtx sc, StepArgs sa) {
    __shared__ int s_cnt[MERGE_LDS_BLOCKS];
    __shared__ int s_part[16], s_run;
    PruneState *st = sc.st;
    PruneState *sn = sc.st_next ? sc.st_next : st;  // the state block of the slot this merge opens (that of the closing slot where there is none)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pass_on = st->pass_on, sel = st->bitsel, n_before = st->n_active;
    const bool closing = sa.prev >= 0 && pass_on != 0;
    const bool in_lds = a.n_blocks <= MERGE_LDS_BLOCKS;
    const unsigned long long *X = a.bits + size_t(sel) * a.bit_words;
    unsigned long long *Xo = a.bits + size_t(sel ^ 1) * a.bit_words;
    if (tid == 0) s_run = closing ? 0 : n_before;
    if (closing) {
        if (in_lds)
            for (int b = tid; b < a.n_blocks; b += 1024) s_cnt[b] = 0;
        __syncthreads();
        // the pass's outcome: the bit copy the next pass reads, the mask bytes of the removed rows, the scan blocks' counts
        for (int w = tid; w < a.bit_words; w += 1024) {
            const unsigned long long old = X[w];
            unsigned long long rm = a.exch[w];
            const unsigned long long now = old & ~rm;
            Xo[w] = now;
            if (in_lds && now) atomicAdd(&s_cnt[w / SCAN_BLOCK_WORDS], __popcll(now));  // (words behind the last block's are zero)
            if (rm) {
                a.exch[w] = 0;
                for (rm &= old; rm; rm &= rm - 1) a.mask[int64_t(w) * 64 + (__ffsll((long long)rm) - 1)] = 0;
            }
        }
        __syncthreads();  // (one block: its global and LDS writes are visible to all its threads behind the barrier)
        for (int b0 = 0; b0 < a.n_blocks; b0 += 1024) {
            const int b = b0 + tid;
            int c = 0;
            if (b < a.n_blocks) {
                if (in_lds) {
                    c = s_cnt[b];
                } else {
                    for (int u = 0; u < SCAN_BLOCK_WORDS; ++u)  // (the block list is padded beyond the last word of a bit copy)
                        c += b * SCAN_BLOCK_WORDS + u < a.bit_words ? __popcll(Xo[size_t(b) * SCAN_BLOCK_WORDS + u]) : 0;
                }
                sc.bsum[b] = c;
            }
            int incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (lane == 63) s_part[wv] = incl;
            __syncthreads();
            int base = s_run;
            for (int q = 0; q < wv; ++q) base += s_part[q];
            if (b < a.n_blocks) sc.boff[b] = base + incl - c;
            __syncthreads();
            if (tid == 1023) s_run = base + incl;
            __syncthreads();
        }
        if (tid == 0) sc.boff[a.n_blocks] = s_run;
    }
    __syncthreads();
    const int n_active = s_run;
    if (tid == 0) {
        if (closing) {
            PassRecord &r = sc.rec[sa.prev];
            r.formed = (long long)a.exch[a.bit_words + CNT_FORMED], r.exact = (long long)a.exch[a.bit_words + CNT_EXACT];
            r.screened = (long long)a.exch[a.bit_words + CNT_SCREENED], r.evaluated = (long long)a.exch[a.bit_words + CNT_EVALUATED];
            r.removed = (long long)(n_before - n_active);
            r.n_after = n_active;
            if (sa.prev_algo >= 0) r.algo = sa.prev_algo;
        }
        sn->n_active = n_active;
        sn->bitsel = closing ? sel ^ 1 : sel;
        sn->cull_on = 0;
        for (int w = 0; w < 8; ++w) a.exch[a.bit_words + w] = 0;
        int on = 0;
        if (sa.cur >= 0) {
            on = (sa.k_cur == 1 || 20 * sa.k_cur < (long long)n_active) ? 1 : 0;  // rmsd_pruning.py:192
            PassRecord &r = sc.rec[sa.cur];
            r.k = sa.k_cur, r.n_before = n_active, r.n_after = n_active, r.on = on, r.algo = sa.algo_cur;
            r.formed = r.exact = r.screened = r.evaluated = r.removed = r.known = 0;
        }
        sn->pass_on = on;
        sn->ticket = 0;
        if (a.next_s_lo < 0) sn->A = n_active, sn->row_lo = 0;
    }
    if (a.next_s_lo >= 0 && wv == 0) {  // (boff and the new bit copy were written by this block, before the barriers above)
        const unsigned long long *Xn = closing ? Xo : X;
        const int lo = rank_below_wave(sc.boff, Xn, a.n_blocks, n_active, a.next_s_lo), hi = rank_below_wave(sc.boff, Xn, a.n_blocks, n_active, a.next_s_hi);
        if (lane == 0) sn->row_lo = lo, sn->A = hi - lo;
    }
}

// Summary words of `count` cache views (one bit per 1024 view bits, CacheViews) rebuilt from their bits: after the host has
// summed the views of the remaining passes over the ranks, the summed summary words mean nothing.
inline __global__ __launch_bounds__(256) void k_views_summaries(unsigned long long *__restrict__ views, long long stride, int bit_words, int dsum_words, int count) {
    // one thread per summary BIT (16 view words); the 64 bits of a summary word sit in one wavefront and meet by ballot
    const int per_view = dsum_words * 64;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < int64_t(count) * per_view; e += int64_t(gridDim.x) * blockDim.x) {
        const int v = int(e / per_view), sb = int(e - int64_t(v) * per_view);
        unsigned long long *bits = views + int64_t(v) * stride;
        const int64_t w0 = int64_t(sb) * 16;
        unsigned long long any = 0;
        if (w0 < bit_words) {
#pragma unroll
            for (int u = 0; u < 16; ++u) any |= (w0 + u < bit_words) ? bits[w0 + u] : 0ull;
        }
        const unsigned long long word = __ballot(any != 0);
        if ((threadIdx.x & 63) == 0) bits[bit_words + (sb >> 6)] = word;
    }
}

// End of a run: the pass records and (optionally) the survivor mask go to host-visible memory from ONE small launch instead
// of two copy commands.  `rec_host` and `mask_host` are pinned host allocations mapped into the device's address space.
inline __global__ __launch_bounds__(256) void k_export_run(const unsigned long long *__restrict__ rec, int rec_words, unsigned long long *__restrict__ rec_host,
                                                     const unsigned long long *__restrict__ mask, int64_t mask_words, const uint8_t *__restrict__ mask_bytes,
                                                     int64_t n, unsigned long long *__restrict__ mask_host, const unsigned *__restrict__ dmax_bits) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t e = tid; e < rec_words; e += stride) rec_host[e] = rec[e];
    if (tid == 0) rec_host[rec_words] = dmax_bits ? (unsigned long long)*dmax_bits : 0ull;  // (behind the records: did the descriptor build meet a non-finite structure)
    if (mask_host) {
        for (int64_t e = tid; e < mask_words; e += stride) mask_host[e] = mask[e];
        uint8_t *tail = reinterpret_cast<uint8_t *>(mask_host);
        for (int64_t b = mask_words * 8 + tid; b < n; b += stride) tail[b] = mask_bytes[b];
    }
}

}  // namespace tsc
