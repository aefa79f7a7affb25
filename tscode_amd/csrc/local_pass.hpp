// local_pass.hpp -- a whole pass of prune_conformers_rmsd in ONE launch, for passes whose chunks are short.
//
// A pass only ever compares structures of the same chunk (tscode/rmsd_pruning.py:136-147), so when the longest chunk of
// a pass holds at most LP_MAX_ROWS structures a workgroup can own a chunk end to end: it ranks the chunk's active
// structures (the mask bits, by ballot), finds every row's stop column in the cache view, screens and evaluates the
// pairs, and applies the verdicts (mask, cache keys, scan counts, statistics) -- the work of k_open_rows, k_rmsd_sieve and the
// tile-wise apply without the kernel boundary in between.  The host takes this path for passes
// whose chunks are a few row tiles long and for small ensembles (see tsc_prune_pass_local), where a pass is bound by
// launch latency, not by work.
//
// Long chunks are shared: block j of the NB blocks of a chunk takes the row tiles j, j + NB, ... (rows of a pass are
// independent, :92,101-113); every block of a chunk repeats the cheap ranking, only its own rows go further.
// Same verdict functions as the big kernel (sieve.hpp): descriptor screen -> H -> quartic tests -> explicit rotation.
//
// Two forms of the screen, two kernels (template <bool MM>, a register allocation each; the host picks by "sieve_mm16", options.hpp: the option of the 16-row matrix-core screen):
//   MM = false  the packed-fp32 screen of sieve.hpp, one live row after the other against 64 columns (the rows' descriptors in LDS, the
//               columns' double-buffered in registers): about 30 vector instructions per row and step.
//   MM = true   the matrix-core screen of mm.hpp (level 1: v_mfma_f32_16x16x16_f16 on float16 records, screen_limit_mm): a step of 64
//               columns is four blocks of 16 against the tile's 16 rows -- 8 MFMAs, 32 v_alignbit_b32 that gather the sign bits, and an
//               extraction loop that takes one candidate per lane and turn.  The records are read BY STRUCTURE INDEX from a buffer of the
//               run's own (LocalPassArgs::rec), written once per run: by k_init_run where the descriptors are final before the run is set
//               up (the fused pipeline, descriptors of tsc_embed_masked_dev), by k_mm_records behind the descriptor build otherwise
//               (prune.hip).  k_open_rows' records by POSITION are not this kernel's: it has no opener.  The rows' operands wait in
//               the LDS area the other form keeps its rows in, ONE column step is in registers, requested where it is used: anything
//               more that lives around the evaluation stages is spilled (MEASURED.md section 28 has the forms that were tried).
//               The float16 rounding lets a per cent or so more pairs through than the fp32 screen and queues a step's candidates in
//               another order: pairs_computed, pairs_screened and the batch counts differ between the forms; verdicts, masks, cache
//               keys and pairs_evaluated do not (tests/test_local_pass_mm.py).
#pragma once
#include "mm.hpp"
#include "shapes.hpp"
#include "sieve.hpp"

namespace tsc {

// (LP_MAX_ROWS, LP_TI and LP_TILES_PER_BLOCK: shapes.hpp)
constexpr int LP_WAVES = 4;
constexpr int LP_THREADS = LP_WAVES * 64;
constexpr int LP_QCAP = LP_TI * 64 + 64;
constexpr int LP_WORDS = LP_MAX_ROWS / 64;
constexpr int LP_TICKET_GROUPS = 16;  // two-level ticket: same-address atomics serialise (~12 ns each)
#ifndef TSC_LP_OCC
#define TSC_LP_OCC 4
#endif
constexpr int LP_OCCUPANCY = TSC_LP_OCC;  // workgroups per CU the register allocation aims at (unbounded, the kernel takes 255 VGPRs: one)

struct LocalPassArgs {
    int h;
    int use_cache;
    int nb_regular;  // blocks per chunk for chunks 0 .. k-2
    int nb_last;     // blocks of the last chunk (it takes the remainder, :141-142)
    int c_lo;        // first chunk of this launch and how many regular chunks (not the last one of the pass) follow it: 0 and k - 1,
    int n_reg;       // unless the pass is partitioned over ranks (rmsd.hpp, k_pass_merge): then this rank's chunks; blocks beyond
                     // n_reg * nb_regular belong to the last chunk of the pass
    unsigned long long *exch;  // rank-partitioned pass (else null): removed rows are noted here and applied by k_pass_merge
    double thr, maxdev_thr, half_h_thr2, two_thr2, desc_limit;
    const unsigned *dmax_bits;
    const _Float16 *rec;       // the MM form: the float16 records of the matrix-core screen (mm_record.hpp) by STRUCTURE index, written once per run
    unsigned long long *dbg;   // -DTSC_DBG_STAMPS builds only: 8 time stamps per wavefront of the launch (tools/stamps.py), else null
};

struct LocalTickets {  // zeroed by k_init_run and again by the wavefront that closes a pass
    unsigned group[LP_TICKET_GROUPS][32];  // one counter per 128-byte line
    unsigned top;
    unsigned pad[31];
};

// -DTSC_DBG_STAMPS builds: slot 2 = the wavefront enters its first evaluation stage, 4 = it has left its last one, 6 (a pass left open
// does not use it) = how many sign batches it ran + 65536 * how many exact batches
#ifdef TSC_DBG_STAMPS
#define LP_STAGE_IN(exact)                                \
    do {                                                  \
        if (!n_stages) TSC_STAMP(2);                      \
        n_stages += (exact) ? 65536 : 1;                  \
    } while (0)
#define LP_STAGE_OUT() TSC_STAMP(4)
#define LP_STAGE_COUNT()                                                                                                             \
    do {                                                                                                                             \
        if (a.dbg && (threadIdx.x & 63) == 0) a.dbg[size_t(blockIdx.x) * 32 + (threadIdx.x >> 6) * 8 + 6] = (unsigned long long)n_stages; \
    } while (0)
#else
#define LP_STAGE_IN(exact) do { } while (0)
#define LP_STAGE_OUT() do { } while (0)
#define LP_STAGE_COUNT() do { } while (0)
#endif

__device__ inline unsigned long long lds_extract64(const unsigned long long *bits, int start) {
    const int w = start >> 6, sh = start & 63;
    const unsigned long long lo = bits[w] >> sh;
    const unsigned long long hi = sh ? (bits[w + 1] << (64 - sh)) : 0ull;
    return lo | hi;
}

// views_insert_wave (pass_state.hpp) for this kernel, whose launch is as long as its slowest workgroup's chain: the same bits in the same words,
// but ONE round trip for the summary words of all later views instead of one per view.  The bit of a key goes out as it is found (no
// answer is waited for); the summary word of view j -- a load, and an or only where a bit is missing: thousands of rows would else or the
// same word -- is left to lane j - cv.first, and the lanes go for their words together behind the loop.  Rows of one tile lie in one
// chunk, so their keys share a summary word unless the chunk straddles a multiple of 65 536 structures: such a second word is dealt with
// on the spot, as pass_state.hpp does.
__device__ inline void lp_views_insert_wave(const CacheViews &cv, bool removed, int a, int b) {
    if (__ballot(removed) == 0) return;
    const int lane = threadIdx.x & 63;
    static_assert(MAX_SLOTS <= 64, "a lane per later view");
    long long my_word = -1;
    unsigned long long my_sb = 0ull;
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
        for (bool primary = true; left; primary = false) {
            const int leader = __ffsll((long long)left) - 1;
            const int word = __shfl(b >> 16, leader);
            const bool same = ok && (b >> 16) == word;
            unsigned long long sb = same ? 1ull << ((b >> 10) & 63) : 0ull;
            for (int off = 32; off > 0; off >>= 1) sb |= __shfl_xor(sb, off);
            if (primary) {
                if (lane == j - cv.first) my_word = int64_t(j) * cv.stride + cv.bit_words + word, my_sb = sb;
            } else if (lane == leader) {
                unsigned long long *ds = v + cv.bit_words + word;
                if ((__hip_atomic_load(ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & sb) != sb) atomicOr(ds, sb);
            }
            left &= ~__ballot(same);
        }
    }
    if (my_sb) {
        unsigned long long *ds = cv.views + my_word;
        if ((__hip_atomic_load(ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & my_sb) != my_sb) atomicOr(ds, my_sb);
    }
}

constexpr int LP_MM_BLOCKS = 64 / MM_STEP;  // the MM form: 16-column blocks of a column step

template <bool MM>
inline __global__ __launch_bounds__(LP_THREADS, LP_OCCUPANCY) void k_pass_chunks(PassGeom g, LocalPassArgs a, PruneState *__restrict__ st, uint8_t *__restrict__ mask,
                                                             unsigned long long *__restrict__ bits, int bit_words,
                                                             const unsigned long long *__restrict__ dbit, const double *__restrict__ heavy,
                                                             const double *__restrict__ Gall, const float *__restrict__ D,
                                                             CacheViews cv, PassCounters *__restrict__ cnt, int32_t *__restrict__ bsum, int block_items,
                                                             StepCtx sc, StepArgs next, LocalTickets *__restrict__ tickets, DeriveArgs dv) {
    __shared__ unsigned long long s_mb[LP_WORDS + 2], s_db[LP_WORDS + 2];
    __shared__ unsigned short s_wpre[LP_WORDS + 2];
    __shared__ unsigned short s_act[LP_MAX_ROWS], s_cend[LP_MAX_ROWS];
    __shared__ int s_best[LP_MAX_ROWS];
    __shared__ unsigned short s_queue[LP_WAVES][LP_QCAP], s_exq[LP_WAVES][128];
    __shared__ __attribute__((aligned(16))) float s_rowdesc[LP_WAVES][LP_TI * DW];  // (the MM form: a tile's row operands, 16 bytes per lane)
    __shared__ double s_jacobi[LP_WAVES][32];  // the Jacobi fallback of the exact stage (pair_math.hpp: top_eigvec4_mem), per wavefront
    __shared__ unsigned long long s_stat[8];  // block totals of the five statistics
    __shared__ int s_A, s_anydb, s_last, s_open[2];
    static_assert(DW == 16 && LP_TI * DW == 256, "row staging: 4 rows x 16 components per 64 lanes");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    TSC_STAMP(0);  // the wavefront has started
    // which chunk, and which share of its row tiles
    int c, j, nb;
    {
        const int reg_blocks = a.n_reg * a.nb_regular;
        if (int(blockIdx.x) < reg_blocks) {
            c = int(blockIdx.x) / a.nb_regular, j = int(blockIdx.x) - c * a.nb_regular, nb = a.nb_regular;
            c += a.c_lo;
        } else {
            c = g.k - 1, j = int(blockIdx.x) - reg_blocks, nb = a.nb_last;
        }
    }
    const int first = c * g.cs;                                  // :140
    const int L = ((c == g.k - 1) ? g.n : first + g.cs) - first;  // :141-144  (<= LP_MAX_ROWS, checked by the host)
    const int nw = (L + 63) >> 6;
    // Requested in the round trip the state block takes, not behind it: the run's descriptor bound and this chunk's words of the cache
    // view and of BOTH bit copies of the mask (which of the two the pass reads is what the state block says; the other one is being
    // written by this launch and what was read of it is dropped).  All of it was final at the kernel boundary.
    static_assert(LP_WORDS <= LP_THREADS, "a thread per 64 structures of the chunk");
    const unsigned dmax_raw = *a.dmax_bits;
    // (the two words a chunk's 64 structures straddle, as they are: put together behind the round trip.  Every bit copy and view has
    // words to spare behind its last structure: prune.hip, bit_words)
    unsigned long long w_copy0[2] = {0ull, 0ull}, w_copy1[2] = {0ull, 0ull}, w_view[2] = {0ull, 0ull};
    if (tid < nw) {
        const int64_t w0 = (int64_t(first) >> 6) + tid;
        w_copy0[0] = bits[w0], w_copy0[1] = bits[w0 + 1];
        w_copy1[0] = bits[bit_words + w0], w_copy1[1] = bits[bit_words + w0 + 1];
        if (a.use_cache) w_view[0] = dbit[w0], w_view[1] = dbit[w0 + 1];
    }
    // the state block of this pass: written by whoever closed the pass before it, or -- that pass was left open (pass_state.hpp,
    // pass_derive) -- worked out here by every workgroup for itself.  The scan blocks' counts are being decremented by this very
    // launch: no prefix is derived from them here, the next kernel that opens a pass makes its own
    int open_on, open_sel;
    if (dv.prev_st) {
        if (wid == 0) {
            const Derived d = pass_derive(dv, st, blockIdx.x == 0, nullptr, 0, nullptr, nullptr);
            if (lane == 0) s_open[0] = d.pass_on, s_open[1] = d.bitsel;
        }
        __syncthreads();
        open_on = s_open[0], open_sel = s_open[1];
    } else {
        open_on = st->pass_on, open_sel = st->bitsel;
    }
    // (the same in every lane, and said so: what is worked out from them -- the bit copies' addresses, the tile counts -- stays scalar)
    open_on = __builtin_amdgcn_readfirstlane(open_on), open_sel = __builtin_amdgcn_readfirstlane(open_sel);
    const bool pass_on = open_on != 0;
    // the pass reads one bit copy of the mask and clears the rows it removes in the other (every row of a pass sees the mask
    // as it was when the pass began, rmsd_pruning.py:151-157, whatever order the workgroups run in)
    unsigned long long *mbit_next = bits + size_t(open_sel ^ 1) * bit_words;
    if (tid < 8) s_stat[tid] = 0;
    int n_eval = 0, n_exact = 0;  // pairs this wavefront formed H for / sent to the exact stage (wave-uniform: kept scalar)
    [[maybe_unused]] int n_stages = 0;
    int my_screened = 0;  // lanes 0..15 of a wavefront: pairs of its tiles' rows that went through the screen

    if (pass_on) {
        // ---- 1. the chunk's mask and cache view as bits; ranks of the active structures.  The other bit copy may lag one pass
        // behind (a superset of this one): and-ing this chunk's words into it brings it up to date, and commutes with the
        // bits other workgroups -- of this very chunk when it is shared -- clear there in step 4
        // (the words are here already: thread t holds word first / 64 + t and the one behind it, which the chunk's last thread adds
        // where the chunk reaches into it)
        if (j == 0 && !a.exch && tid < nw) {
            const int w0 = (first >> 6) + tid;
            atomicAnd(&mbit_next[w0], open_sel ? w_copy1[0] : w_copy0[0]);
            if (tid == nw - 1 && w0 + 1 <= ((first + L - 1) >> 6)) atomicAnd(&mbit_next[w0 + 1], open_sel ? w_copy1[1] : w_copy0[1]);
        }
        if (tid < nw) {
            const int sh = first & 63;  // (extract64 of pass_state.hpp on the words already here)
            auto join = [sh](const unsigned long long (&w)[2]) { return (w[0] >> sh) | (sh ? (w[1] << (64 - sh)) : 0ull); };
            unsigned long long m = open_sel ? join(w_copy1) : join(w_copy0), v = join(w_view);
            const int rem = L - 64 * tid;
            if (rem < 64) m &= (1ull << rem) - 1ull, v &= (1ull << rem) - 1ull;
            s_mb[tid] = m;
            s_db[tid] = v;
        }
        if (tid < 2) s_mb[nw + tid] = 0, s_db[nw + tid] = 0;
        __syncthreads();
        if (tid == 0) {
            int run = 0, any = 0;
            for (int w = 0; w < nw; ++w) {
                s_wpre[w] = (unsigned short)run;
                run += __popcll(s_mb[w]);
                any |= (s_db[w] != 0ull) ? 1 : 0;
            }
            s_wpre[nw] = (unsigned short)run;
            s_A = run, s_anydb = any;
        }
        __syncthreads();
        const int A = __builtin_amdgcn_readfirstlane(s_A);
        auto rank_of = [&](int t) { return int(s_wpre[t >> 6]) + __popcll(s_mb[t >> 6] & ((t & 63) ? (~0ull >> (64 - (t & 63))) : 0ull)); };
        for (int t = tid; t < L; t += LP_THREADS)
            if ((s_mb[t >> 6] >> (t & 63)) & 1ull) s_act[rank_of(t)] = (unsigned short)t;
        __syncthreads();
        // ---- 2. stop column of this block's rows (first active column whose key is cached, :65-67), best = none
        const int n_tiles = (A + LP_TI - 1) / LP_TI;
        const int my_tiles = n_tiles > j ? (n_tiles - j + nb - 1) / nb : 0;
        for (int idx = tid; idx < my_tiles * LP_TI; idx += LP_THREADS) {
            const int r = (j + (idx / LP_TI) * nb) * LP_TI + (idx % LP_TI);
            if (r >= A) continue;
            const int t = s_act[r];
            int found = L;
            if (s_anydb) {
                const int len = L - t - 1;  // candidate deltas d = 1 .. len
                for (int d0 = 1; d0 <= len; d0 += 64) {
                    unsigned long long w = lds_extract64(s_mb, t + d0) & lds_extract64(s_db, d0);
                    const int rem = len - d0 + 1;
                    if (rem < 64) w &= (1ull << rem) - 1ull;
                    if (w) {
                        found = t + d0 + __ffsll((long long)w) - 1;
                        break;
                    }
                }
            }
            s_cend[r] = (unsigned short)(found >= L ? A : rank_of(found));
            s_best[r] = INT_MAX;
        }
        __syncthreads();
        TSC_STAMP(1);  // ranked, stop columns found

        // ---- 3. pairs: one wavefront per (16 rows) x (all their columns), 64 columns at a time
        const int h3 = a.h * 3;
        [[maybe_unused]] const float limit32 = MM ? 0.0f : screen_limit32(__uint_as_float(dmax_raw), a.desc_limit);
        // (the same in every lane, and said so: a scalar register, not a vector one held through the evaluation stages)
        [[maybe_unused]] const float limit_mm = MM ? __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(screen_limit_mm(dmax_raw, a.desc_limit)))) : 0.0f;
        [[maybe_unused]] const int g4 = lane >> 4, rc = lane & 15;  // the MM form's lane: k group (slots 4 g4 .. 4 g4 + 3), row or column of a block
        // a lane's place among the set bits of a ballot: how many lanes below it are in
        auto place_in = [](unsigned long long m) __attribute__((always_inline)) {
            return int(__builtin_amdgcn_mbcnt_hi(unsigned(m >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m), 0u)));
        };
        unsigned short *queue = s_queue[wid], *exq = s_exq[wid];
        float *rowdesc = s_rowdesc[wid];
        double *jac = s_jacobi[wid];
        int tile_no = 0;
        for (int rt = j; rt < n_tiles; rt += nb, ++tile_no) {
            if ((tile_no % LP_WAVES) != wid) continue;  // this block's tiles are dealt round-robin to its wavefronts
            const int r0 = rt * LP_TI;
            const int nrows = min(LP_TI, A - r0);
            const int my_cend = lane < nrows ? int(s_cend[r0 + lane]) : 0;
            const bool live0 = lane < nrows && my_cend > r0 + lane + 1;
            unsigned alive = unsigned(__builtin_amdgcn_ballot_w64(live0));
            if (!alive) continue;
            int cmax = live0 ? my_cend : 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
            cmax = __builtin_amdgcn_readfirstlane(cmax);
            [[maybe_unused]] float row_part[4];  // (the rows' descriptors and the first column tile are requested together, the LDS stores come behind both)
            [[maybe_unused]] f16x4 Ar[NFAM];     // the MM form: the rows' operands, lane (g4, rc) holds row rc's slots
            if constexpr (MM) {
                const _Float16 *rr = a.rec + int64_t(first + s_act[min(r0 + rc, A - 1)]) * MM_REC_HALVES;
#pragma unroll
                for (int fam = 0; fam < NFAM; ++fam) Ar[fam] = mm_load_A(rr, fam, g4);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int rr = min(r0 + 4 * q + (lane >> 4), A - 1);
                    row_part[q] = D[int64_t(first + s_act[rr]) * DW + (lane & 15)];
                }
            }
            int qn = 0, qe = 0;

            // The two evaluation stages of the walked kernels (sieve.hpp), in this kernel's own form and with ONE call site each, in the
            // drain loop behind the column step: a stage's body holds H, the quartic or the rotation in float64, and every further copy
            // of it was another 5 - 10 KB of code and another set of values for the allocator to keep apart from the screen's.
            // A queue entry is (row of the tile << 12 | column rank); the structures are held as 32-bit indices, the pointers formed
            // where they are used.
            auto note_similar = [&](bool sim, int t, int col) __attribute__((always_inline)) {
                if (sim) atomicMin(&s_best[r0 + t], col);
                unsigned long long sm = __builtin_amdgcn_ballot_w64(sim);
                while (sm) {  // rows that found a similar column stop being screened (the reference returns there, :75-77)
                    const int l = __ffsll((long long)sm) - 1;
                    sm &= sm - 1;
                    alive &= ~(1u << __builtin_amdgcn_readlane(t, l));
                }
            };
            auto exact_stage = [&](int base, int cnt) __attribute__((always_inline)) {
                LP_STAGE_IN(true);
                int lpp = 64;
                while (lpp > 1 && 64 / lpp < cnt) lpp >>= 1;
                const int grp = lane / lpp, sub = lane - grp * lpp;
                bool sim = false, degenerate = false;
                int t = 0, col = 0;
                unsigned ent = 0;
                if (grp < cnt) {
                    ent = exq[base + grp];
                    t = int(ent >> 12), col = int(ent & 0xfffu);
                    const int i = first + s_act[r0 + t], jj = first + s_act[col];
                    const double *pp = heavy + int64_t(i) * h3, *pq = heavy + int64_t(jj) * h3;
                    const double Gi = Gall[i], Gj = Gall[jj];
                    double H[9], e[4];
                    pair_H(pp, pq, a.h, sub, lpp, H);
                    if (rotation_quaternion_fast(H, Gi, Gj, e)) {  // (the lanes of a group hold the same H: they branch together)
                        // (the entry is read and decoded AGAIN behind the quaternion -- a volatile read, so that it is: the two
                        // pointers and the pair's indices need no registers while the cofactors of the 4x4 are worked out, which is
                        // where this kernel runs out of them)
                        const unsigned ent2 = reinterpret_cast<const volatile unsigned short *>(exq)[base + grp];
                        t = int(ent2 >> 12), col = int(ent2 & 0xfffu);
                        const int i2 = first + s_act[r0 + t], j2 = first + s_act[col];
                        double rm, md;
                        residual_rmsd_maxdev(heavy + int64_t(i2) * h3, heavy + int64_t(j2) * h3, a.h, e, rm, md, sub, lpp);
                        sim = sub == 0 && rm < a.thr && md < a.maxdev_thr;  // rmsd_pruning.py:75
                    } else {
                        degenerate = sub == 0;
                    }
                }
                note_similar(sim, t, col);
                // A pair whose top eigenvalue is degenerate needs the Jacobi eigen-solver.  In registers its two 4x4 matrices are 64
                // VGPRs in every lane of every batch (and were this kernel's scratch); as in the walked kernels the whole wavefront
                // takes such a pair on instead, one at a time: H by all 64 lanes, the solver by lane 0 on an LDS area, the residual
                // by all lanes again.
                for (unsigned long long dm = __builtin_amdgcn_ballot_w64(degenerate); dm; dm &= dm - 1) {
                    const unsigned e1 = unsigned(__builtin_amdgcn_readlane(int(ent), __ffsll((long long)dm) - 1));
                    const int t2 = int(e1 >> 12), col2 = int(e1 & 0xfffu);
                    const int i = first + s_act[r0 + t2], jj = first + s_act[col2];
                    const double *pp = heavy + int64_t(i) * h3, *pq = heavy + int64_t(jj) * h3;
                    double H[9], e[4], rm, md;
                    pair_H(pp, pq, a.h, lane, 64, H);
                    if (lane == 0) {
                        horn_matrix(H, jac);
                        top_eigvec4_mem(jac, jac + 16, e);
                        jac[0] = e[0], jac[1] = e[1], jac[2] = e[2], jac[3] = e[3];
                    }
                    __builtin_amdgcn_wave_barrier();
                    e[0] = jac[0], e[1] = jac[1], e[2] = jac[2], e[3] = jac[3];
                    __builtin_amdgcn_wave_barrier();
                    residual_rmsd_maxdev(pp, pq, a.h, e, rm, md, lane, 64);
                    if (rm < a.thr && md < a.maxdev_thr) {  // wave-uniform
                        if (lane == 0) atomicMin(&s_best[r0 + t2], col2);
                        alive &= ~(1u << t2);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                LP_STAGE_OUT();
            };
            auto sign_stage = [&](int base, int cnt) __attribute__((always_inline)) {
                LP_STAGE_IN(false);
                int lpp = 64;
                while (lpp > 1 && 64 / lpp < cnt) lpp >>= 1;
                const int grp = lane / lpp, sub = lane - grp * lpp;
                bool cand = false, sim = false;
                unsigned e = 0;
                int t = 0, col = 0;
                if (grp < cnt) {
                    e = queue[base + grp];
                    t = int(e >> 12), col = int(e & 0xfffu);
                    const int i = first + s_act[r0 + t], jj = first + s_act[col];
                    const double half_sum = 0.5 * (Gall[i] + Gall[jj]);
                    double H[9];
                    pair_H(heavy + int64_t(i) * h3, heavy + int64_t(jj) * h3, a.h, sub, lpp, H);
                    const int verdict = pair_verdict(H, half_sum, a.half_h_thr2, a.two_thr2, a.h);
                    cand = sub == 0 && verdict == PAIR_UNDECIDED;
                    sim = sub == 0 && verdict == PAIR_SIMILAR;
                }
                note_similar(sim, t, col);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(cand);
                if (m) {
                    if (cand) exq[qe + place_in(m)] = (unsigned short)e;
                    qe += __popcll(m);
                }
                n_eval = __builtin_amdgcn_readfirstlane(n_eval + cnt);
                n_exact = __builtin_amdgcn_readfirstlane(n_exact + __popcll(m));
                __builtin_amdgcn_wave_barrier();
                LP_STAGE_OUT();
            };

            // column tiles are double-buffered: the gather of the next tile is in flight while this one is screened
            auto load_cols = [&](int c0, f32x2 (&dst)[KD]) __attribute__((always_inline)) {
                const f32x4 *src = reinterpret_cast<const f32x4 *>(D + int64_t(first + s_act[min(c0 + lane, A - 1)]) * DW);
#pragma unroll
                for (int k = 0; k < KD / 2; ++k) {
                    const f32x4 v = src[k];
                    dst[2 * k] = f32x2{v.x, v.y};
                    dst[2 * k + 1] = f32x2{v.z, v.w};
                }
            };
            // the MM form: a step's 64 columns as four blocks of 16, lane (g4, rc) holds column rc of every block -- four 16-byte loads per
            // lane, the bytes of load_cols
            auto load_recs = [&](int c0, f16x4 (&dst)[LP_MM_BLOCKS][NFAM]) __attribute__((always_inline)) {
#pragma unroll
                for (int b = 0; b < LP_MM_BLOCKS; ++b)
                    mm_load_B2(a.rec + int64_t(first + s_act[min(c0 + MM_STEP * b + rc, A - 1)]) * MM_REC_HALVES, g4, dst[b]);
            };
            // ... the rows' operands wait in LDS (where the other form keeps its rows), NOT in registers: whatever lives through the
            // evaluation stages costs this kernel a spill.  A step reads them back with one 16-byte read; rows that are not (or no longer)
            // looking then get +inf in the n0 slot of family 0 (mm.hpp: mark_rows of sieve_item_mm16), from `alive` as it is at that step
            static_assert(NFAM == 2 && LP_TI * DW == 64 * 4, "a lane's two operands are the 16 bytes at its place in the row area");
            auto put_rows = [&]() __attribute__((always_inline)) {
                const f32x2 lo = __builtin_bit_cast(f32x2, Ar[0]), hi = __builtin_bit_cast(f32x2, Ar[1]);
                *reinterpret_cast<f32x4 *>(rowdesc + 4 * lane) = f32x4{lo.x, lo.y, hi.x, hi.y};
            };
            auto get_rows = [&]() __attribute__((always_inline)) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(rowdesc + 4 * lane);
                const f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
                Ar[0] = __builtin_bit_cast(f16x4, lo), Ar[1] = __builtin_bit_cast(f16x4, hi);
                if (g4 == 2 && !((alive >> rc) & 1u)) Ar[0][0] = _Float16(__builtin_inff());
            };
            [[maybe_unused]] f32x2 dq[KD], dq_next[KD];
            [[maybe_unused]] f16x4 Bq[LP_MM_BLOCKS][NFAM];
            int c0 = (r0 + 1) & ~63;  // (< cmax: a live row's stop column lies beyond its own rank)
            if constexpr (MM) {
                put_rows();
            } else {
                load_cols(c0, dq_next);
#pragma unroll
                for (int q = 0; q < 4; ++q) rowdesc[64 * q + lane] = row_part[q];
            }
            __builtin_amdgcn_wave_barrier();
            for (bool screening = true;;) {
                if constexpr (MM) {
                    if (screening) {
                        // ONE column step, requested where it is used.  A second buffer in flight during the step (as dq / dq_next), or this
                        // one requested at the bottom of the loop, lives -- for the register allocator -- around the stages: 29 to 70 spilled
                        // registers and 72 to 128 bytes of scratch, the loads among them.  The step itself is 8 MFMAs and an extraction that
                        // rarely iterates: next to the gather's round trip there is little to hide it behind, the SIMD's other wavefronts do.
                        load_recs(c0, Bq);
                        const bool here = lane < nrows && ((alive >> lane) & 1u) && my_cend > c0 && r0 + lane < c0 + 63;
                        my_screened += here ? max(0, min(my_cend, c0 + 64) - max(r0 + lane + 1, c0)) : 0;
                        get_rows();
                        // 16 rows x 64 columns x two families: 8 MFMAs.  Every accumulator starts at -limit, a pair is kept iff BOTH families
                        // come out negative; the sign bits go into a mask per family, value j = 4 b + i of the step -- row 4 g4 + i, column
                        // 16 b + rc -- at bit 15 - j (mm.hpp)
                        unsigned m0 = 0, m1 = 0;
#pragma unroll
                        for (int b = 0; b < LP_MM_BLOCKS; ++b) {
                            const f32x4 z = {-limit_mm, -limit_mm, -limit_mm, -limit_mm};
                            const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x16f16(Ar[0], Bq[b][0], z, 0, 0, 0);
                            const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x16f16(Ar[1], Bq[b][1], z, 0, 0, 0);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                m0 = __builtin_amdgcn_alignbit(m0, __float_as_uint(s0[i]), 31);
                                m1 = __builtin_amdgcn_alignbit(m1, __float_as_uint(s1[i]), 31);
                            }
                        }
                        static_assert(4 * LP_MM_BLOCKS == 16, "16 values per lane and family: moved to the top half for the count of leading zeros");
                        unsigned hits = (m0 & m1) << 16;
                        while (__builtin_amdgcn_ballot_w64(hits != 0u)) {
                            // one pair per lane and turn (a lane rarely holds two); kept if it lies right of the diagonal, before its row's stop
                            // column, and its row is still looking (clamped columns beyond the active count fail the second test)
                            bool keep = false;
                            unsigned ent = 0;
                            if (hits) {
                                const int jv = __builtin_clz(hits);
                                hits &= ~(0x80000000u >> jv);
                                const int row = 4 * g4 + (jv & 3), col = c0 + MM_STEP * (jv >> 2) + rc;
                                keep = col > r0 + row && ((alive >> row) & 1u) && col < int(s_cend[r0 + row]);
                                ent = (unsigned(row) << 12) | unsigned(col);
                            }
                            const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
                            if (keep) queue[qn + place_in(km)] = (unsigned short)ent;
                            qn += __popcll(km);
                        }
                        c0 += 64;
                        alive &= ~unsigned(__builtin_amdgcn_ballot_w64(lane < nrows && ((alive >> lane) & 1u) && my_cend <= c0));  // rows whose range ends here
                        __builtin_amdgcn_wave_barrier();
                    }
                } else if (screening) {
                    const int col = c0 + lane;
#pragma unroll
                    for (int k = 0; k < KD; ++k) dq[k] = dq_next[k];
                    if (c0 + 64 < cmax) load_cols(c0 + 64, dq_next);
                    const bool here = lane < nrows && ((alive >> lane) & 1u) && my_cend > c0 && r0 + lane < c0 + 63;
                    unsigned rows = unsigned(__builtin_amdgcn_ballot_w64(here));
                    // (columns of this tile inside every live row's range: counted once per tile by the rows' own lanes, not by
                    // seven scalar instructions per row -- sieve.hpp)
                    my_screened += here ? max(0, min(my_cend, c0 + 64) - max(r0 + lane + 1, c0)) : 0;
                    while (rows) {
                        const int t = __ffs(rows) - 1;
                        rows &= rows - 1;
                        const int r = r0 + t;
                        const int ce = __builtin_amdgcn_readlane(my_cend, t);
                        const f32x2 *dr = reinterpret_cast<const f32x2 *>(rowdesc + t * DW);
                        f32x2 s2 = {0.0f, 0.0f};
#pragma unroll
                        for (int k = 0; k < KD; ++k) {
                            const f32x2 d = dr[k] - dq[k];
                            s2 = __builtin_elementwise_fma(d, d, s2);
                        }
                        const bool pass = col > r && col < ce && !(fmaxf(s2.x, s2.y) > limit32);
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
                        if (m) {
                            if (pass) queue[qn + place_in(m)] = (unsigned short)((unsigned(t) << 12) | unsigned(col));
                            qn += __popcll(m);
                        }
                    }
                    c0 += 64;
                    __builtin_amdgcn_wave_barrier();
                }
                // The drain.  Between column steps: sign batches of 64 from the queue's top while it holds as many, and an exact batch
                // of 64 as soon as one has gathered (qe < 64 before a sign batch adds at most 64: s_exq holds 128).  Behind the last
                // column step (screening false): the sign queue's rest, a full exact batch if that made one, the exact queue's rest.
                auto pending = [&]() __attribute__((always_inline)) { return qe >= 64 || qn >= 64 || (!screening && (qn | qe) != 0); };
                if (pending()) {
                    do {
                        if (qe >= 64 || qn == 0) {
                            const int cnt = min(qe, 64);
                            exact_stage(qe - cnt, cnt);
                            qe -= cnt;
                        } else {
                            const int cnt = min(qn, 64);
                            sign_stage(qn - cnt, cnt);
                            qn -= cnt;
                        }
                        if constexpr (MM) alive = unsigned(__builtin_amdgcn_readfirstlane(int(alive)));  // (see below)
                    } while (pending());
                    if (!screening) break;
                    // (the next tile is requested again behind a drain, clamped like any tile: its 32 registers are the stages' to use)
                    if constexpr (!MM) load_cols(c0, dq_next);
                } else if (!screening) {
                    break;
                }
                // (`alive` is the same in every lane -- the stages lower it by rows found with a ballot or in branches the whole wavefront takes --
                // but not provably so: said here, the loop's branches are scalar and what a step loads does not have to outlive the stages
                // lane by lane)
                if constexpr (MM) alive = unsigned(__builtin_amdgcn_readfirstlane(int(alive)));
                screening = c0 < cmax && alive;
            }
        }
        for (int off = 8; off > 0; off >>= 1) my_screened += __shfl_xor(my_screened, off);
        const unsigned long long n_screened = (unsigned long long)my_screened;
        TSC_STAMP(3);  // this wavefront's pairs evaluated
        __syncthreads();

        // ---- 4. apply this block's rows: mask, one cache key per removed row (:69-73), scan counts, evaluation count
        unsigned long long n_evaluated = 0, n_removed = 0;
        for (int rt = j; rt < n_tiles; rt += nb) {
            const int r = rt * LP_TI + lane;  // one wavefront per tile keeps the ballots simple; tiles dealt as above
            if (((rt - j) / nb) % LP_WAVES != wid) continue;
            bool removed = false;
            int my_block = -1, delta = 0;
            unsigned long long ev = 0;
            if (lane < LP_TI && r < A) {
                const int b = s_best[r];
                if (b != INT_MAX) {
                    const int t_r = s_act[r], t_b = s_act[b];
                    if (a.exch) {
                        atomicOr(&a.exch[(first + t_r) >> 6], 1ull << ((first + t_r) & 63));
                    } else {
                        mask[first + t_r] = 0;
                        atomicAnd(&mbit_next[(first + t_r) >> 6], ~(1ull << ((first + t_r) & 63)));
                        my_block = (first + t_r) / block_items;
                    }
                    delta = t_b - t_r;
                    removed = true;
                    ev = (unsigned long long)(b - r);  // columns r+1 .. b were evaluated
                } else {
                    ev = (unsigned long long)(int(s_cend[r]) - r - 1);  // every active column before the stop column
                }
            }
            for (unsigned long long left = __builtin_amdgcn_ballot_w64(removed && my_block >= 0); left;) {
                const int l = __ffsll((long long)left) - 1;
                const int blk = __shfl(my_block, l);
                const unsigned long long same = __builtin_amdgcn_ballot_w64(removed && my_block == blk);
                if (lane == l) atomicSub(&bsum[blk], __popcll(same));
                left &= ~same;
            }
            const int n_rm = __popcll(__builtin_amdgcn_ballot_w64(removed));
            lp_views_insert_wave(cv, removed, first, first + delta);  // the cache keys (:69-73), where later passes will look for them
            for (int off = 32; off > 0; off >>= 1) ev += __shfl_down(ev, off);
            n_evaluated += ev, n_removed += (unsigned long long)n_rm;
        }
        // ---- 5. statistics: one set of atomics per block
        if (lane == 0) {
            if (n_eval) atomicAdd(&s_stat[CNT_FORMED], (unsigned long long)n_eval);
            if (n_exact) atomicAdd(&s_stat[CNT_EXACT], (unsigned long long)n_exact);
            if (n_screened) atomicAdd(&s_stat[CNT_SCREENED], n_screened);
            if (n_evaluated) atomicAdd(&s_stat[CNT_EVALUATED], n_evaluated);
            if (n_removed) atomicAdd(&s_stat[CNT_REMOVED], n_removed);
        }
        __syncthreads();
        if (tid < 5) count_add(cnt, blockIdx.x, tid, s_stat[tid]);
    }

    // ---- 6. the last block closes this pass and opens the next (as k_apply_pass does); two-level ticket.  tickets = null: the pass
    // is left open, the first kernel of the next one closes it behind the kernel boundary (pass_derive)
    if (!tickets) {
        TSC_STAMP(5);
        LP_STAGE_COUNT();
        return;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    TSC_STAMP(5);  // this block's rows applied, its statistics added
    if (tid == 0) {
        int last = 0;
        const unsigned grp = blockIdx.x % LP_TICKET_GROUPS;
        const unsigned in_group = (gridDim.x - grp + LP_TICKET_GROUPS - 1) / LP_TICKET_GROUPS;
        if (atomicAdd(&tickets->group[grp][0], 1u) == in_group - 1) {
            const unsigned groups = min(unsigned(LP_TICKET_GROUPS), gridDim.x);
            last = (atomicAdd(&tickets->top, 1u) == groups - 1) ? 1 : 0;
        }
        s_last = last;
    }
    __syncthreads();
    TSC_STAMP(6);  // arrived at the pass's counter
    if (s_last && tid < 64) {
        pass_step_wave(sc, next);  // (zeroes the tickets as well)
        TSC_STAMP(7);  // pass closed
    }
}

}  // namespace tsc
