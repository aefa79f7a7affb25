// sieve.hpp -- K3 with a rotation-invariant descriptor sieve (descriptor.hpp) in front of the Kabsch evaluation (pair_stages.hpp): the
// packed-fp32 pair kernel of a pass and what the other pair kernels share with it (SieveArgs, FusedApply).  k_rmsd_sieve is a template:
// pairs_sieve.hip and pairs_sieve_plain.hip instantiate it, including this header emits nothing.
//
// Pass kernel (k_rmsd_sieve): one wavefront = 16 rows x one column segment, lane = CPL columns of a tile.
//   screen : descriptors are read by position from a copy in active order that k_open_rows writes on its way (one float4
//            per lane of its 4 lanes per row), so no index load stands in front of a column tile; the two families of a
//            component sit side by side, so one v_pk_add_f32 + one v_pk_fma_f32 advance both
//            distances; the 16 row descriptors sit in LDS and are read as broadcasts; ONE compare per (row, tile) decides
//            whether any column is within the limit; survivors go to a per-wavefront LDS queue (ballot + prefix popcount);
//   drain  : stage 1, whenever the queue holds 64 pairs (or at the end, spread over several lanes per pair): H from the
//            two structures in memory, the quartic tests (reject / accept near-duplicates / undecided);
//            stage 2, the explicit rotation for the undecided, when 64 have gathered or at the end;
//            atomicMin(best[row], column);
//   apply  : (single-rank runs) the work item that finishes a row tile last removes the tile's rows that found a similar
//            column and enters their cache keys into the views of the later passes; the last tile of the pass closes it.
// Any number of heavy atoms is supported (no register-resident structure).
#pragma once
#include "common.hpp"
#include "descriptor.hpp"
#include "pair_stages.hpp"
#include "pass_state.hpp"

namespace tsc {

struct SieveArgs {
    int n;   // upper bound of the active count the grid was sized for (structures of the run)
    int h;
    int tile_begin;
    int tile_stride;
    int seg_cols;
    double thr, maxdev_thr;
    double half_h_thr2;   // h * thr^2 / 2
    double two_thr2;      // 2 thr^2 when the near-duplicate test applies (h >= 4), else -1
    int drain_min;        // queue length that triggers a drain between column tiles (1..64)
    const int32_t *tile_cmax;   // device: per row tile a pair -- [2 t] the largest stop column of its 16 rows, [2 t + 1] the smallest first column of its
                                // rows that have columns left (k_open_rows; 0 where the pass's rows start behind their diagonal)
    const int32_t *cbeg;        // device: per row, the first column the pass still has to look at -- the columns before it were found dissimilar by
                                // an earlier pass (k_open_rows, known[]); r + 1 where the pass does not skip.  A HINT: a kernel that ignores it and
                                // the tiles' smallest evaluates known pairs again, to the same verdicts
    const unsigned *dmax_bits;  // device: largest |descriptor component| of the run (bit pattern of a float), see screen_limit32
    double desc_limit;          // h thr^2: exact squared descriptor distance above which a pair is certainly dissimilar
    const float *heavy32;       // float32 copy of the heavy atoms (heavy32_pitch(h) floats per structure), or null: stage 1 in float64 only
    unsigned long long *dbg;    // -DTSC_DBG_STAMPS builds only: 8 time stamps per wavefront of the launch (tools/stamps.py), else null
};

#ifdef TSC_DBG_STAMPS   // measurement hook: where a wavefront of the pair kernel spends its time (100 MHz wall clock)
#define TSC_STAMP(i)                                                                                                                  \
    do {                                                                                                                              \
        if (a.dbg) {                                                                                                                  \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                               \
            if ((threadIdx.x & 63) == 0)                                                                                              \
                a.dbg[(size_t(blockIdx.y) * gridDim.x + blockIdx.x) * 32 + (threadIdx.x >> 6) * 8 + (i)] = wall_clock64();             \
        }                                                                                                                             \
    } while (0)
#else
#define TSC_STAMP(i) do { } while (0)
#endif

#ifndef TSC_SIEVE_OCC2
#define TSC_SIEVE_OCC2 5
#endif
#ifndef TSC_SIEVE_OCC1
#define TSC_SIEVE_OCC1 6
#endif
// What the pair kernel of a single-rank run does when the LAST work item of a row tile finishes: it applies the tile's
// verdicts (apply_wave_rows, pass_state.hpp) -- no k_apply_pass launch behind the pair kernel.  tickets = null: that is all, the pass is
// left open and the first kernel of the next pass closes it (pass_state.hpp, pass_derive).  Otherwise (a rank-partitioned pass) the tile
// that was the last of the pass closes it (pass_step_wave).  Work items of a tile = its column segments that start
// below the tile's largest stop column (the others leave at their first test and do not count).
struct FusedApply {
    ApplyArgs ap;
    int32_t *tile_done;  // arrivals per row tile (zero between passes)
    PassTickets *tickets;
    unsigned n_tiles;    // blocks of k_open_rows = row tiles that arrive, here or there
    StepCtx sc;
    StepArgs next;
};

template <int TI, int CPL, bool TRIM, bool F32 = false>
__device__ __forceinline__ void sieve_item(const double *__restrict__ heavy, const int32_t *__restrict__ act,
                                           const double *__restrict__ Gall, const float *__restrict__ D,
                                           const int32_t *__restrict__ cend,
                                           int32_t *__restrict__ best, PassCounters *__restrict__ counters,
                                           const PruneState *__restrict__ st, const SieveArgs a, int &A_out, int &bitsel_out) {
    static_assert(TI <= 16, "queue entries keep the row in 4 bits");
    static_assert(DW == 2 * KD, "two families of KD components");
    constexpr int QCAP = TI * 64 * CPL + 64;  // one column tile can add TI * 64 * CPL pairs on top of a remainder below 64
    // CPL columns per lane: a tile is 64 * CPL columns, so one LDS read of a row
    constexpr int TILE_COLS = 64 * CPL;  // descriptor serves 4 x 64 pairs and the loop overhead is paid once per 256
    // an entry packs the row (4 bits) and the column offset inside the segment (12 bits: segments are <= 4096 columns)
    __shared__ unsigned short s_queue[4][QCAP];
    __shared__ unsigned short s_exq[4][128];  // pairs that the sign test could not reject, waiting for the exact path
    __shared__ double s_jacobi[4][32];        // scratch of the Jacobi fallback of the exact path (pair_math.hpp), per wavefront
    constexpr int RS = TRIM ? 20 : DW;  // floats per row record in LDS; TRIM: 16 components, the two squared norms, 2 of padding (80 B)
    __shared__ __attribute__((aligned(16))) float s_rowdesc[4][TI * RS];
    __shared__ f32x2 s_rownorm[4][TRIM ? 1 : TI];  // |row descriptor|^2 per family (TRIM keeps them in the row record)
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * 4 + wid;
    const int tile = a.tile_begin + slot * a.tile_stride;
    const int r0 = tile * TI;
    const int seg_lo = ((r0 + 1) & ~63) + int(blockIdx.y) * a.seg_cols;
    const int seg_hi = seg_lo + a.seg_cols;

    // ---- prologue in one memory round trip: the state, this item's 16 stop columns / best columns (they decide whether
    // it has work at all: most items of a late pass have none) and the descriptors of its rows and first column tile.
    // act[x] (needed for the coordinates of the pairs that reach H) is a valid structure index for every x < n:
    // k_init_run fills it with the identity, every pass rewrites a prefix.
    const int pass_on = st->pass_on, n_active = st->A;
    A_out = n_active, bitsel_out = st->bitsel;  // (for the fused tail: the state block cannot change before this item has arrived there)
    int my_cend = 0, my_best = 0;
    if (lane < TI && r0 + lane < a.n) {
        my_cend = cend[r0 + lane];
        my_best = __hip_atomic_load(&best[r0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static_assert(DW == 16 && TI * DW == 256, "row staging: 4 rows x 16 components per 64 lanes");
    // D holds the descriptors in ACTIVE order (position r = the r-th active structure; k_open_rows copies them there every
    // pass): rows and columns are read by position, nothing is gathered through act[] in front of the screen.  Positions
    // up to n - 1 are readable; those beyond the active count hold stale values that no row's range admits.
    int row_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) row_src[j] = min(r0 + 4 * j + (lane >> 4), a.n - 1);
    int col_src[CPL];
    auto load_cols = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < CPL; ++u) col_src[u] = min(c0 + 64 * u + lane, a.n - 1);
    };
    load_cols(seg_lo);
    if (pass_on == 0 || r0 >= n_active) return;
    const int nrows = min(TI, n_active - r0);
    const bool live0 = lane < nrows && my_cend > max(r0 + lane + 1, seg_lo) && my_best >= seg_lo;
    unsigned alive = unsigned(__ballot(live0));
    if (!alive) return;

    const float limit32 = screen_limit32_dot(__uint_as_float(*a.dmax_bits), a.desc_limit);
    const int limit_bits = __float_as_int(limit32);  // (positive: the integer order of the bit patterns is the float order from zero up)
    float rd_stage[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rd_stage[j] = D[int64_t(row_src[j]) * DW + (lane & 15)];
    f32x2 dq[CPL][KD];  // .x = family 0, .y = family 1
    f32x2 cn[CPL];      // their squared norms
    auto load_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(D + int64_t(col_src[u]) * DW);
#pragma unroll
            for (int k = 0; k < KD / 2; ++k) {
                const f32x4 v = src[k];
                dq[u][2 * k] = f32x2{v.x, v.y};
                dq[u][2 * k + 1] = f32x2{v.z, v.w};
            }
            f32x2 nc = {0.0f, 0.0f};  // |column descriptor|^2 per family, once per tile (shared by its 16 rows)
#pragma unroll
            for (int k = 0; k < KD; ++k) nc = __builtin_elementwise_fma(dq[u][k], dq[u][k], nc);
            // TRIM: the dot-product chain of a row starts from -|c|^2 / 2 (exact: a power of two), so that one fma by -2 onto
            // |r|^2 finishes |r|^2 + |c|^2 - 2 r.c without the separate packed add per column
            cn[u] = TRIM ? nc * f32x2{-0.5f, -0.5f} : nc;
        }
    };
    load_tile();

    int cmax = live0 ? my_cend : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
    cmax = min(__builtin_amdgcn_readfirstlane(cmax), seg_hi);

    // the row descriptors of this work item -> LDS (rows beyond nrows are never read back)
    float *rowdesc = s_rowdesc[wid];
#pragma unroll
    for (int j = 0; j < 4; ++j) rowdesc[(4 * j + (lane >> 4)) * RS + (lane & 15)] = rd_stage[j];
    __builtin_amdgcn_wave_barrier();
    if (lane < TI) {  // squared norms of the row descriptors, per family
        const f32x2 *dr = reinterpret_cast<const f32x2 *>(rowdesc + lane * RS);
        f32x2 nr = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < KD; ++k) nr = __builtin_elementwise_fma(dr[k], dr[k], nr);
        if constexpr (TRIM) *reinterpret_cast<f32x2 *>(rowdesc + lane * RS + DW) = nr;
        else s_rownorm[wid][lane] = nr;
    }
    __builtin_amdgcn_wave_barrier();

    TSC_STAMP(1);  // prologue data has arrived
    const int h3 = a.h * 3;
    unsigned short *queue = s_queue[wid];
    int qn = 0;
    unsigned long long n_eval = 0, n_exact = 0;
    int my_screened = 0;  // lanes 0..15: pairs of this item's rows that went through the screen (<= 16 x segment)
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    // Queue entries are evaluated in two stages, each over batches of up to 64 pairs with lpp = 64 / pow2ceil(batch) lanes
    // per pair.  Stage 1 forms H and applies the sign test; the few pairs it cannot reject (a few per cent) go to a second
    // queue.  Stage 2 -- the long explicit-rotation path -- runs when 64 of those have gathered (or at the end), so its
    // cost is paid once per 64 candidates instead of once per stage-1 batch with a handful of lanes busy.
    unsigned short *exq = s_exq[wid];
    int qe = 0;
    int64_t si = 0, sj = 0;  // the structures of the pair decoded last
    auto decode = [&](unsigned e, int &t, int &col, const double *&pp, const double *&pq, double &Gi, double &Gj) __attribute__((always_inline)) {
        t = int(e >> 12);
        col = seg_lo + int(e & 0xfffu);
        const int64_t i = act[r0 + t], j = act[col];
        si = i, sj = j;
        pp = heavy + i * h3, pq = heavy + j * h3;
        Gi = Gall[i], Gj = Gall[j];
    };
    auto sign_stage = [&](int base, int cnt) __attribute__((always_inline)) {
        int lpp = 64;
        while (lpp > 1 && 64 / lpp < cnt) lpp >>= 1;
        const int g = lane / lpp, sub = lane - g * lpp;
        bool cand = false, sim = false;
        unsigned e = 0;
        int t = 0;
        if (g < cnt) {  // a lane group is either wholly busy or wholly idle: the group shuffles only involve converged lanes
            e = queue[base + g];
            int col;
            const double *pp, *pq;
            double Gi, Gj;
            decode(e, t, col, pp, pq, Gi, Gj);
            const int verdict = pair_stage1<F32>(heavy, a.heavy32, si, sj, a.h, 0.5 * (Gi + Gj), a.half_h_thr2, a.two_thr2, sub, lpp);
            cand = sub == 0 && verdict == PAIR_UNDECIDED;
            sim = sub == 0 && verdict == PAIR_SIMILAR;
            if (sim) atomicMin(&best[r0 + t], col);
        }
        unsigned long long sm = __builtin_amdgcn_ballot_w64(sim);
        while (sm) {  // rows that found a similar column stop being screened (the reference returns there, :75-77)
            const int l = __ffsll((long long)sm) - 1;
            sm &= sm - 1;
            alive &= ~(1u << __builtin_amdgcn_readlane(t, l));
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(cand);
        if (m) {
            if (cand) exq[qe + __popcll(m & lt_mask)] = (unsigned short)e;
            qe += __popcll(m);
        }
        n_eval += cnt;
        n_exact += __popcll(m);
        __builtin_amdgcn_wave_barrier();
    };
    auto exact_stage = [&](int base, int cnt) __attribute__((always_inline)) {
        int lpp = 64;
        while (lpp > 1 && 64 / lpp < cnt) lpp >>= 1;
        const int g = lane / lpp, sub = lane - g * lpp;
        bool sim = false, degenerate = false;
        int t = 0;
        unsigned ent = 0;
        if (g < cnt) {
            int col;
            const double *pp, *pq;
            double Gi, Gj, H[9], e[4];
            ent = exq[base + g];
            decode(ent, t, col, pp, pq, Gi, Gj);
            pair_H(pp, pq, a.h, sub, lpp, H);
            if (rotation_quaternion_fast(H, Gi, Gj, e)) {  // (the lanes of a group hold the same H: they branch together)
                double rm, md;
                residual_rmsd_maxdev(pp, pq, a.h, e, rm, md, sub, lpp);
                sim = sub == 0 && rm < a.thr && md < a.maxdev_thr;  // rmsd_pruning.py:75
                if (sim) atomicMin(&best[r0 + t], col);
            } else {
                degenerate = sub == 0;
            }
        }
        unsigned long long sm = __builtin_amdgcn_ballot_w64(sim);
        while (sm) {  // rows that found a similar column stop being screened (the reference returns there, :75-77)
            const int l = __ffsll((long long)sm) - 1;
            sm &= sm - 1;
            alive &= ~(1u << __builtin_amdgcn_readlane(t, l));
        }
        // Pairs whose top eigenvalue is degenerate (collinear, planar through the origin, mirror-symmetric structures) need
        // the Jacobi eigen-solver.  Its two 4x4 matrices would cost every work item 64 registers, so the whole wavefront
        // takes such a pair on, one at a time: H by all 64 lanes, the solver by lane 0 on a 256-byte LDS area, the residual
        // by all lanes again.
        for (unsigned long long dm = __builtin_amdgcn_ballot_w64(degenerate); dm; dm &= dm - 1) {
            const unsigned e1 = unsigned(__builtin_amdgcn_readlane(int(ent), __ffsll((long long)dm) - 1));
            int t2, col2;
            const double *pp, *pq;
            double Gi, Gj, H[9], e[4], rm, md;
            decode(e1, t2, col2, pp, pq, Gi, Gj);
            pair_H(pp, pq, a.h, lane, 64, H);
            double *jac = s_jacobi[wid];
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
                if (lane == 0) atomicMin(&best[r0 + t2], col2);
                alive &= ~(1u << t2);
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    auto drain = [&](int base, int cnt) __attribute__((always_inline)) {
        sign_stage(base, cnt);
#ifdef TSC_DBG_NOEXACT
        qe = 0;
#endif
        if (qe >= 64) {
            exact_stage(qe - 64, 64);
            qe -= 64;
        }
    };

    for (int c0 = seg_lo; c0 < cmax;) {  // (alive != 0 here)
        {   // ---- screen one tile against every live row
            const bool here = lane < nrows && ((alive >> lane) & 1u) && my_cend > c0 && r0 + lane < c0 + TILE_COLS - 1;
            unsigned rows = unsigned(__ballot(here));
            // columns of this tile inside every live row's range (r, cend): counted once per tile by the rows' own lanes (a few
            // vector instructions per tile; as seven scalar ones per (row, tile) it was a quarter of the row loop's instructions)
            my_screened += here ? max(0, min(my_cend, c0 + TILE_COLS) - max(r0 + lane + 1, c0)) : 0;
            if constexpr (TRIM) {
                // rows whose range (r, cend) holds the WHOLE tile need no column mask: one bit per row
                const unsigned full = unsigned(__ballot(here && r0 + lane < c0 && my_cend >= c0 + TILE_COLS));
                // the same screen with fewer vector instructions per (row, tile): one LDS record per row (components and norms
                // behind one address), the norms folded into the dot-product chain, and the two families compared with the limit
                // separately instead of max / max / min / compare (NaN handling unchanged: a NaN component never rejects).
                // Two loops over the same body: first the rows that hold the whole tile (no column mask, no test for it),
                // then the few whose range ends or begins inside it.
                auto screen_row = [&](const int t, auto partial) __attribute__((always_inline)) {
#ifdef TSC_DBG_NOROWLOAD      // (measurement hook: every row of a tile uses row 0's record -- wrong verdicts, the screen without its per-row LDS reads)
                        const f32x2 *rec = reinterpret_cast<const f32x2 *>(rowdesc);
#else
                        const f32x2 *rec = reinterpret_cast<const f32x2 *>(rowdesc + t * RS);
#endif
                        f32x2 rd[KD];
#pragma unroll
                        for (int k = 0; k < KD; ++k) rd[k] = rec[k];
                        const f32x2 nr = rec[KD];
                        // Both family distances against the limit as INTEGER compares of the bit patterns (for a positive limit the
                        // order of non-negative floats; a negative sum -- rounding -- is below it either way; a NaN with a clear
                        // sign bit counts as beyond the limit where a float compare would let it through to H, which rejects it:
                        // :75).  The larger of a column's two families, the smaller of that over the lane's columns, ONE compare
                        // and one branch on it per (row, tile): the scalar side of this loop (27 instructions per trip against 24
                        // vector ones before: each family's compare into a lane mask, the masks combined and tested there) was
                        // what a wavefront spent its trip on.
                        int worst[CPL];
#pragma unroll
                        for (int u = 0; u < CPL; ++u) {
                            f32x2 acc = cn[u];                         // -|c|^2 / 2
#pragma unroll
                            for (int k = 0; k < KD; ++k) acc = __builtin_elementwise_fma(rd[k], dq[u][k], acc);
                            const f32x2 s2 = __builtin_elementwise_fma(acc, f32x2{-2.0f, -2.0f}, nr);
                            worst[u] = max(__float_as_int(s2.x), __float_as_int(s2.y));
                        }
                        if constexpr (decltype(partial)::value) {  // the tile crosses an end of the row's range: only the columns inside count
                            const int r = r0 + t, ce = __builtin_amdgcn_readlane(my_cend, t);
#pragma unroll
                            for (int u = 0; u < CPL; ++u) {
                                const int col = c0 + 64 * u + lane;
                                worst[u] = (col > r && col < ce) ? worst[u] : INT_MAX;
                            }
                        }
                        int nearest = worst[0];
#pragma unroll
                        for (int u = 1; u < CPL; ++u) nearest = min(nearest, worst[u]);
                        if (__builtin_amdgcn_ballot_w64(nearest <= limit_bits)) {   // (rare) some column of the tile is within the limit
#pragma unroll
                            for (int u = 0; u < CPL; ++u) {
                                const unsigned long long m = __builtin_amdgcn_ballot_w64(worst[u] <= limit_bits);
                                if (m) {
                                    if ((m >> lane) & 1ull) queue[qn + __popcll(m & lt_mask)] = (unsigned short)((unsigned(t) << 12) | unsigned(c0 + 64 * u + lane - seg_lo));
                                    qn += __popcll(m);
                                }
                            }
                        }
                };
                auto screen_rows = [&](unsigned todo, auto partial) __attribute__((always_inline)) {
                    while (todo) {
                        const int t = __ffs(todo) - 1;
                        todo &= todo - 1;
                        screen_row(t, partial);
                    }
                };
                if ((rows & full) == 0xffffu) {
                    // all 16 rows hold the whole tile (the usual tile of a large pass): the loop unrolled, every row's record at
                    // a constant LDS offset, no index arithmetic and no loop control between the rows
#pragma unroll
                    for (int t = 0; t < TI; ++t) screen_row(t, std::false_type{});
                } else {
                    screen_rows(rows & full, std::false_type{});
                    screen_rows(rows & ~full, std::true_type{});
                }
            } else
            while (rows) {
                const int t = __ffs(rows) - 1;
                rows &= rows - 1;
                const int r = r0 + t;
                const int ce = __builtin_amdgcn_readlane(my_cend, t);
                const f32x2 *dr = reinterpret_cast<const f32x2 *>(rowdesc + t * DW);
                f32x2 rd[KD];
#pragma unroll
                for (int k = 0; k < KD; ++k) rd[k] = dr[k];
                // larger of the two family distances for the lane's CPL columns, as |r|^2 + |c|^2 - 2 r.c in packed fp32 (one
                // v_pk_fma_f32 per component advances both families; 10 instructions per column, screen_limit32_dot has
                // the error bound)
                const f32x2 nr = s_rownorm[wid][t];
                float mx[CPL];
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    f32x2 dot = {0.0f, 0.0f};
#pragma unroll
                    for (int k = 0; k < KD; ++k) dot = __builtin_elementwise_fma(rd[k], dq[u][k], dot);
                    const f32x2 s2 = __builtin_elementwise_fma(dot, f32x2{-2.0f, -2.0f}, nr + cn[u]);
                    mx[u] = fmaxf(s2.x, s2.y);
                }
                if (!(r < c0 && ce >= c0 + TILE_COLS)) {  // the tile crosses an end of the row's range: mask the columns outside
#pragma unroll
                    for (int u = 0; u < CPL; ++u) {
                        const int col = c0 + 64 * u + lane;
                        mx[u] = (col > r && col < ce) ? mx[u] : __builtin_inff();
                    }
                }
                // most rows of a tile have no column within the limit: one test for all CPL * 64 pairs (a NaN distance --
                // NaN coordinates -- is ignored by the minimum; such a pair is not similar for the reference either, :75)
                float mn = mx[0];
#pragma unroll
                for (int u = 1; u < CPL; ++u) mn = fminf(mn, mx[u]);
                if (__builtin_amdgcn_ballot_w64(!(mn > limit32))) {
#pragma unroll
                    for (int u = 0; u < CPL; ++u) {
                        const bool pass = !(mx[u] > limit32);
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
                        if (m) {
                            if (pass) queue[qn + __popcll(m & lt_mask)] = (unsigned short)((unsigned(t) << 12) | unsigned(c0 + 64 * u + lane - seg_lo));
                            qn += __popcll(m);
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- drain full batches between tiles; a remainder below 64 waits for the next tile
#ifdef TSC_DBG_NODRAIN
        qn = 0;
#endif
        while (qn >= a.drain_min) {
            const int cnt = min(qn, 64);
            drain(qn - cnt, cnt);
            qn -= cnt;
        }
        // the next tile's columns (loaded here, after the drain, so that they do not occupy registers during it)
        c0 += TILE_COLS;
        if (!(c0 < cmax && alive)) break;
#ifndef TSC_DBG_NOTILELOAD   // (measurement hook: keep the first tile's descriptors -- wrong verdicts, the screen without its global loads)
        load_cols(c0);
        load_tile();
#endif
    }
    TSC_STAMP(2);  // screen done
#ifdef TSC_DBG_NODRAIN
    qn = 0;
#endif
    if (qn > 0) drain(0, qn);
#ifdef TSC_DBG_NOEXACT
    qe = 0;
#endif
    if (qe > 0) exact_stage(0, qe);
    TSC_STAMP(3);  // candidates evaluated
    for (int off = 8; off > 0; off >>= 1) my_screened += __shfl_xor(my_screened, off);
    if (lane == 0) {
        count_add(counters, unsigned(slot), CNT_FORMED, n_eval);
        count_add(counters, unsigned(slot), CNT_EXACT, n_exact);
        count_add(counters, unsigned(slot), CNT_SCREENED, (unsigned long long)my_screened);
    }
}

template <int TI, int CPL, bool TRIM = false, bool FUSED = false, bool F32 = false>
inline __global__ __launch_bounds__(256, CPL == 4 ? 4 : (CPL == 2 ? TSC_SIEVE_OCC2 : TSC_SIEVE_OCC1)) void k_rmsd_sieve(const double *__restrict__ heavy, const int32_t *__restrict__ act,
                                                        const double *__restrict__ Gall, const float *__restrict__ D,
                                                        const int32_t *__restrict__ cend,
                                                        int32_t *__restrict__ best, PassCounters *__restrict__ counters,
                                                        const PruneState *__restrict__ st, SieveArgs a, FusedApply fa) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = a.tile_begin + slot * a.tile_stride;
    const int r0 = tile * TI;
    const int seg_base = (r0 + 1) & ~63;
    const int seg_lo = seg_base + int(blockIdx.y) * a.seg_cols;
    TSC_STAMP(0);  // the wavefront has started
    if (r0 >= a.n || seg_lo >= a.n) return;  // beyond the upper bound the grid was sized for: nothing to read
    // most items of a pass with long chunks start beyond every stop column of their row tile (0 for a tile without rows or
    // a pass that is gated off: k_open_rows): one scalar load and out
    const int tcm = a.tile_cmax[2 * tile];
    if (tcm <= seg_lo) return;
    int A = 0, bitsel = 0;
    sieve_item<TI, CPL, TRIM, F32>(heavy, act, Gall, D, cend, best, counters, st, a, A, bitsel);
    if constexpr (FUSED) {
        // this item's atomicMin's on best[] are at the L2 before its arrival is
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const int lim = min(a.n, tcm);
        const int n_live = min(int(gridDim.y), (lim - seg_base + a.seg_cols - 1) / a.seg_cols);
        // (the tail of a light pass is a chain of dependent round trips -- arrival, state, best[], act[], the atomics' way out, the pass's
        // counter -- and its length is the pass: the only item of its tile needs no arrival, and the state block was read in the prologue)
        if (n_live > 1) {
            int last = 0;
            if (lane == 0) last = (atomicAdd(&fa.tile_done[tile], 1) == n_live - 1) ? 1 : 0;
            TSC_STAMP(4);  // arrived at the tile's counter
            if (!__builtin_amdgcn_readfirstlane(last)) return;
            if (lane == 0) fa.tile_done[tile] = 0;
        }
        unsigned long long ev_total = 0, rm_total = 0;
        apply_wave_rows(fa.ap, bitsel, r0 + lane, lane < TI && r0 + lane < A, ev_total, rm_total);
        int fin = 0;
        if (lane == 0) {
            count_add(counters, unsigned(slot), CNT_EVALUATED, ev_total);
            count_add(counters, unsigned(slot), CNT_REMOVED, rm_total);
        }
        if (!fa.tickets) {  // the pass is left open: the first kernel of the next one closes it behind the kernel boundary (pass_state.hpp, pass_derive)
            TSC_STAMP(5);
            return;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TSC_STAMP(5);  // tile applied
        if (lane == 0) fin = tickets_arrive(fa.tickets, unsigned(tile), fa.n_tiles, PT_GROUPS) ? 1 : 0;
        TSC_STAMP(6);  // arrived at the pass's counter
        if (__builtin_amdgcn_readfirstlane(fin)) {
            pass_step_wave(fa.sc, fa.next);
            TSC_STAMP(7);  // pass closed
        }
    }
}

}  // namespace tsc
