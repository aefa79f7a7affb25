// rmsd_tile.hpp -- the register-tiled all-pairs kernel of the prune (pairs_tile.hip launches it; a template, so including it emits nothing).
//
// No MFMA, no LDS tiles for q: a lane owns one column structure q_j in registers (<= 32 heavy atoms after
// padding), the row structure p_i is wavefront-uniform and is read through the scalar cache, so the
// inner loop is 9 v_fma_f64 per atom with one SGPR operand each.
#pragma once
#include "pair_math.hpp"
#include "pass_state.hpp"

namespace tsc {

// ---------------------------------------------------------------------------------------------------
// the tile kernel

struct TileArgs {
    long long ld;     // leading dimension of Xc (structures per coordinate row)
    int h;
    int tile_begin;   // first tile of this rank
    int tile_stride;  // world size (row tiles are dealt round-robin to ranks)
    int seg_cols;     // columns per grid.y segment (multiple of 64)
    double thr, maxdev_thr;
    double half_h_thr2;  // h * thr^2 / 2
};

// One wavefront = one work item = (row tile of TI consecutive active rows) x (one column segment).
// Lane = column.  For every 64-column tile: load q_j into registers, then for each live row accumulate
// H = p_i^T q_j, run the sign test, remember survivors as per-lane bits; after the row loop the few
// survivors take the exact path and the smallest similar column of each row goes to best[] (atomicMin).
// A row stops being visited once it has a similar column to its left (the reference returns at the
// first similar column, rmsd_pruning.py:75-77).
template <int HP, int TI>
inline __global__ __launch_bounds__(256, 2) void k_rmsd_tile(const double *__restrict__ Xr, const double *__restrict__ Xc,
                                                       const double *__restrict__ G, const int32_t *__restrict__ cend,
                                                       int32_t *__restrict__ best, PassCounters *__restrict__ counters,
                                                       const PruneState *__restrict__ st, TileArgs a) {
    // Xr [n_active][HP*3] row structures; Xc [HP*3][ld] column structures; G [ld] squared norms;
    // cend [n_active] exclusive column bound of each row; best [n_active] atomicMin target (INT_MAX = none);
    // counters[0] pairs computed, counters[1] pairs sent to the exact path.
    static_assert(TI <= 32, "row liveness is a 32-bit lane mask");
    constexpr int HP3 = HP * 3;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (st->pass_on == 0) return;
    const int n_active = st->A;
    const int slot = blockIdx.x * 4 + wid;
    const int tile = a.tile_begin + slot * a.tile_stride;
    const int r0 = tile * TI;
    if (r0 >= n_active) return;
    const int nrows = min(TI, n_active - r0);
    const int seg_lo = ((r0 + 1) & ~63) + int(blockIdx.y) * a.seg_cols;
    const int seg_hi = seg_lo + a.seg_cols;

    int my_cend = 0, my_best = 0;
    if (lane < nrows) {
        my_cend = cend[r0 + lane];
        my_best = __hip_atomic_load(&best[r0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool live0 = lane < nrows && my_cend > max(r0 + lane + 1, seg_lo) && my_best >= seg_lo;
    unsigned alive = unsigned(__ballot(live0));
    if (!alive) return;
    int cmax = live0 ? my_cend : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
    cmax = min(__builtin_amdgcn_readfirstlane(cmax), seg_hi);

    unsigned long long n_computed = 0, n_cand = 0;
    for (int c0 = seg_lo; c0 < cmax && alive; c0 += 64) {
        const int col = c0 + lane;
        double q[HP3];
        {
            const double *xc = Xc + col;
#pragma unroll
            for (int d = 0; d < HP3; ++d, xc += a.ld) q[d] = *xc;
        }
        const double Gq = G[col];
        unsigned mycand = 0;  // bit t: this lane's column survived the sign test against row t
        unsigned candrows = 0;
        for (int t = 0; t < nrows; ++t) {
            if (!((alive >> t) & 1u)) continue;
            const int r = r0 + t;
            const int ce = __builtin_amdgcn_readlane(my_cend, t);
            if (ce <= c0 || r >= c0 + 63) continue;
            const double *__restrict__ pr = Xr + int64_t(r) * HP3;
            double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < HP; ++k) {
                const double px = pr[3 * k], py = pr[3 * k + 1], pz = pr[3 * k + 2];
                H[0] = fma(px, q[3 * k], H[0]), H[1] = fma(px, q[3 * k + 1], H[1]), H[2] = fma(px, q[3 * k + 2], H[2]);
                H[3] = fma(py, q[3 * k], H[3]), H[4] = fma(py, q[3 * k + 1], H[4]), H[5] = fma(py, q[3 * k + 2], H[5]);
                H[6] = fma(pz, q[3 * k], H[6]), H[7] = fma(pz, q[3 * k + 1], H[7]), H[8] = fma(pz, q[3 * k + 2], H[8]);
            }
            const double L = 0.5 * (G[r] + Gq) - a.half_h_thr2;
            const bool valid = col > r && col < ce;
            const bool cand = valid && !certainly_dissimilar(H, L, 0.5 * (G[r] + Gq), a.h);
            const unsigned long long vm = __ballot(valid);
            n_computed += __popcll(vm);
            if (__ballot(cand)) candrows |= 1u << t;
            mycand |= cand ? (1u << t) : 0u;
        }
        // exact path for the survivors of this column tile
        while (candrows) {
            const int t = __ffs(candrows) - 1;
            candrows &= candrows - 1;
            const int r = r0 + t;
            bool sim = false;
            if ((mycand >> t) & 1u) {
                double rm, md;
                rmsd_and_max_pair(Xr + int64_t(r) * HP3, Xr + int64_t(col) * HP3, a.h, rm, md);
                sim = rm < a.thr && md < a.maxdev_thr;  // rmsd_pruning.py:75
            }
            n_cand += __popcll(__ballot((mycand >> t) & 1u));
            const unsigned long long sm = __ballot(sim);
            if (sm) {
                if (lane == 0) atomicMin(&best[r], c0 + __ffsll((long long)sm) - 1);
                alive &= ~(1u << t);
            }
        }
    }
    if (lane == 0) {
        count_add(counters, unsigned(slot), CNT_FORMED, n_computed);
        count_add(counters, unsigned(slot), CNT_EXACT, n_cand);
    }
}

}  // namespace tsc
