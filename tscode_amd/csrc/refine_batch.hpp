// refine_batch.hpp -- the moments of inertia with their pair search and the symmetry-corrected RMSD prune for many ensembles per
// launch (device functions: moi.hpp, rot_corr.hpp, tfd.hpp).  Included only by refine_batch.hip, which launches these kernels.
#pragma once
#include "moi.hpp"
#include "rot_corr.hpp"
#include "tfd.hpp"

namespace tsc {

// ---- moments of inertia (moi.hpp) ----------------------------------------------------------------------------------------------
// Segment s is an ensemble of its own: N structures of n atoms at structures + coord0 with the masses at masses + mass0.  The rows of
// all segments are numbered through (row0 is a segment's first number); a row finds its segment by that table, its moments lie at
// out + 3 * (row0 + i), and row i searches j > i inside its own segment only: first[row0 + i] is an index INSIDE the segment.
struct MoiSegment {
    int64_t row0, coord0, mass0;
    double max_deviation;
    int32_t N, n;
};

inline __global__ __launch_bounds__(256) void k_inertia_moments_seg(const double *__restrict__ structures, const double *__restrict__ masses,
                                                              const MoiSegment *__restrict__ segs, int n_segs, int64_t total_rows,
                                                              double *__restrict__ out) {
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < total_rows; r += int64_t(gridDim.x) * blockDim.x) {
        const MoiSegment g = segs[tfd_last_not_above(segs, n_segs, r, [](const MoiSegment &q) { return q.row0; })];
        inertia_moments_of(structures + g.coord0 + (r - g.row0) * g.n * 3, g.n, masses + g.mass0, out + 3 * r);
    }
}

inline __global__ __launch_bounds__(256) void k_moi_first_similar_seg(const double *__restrict__ mo, const MoiSegment *__restrict__ segs, int n_segs,
                                                                int64_t total_rows, int32_t *__restrict__ first) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < total_rows; r += int64_t(gridDim.x) * 4) {
        const MoiSegment g = segs[tfd_last_not_above(segs, n_segs, r, [](const MoiSegment &q) { return q.row0; })];
        const int32_t found = moi_first_similar_row(mo + 3 * g.row0, g.N, r - g.row0, g.max_deviation, lane);
        if (lane == 0) first[r] = found;
    }
}

// ---- symmetry-corrected RMSD (rot_corr.hpp) -------------------------------------------------------------------------------------
// One schedule slot of prune_conformers_rmsd_rot_corr (:1080-1152 without the graph step) for the segments whose gate is open in it.
// Every segment is an ensemble of its own -- its own molecule, set-up, threshold and pass geometry -- with its structures at
// coords + coord0, its cache rows of `words` words at cache + cache0 and its rows at first + row0; all open segments share k (the
// schedule is walked in lockstep), so workgroup b serves chunk b % k of segment b / k.  first holds indices INSIDE the segment.
// dynamic LDS: rot_corr_lds_bytes of the largest open segment; a workgroup lays out its own segment's lists and wave blocks inside it.
struct RotCorrSegment {
    RotCorrArgs a;
    int64_t coord0, cache0, row0;      // in doubles, 32-bit words and rows
    int64_t words, d, num_active;
    double thr;
    unsigned long long *evaluated;     // the segment's pair counter
};

inline __global__ __launch_bounds__(64 * RC_WAVES) void k_rot_corr_pass_seg(const RotCorrSegment *__restrict__ segs, int64_t k,
                                                                            double *__restrict__ coords, uint32_t *__restrict__ cache,
                                                                            int32_t *__restrict__ first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const RotCorrSegment g = segs[blockIdx.x / k];
    const int64_t step = blockIdx.x % k;
    const int64_t lo = g.d * step, hi = step == k - 1 ? g.num_active : g.d * (step + 1);   // :1093-1096
    if (lo >= hi) return;                                   // (block-uniform, in front of the first barrier)
    rot_corr_chunk(g.a, coords + g.coord0, cache + g.cache0, g.words, first + g.row0, lo, hi, g.thr, s_raw, g.evaluated);
}

}  // namespace tsc
