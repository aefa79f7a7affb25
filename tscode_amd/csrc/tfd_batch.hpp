// tfd_batch.hpp -- prune_conformers_tfd for many ensembles per launch (device functions: tfd.hpp).  Included only by
// select_batch.hip, which launches these kernels.
#pragma once
#include "tfd.hpp"

namespace tsc {

// Segment s of a batch is an ensemble of its own: N structures of n atoms at coords + coord0, T quadruplets at quads + 4 * quad0.  Its
// fingerprints are f32[N][T] at tf + elem0: elem0 is the running sum of N * T, and an element finds its segment by that table.
struct TfdSegment {
    int64_t coord0, quad0, elem0;
    int32_t N, n, T, pad;
};
// _get_tf_mat of every segment: out f32[total], total = the sum of N * T
inline __global__ __launch_bounds__(256) void k_torsion_fingerprints_seg(const double *__restrict__ coords, const int32_t *__restrict__ quads,
                                                                   const TfdSegment *__restrict__ segs, int n_segs, int64_t total,
                                                                   float *__restrict__ out) {
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const TfdSegment g = segs[tfd_last_not_above(segs, n_segs, e, [](const TfdSegment &q) { return q.elem0; })];
        const int64_t el = e - g.elem0, s = el / g.T;   // (a segment that holds an element has T >= 1)
        out[e] = tfd_fingerprint_element(coords + g.coord0 + s * g.n * 3, quads + 4 * g.quad0, int(el - s * g.T));
    }
}

// One schedule slot for the segments whose gate is open in it (:166), each with its own pass geometry.  The rows of these segments are
// numbered through: wave0 is a segment's first number, and a wavefront finds its row's segment by that table.  first[row0 + i] = what
// k_tfd_first_similar gives row i of the segment alone, an index INSIDE the segment; rows of other segments are neither read nor written.
struct TfdPassSegment {
    int64_t wave0, row0, elem0, d, k, num_active;
    double thresh;
    int32_t N, T;
};
inline __global__ __launch_bounds__(256) void k_tfd_first_similar_seg(const float *__restrict__ tf, const TfdPassSegment *__restrict__ segs, int n_segs,
                                                                int64_t total_rows, int32_t *__restrict__ first) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < total_rows; r += int64_t(gridDim.x) * 4) {
        const TfdPassSegment g = segs[tfd_last_not_above(segs, n_segs, r, [](const TfdPassSegment &q) { return q.wave0; })];
        const int64_t i = r - g.wave0;
        const int32_t found = tfd_first_similar_row(tf + g.elem0, g.T, i, g.d, g.k, g.num_active, g.thresh, lane);
        if (lane == 0) first[g.row0 + i] = found;
    }
}

}  // namespace tsc
