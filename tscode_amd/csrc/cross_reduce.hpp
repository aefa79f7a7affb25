// cross_reduce.hpp -- the second step of the cross-set RMSD's `nearest` epilogue (cross.hpp: CX_NEAREST).  A header of its own because a
// non-template kernel is compiled into every unit that includes its header: cross.hip launches it, leader.hip (which includes cross.hpp for
// the CX_FIRST rectangle) does not.
#pragma once

#include "common.hpp"

namespace tsc {

// Second step of CX_NEAREST: a thread per query row takes the segments in ascending order (ascending library indices); a strictly smaller
// rmsd wins, so that ties stay with the lowest index.  index -1: no pair of the row compared below +inf (an empty or non-finite row).
inline __global__ __launch_bounds__(256) void k_cross_nearest_reduce(const double *__restrict__ pr, const double *__restrict__ pm, const int32_t *__restrict__ pi,
                                                               int n_seg, long long nq, int32_t *__restrict__ index, double *__restrict__ rmsd,
                                                               double *__restrict__ maxdev) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < nq; r += (long long)gridDim.x * blockDim.x) {
        double br = INFINITY, bm = INFINITY;
        int bi = -1;
        for (int s = 0; s < n_seg; ++s) {
            const long long o = (long long)s * nq + r;
            const double v = pr[o];
            if (v < br) br = v, bm = pm[o], bi = pi[o];
        }
        index[r] = bi, rmsd[r] = br, maxdev[r] = bm;
    }
}

}  // namespace tsc
