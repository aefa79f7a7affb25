// diverse_align_kernel.hpp -- k_align_structures, the one kernel of diverse.hpp's family that a unit carries without launching it:
// diverse.hip launches it, select_batch.hip (through diverse_batch.hpp) only carries it.  k_align_structures_seg calls the same
// dv_align_structures, and what the compiler makes of that call depends on the other caller being in the unit: alone, the function is
// inlined into k_align_structures_seg and the kernel is no longer the code that was measured.  So the two stay together.
#pragma once
#include "diverse.hpp"

namespace tsc {

inline __global__ __launch_bounds__(256) void k_align_structures(const double *__restrict__ in, int64_t N, int n, const int32_t *__restrict__ idx,
                                                                 int n_idx, double *__restrict__ out) {
    dv_align_structures(in, N, n, idx, n_idx, out, blockIdx.x);
}

}  // namespace tsc
