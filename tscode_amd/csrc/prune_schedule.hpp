// prune_schedule.hpp -- the pass schedule of prune_conformers_rmsd (tscode/rmsd_pruning.py:186-188), the gate of a pass (:192) and the chunk
// of a row (:136-144), stated once for the host (prune_host.hpp, prune_batch_plan.hpp) and for the kernels that walk the schedule themselves
// (prune_batch.hpp, prune_team.hpp).
#pragma once

#include "common.hpp"

namespace tsc {

// whole numbers: int(k) -- the reference itself fails for float k
constexpr int KS[TSC_MAX_PASSES] = {500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1};  // :186-188

// :192 -- the pass of k chunks runs on `active` structures still in the mask
__host__ __device__ inline bool pass_gate(long long k, long long active) { return k == 1 || 20 * k < active; }

// The chunk [f, l) of row i in a pass of k chunks of cs = N / k structures each, the last one running to N; returns the chunk's index
__host__ __device__ inline int chunk_of_row(int i, int N, int k, int cs, int &f, int &l) {
    const int c = i / cs < k - 1 ? i / cs : k - 1;
    f = c * cs;                        // :140
    l = (c == k - 1) ? N : f + cs;     // :141-144
    return c;
}

}  // namespace tsc
