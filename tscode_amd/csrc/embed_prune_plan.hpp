// embed_prune_plan.hpp -- the sizes of an embed-and-prune run's device buffers (adjacent.hip: tsc_embed_prune_*): how many rows they hold
// after a slab has appended its kept poses, and what a row costs.  Plain host arithmetic, no HIP call: tools/probe/embed_prune_plan_check.cpp
// runs it on the CPU at sizes worked out by hand.
#pragma once

#include <cstdint>

namespace tsc {

constexpr int64_t EP_MIN_ROWS = 1024;               // the first allocation: a run that keeps a handful of poses does not grow at all
constexpr int64_t EP_MAX_ROWS = INT32_MAX - 4097;   // what the prune that follows takes (tsc_prune_create: n < 2^31 - 1 - 4096)

// Rows the buffers hold once `need` rows are wanted, from `cap` rows now (0: nothing allocated yet): `cap` while it is enough -- nothing
// moves --, otherwise doubled (from EP_MIN_ROWS the first time) until it is, and never more than EP_MAX_ROWS.  -1: `need` is negative or
// beyond EP_MAX_ROWS, or `cap` is negative.  need = 0 allocates nothing.
inline int64_t ep_grown_capacity(int64_t cap, int64_t need) {
    if (cap < 0 || need < 0 || need > EP_MAX_ROWS) return -1;
    if (need <= cap) return cap;
    int64_t grown = cap > 0 ? cap : EP_MIN_ROWS;
    while (grown < need) grown *= 2;                // (need < 2^31: the doubling stays far inside 64 bits)
    return grown < EP_MAX_ROWS ? grown : EP_MAX_ROWS;
}

// Bytes of the run's buffers per kept pose: its heavy atoms, and per molecule a rotation (72), a position (24) and a conformer index (4)
inline int64_t ep_row_bytes(int n_heavy, int n_mols) { return int64_t(24) * n_heavy + int64_t(100) * n_mols; }

// First double of row `row` in a buffer of `row_doubles` doubles per row (where a slab's rows are appended)
inline int64_t ep_row_offset(int64_t row, int row_doubles) { return row * int64_t(row_doubles); }

}  // namespace tsc
