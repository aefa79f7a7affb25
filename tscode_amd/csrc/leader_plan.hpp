// leader_plan.hpp -- what an energy-ordered RMSD prune (leader.hip: the greedy "keep a row iff no kept row before it is similar") launches,
// as numbers: the rows of a block, the blocks of a run, the capacity and leading dimension of the growing library pack, the grid of the
// in-block similarity bits and the launches and read-backs of a whole run.  Plain functions that include nothing of HIP and make no HIP
// call: leader.hip launches what they say, tools/probe/leader_plan_check.cpp checks them without a GPU.
#pragma once

#include <cstdint>

#include "cross_plan.hpp"

namespace tsc {

constexpr int LEADER_BLOCK = 1024;               // rows of the order decided per round: one library walk, one in-block triangle, one replay
constexpr int LEADER_WORDS = LEADER_BLOCK / 64;  // 64-bit words of a row's similarity bits
constexpr int LD_ROWS = 16;                      // rows of a bits work item (one wavefront: a lane is an earlier row of the block)
constexpr int LD_WAVES = 4;                      // work items of a workgroup: four consecutive row tiles on one 64-column tile
static_assert(LEADER_BLOCK % 64 == 0 && LEADER_BLOCK % (LD_ROWS * LD_WAVES) == 0, "whole bit words, whole workgroups of row tiles");

static inline int64_t leader_blocks(int64_t n) { return cx_ceil_div(n, LEADER_BLOCK); }
// rows of block b (0 .. leader_blocks(n) - 1): LEADER_BLOCK but for the last
static inline int leader_block_rows(int64_t n, int64_t b) {
    const int64_t left = n - b * LEADER_BLOCK;
    return int(left < LEADER_BLOCK ? left : LEADER_BLOCK);
}
// structures the library pack has room for: the caller's library and, at worst, every row of the call (n + n_library <= 2^31 - 1)
static inline int64_t leader_capacity(int64_t n_library, int64_t n) { return n_library + n; }
// structures per coordinate row of its transposed copy, and entries of its squared norms
static inline int64_t leader_ld(int64_t n_library, int64_t n) { return cross_ld(leader_capacity(n_library, n)); }

// The in-block bits of nb rows: grid.x walks the row tiles four to a workgroup, grid.y the 64-column tiles; an item whose columns all lie
// at or behind its rows (c0 > r0) has nothing to state and leaves at once
struct LeaderBitsGrid {
    unsigned x, y;
};
static inline LeaderBitsGrid leader_bits_grid(int nb) {
    LeaderBitsGrid g;
    g.x = unsigned(cx_ceil_div(cx_ceil_div(nb, LD_ROWS), LD_WAVES));
    g.y = unsigned(cx_ceil_div(nb, 64));
    return g;
}
// whether the item (row tile rt, column tile ct) states pairs: its first column lies in front of its last row
static inline bool leader_item_has_pairs(int64_t rt, int64_t ct) { return ct * 64 <= rt * LD_ROWS; }

// Launches and 4-byte read-backs of a whole run, from shapes alone.  Per block: the library walk (none while the pack is empty, which only
// the first block of a call without a library can be sure of -- counted as present from the second block on), the bits, the replay, the
// append (none after the last block), one read-back.  In front: the gather (an order given), the two packs (the library's only where there
// is one) and three fills (first[], the pack's norms, its transposed copy on the register path).
struct LeaderCounts {
    int64_t blocks, launches, readbacks;
};
static inline LeaderCounts leader_counts(int64_t n, int64_t n_library, bool ordered, bool register_path) {
    LeaderCounts k;
    k.blocks = leader_blocks(n);
    k.readbacks = k.blocks;
    const int64_t walks = n_library > 0 ? k.blocks : (k.blocks > 0 ? k.blocks - 1 : 0);
    const int64_t appends = k.blocks > 0 ? k.blocks - 1 : 0;
    k.launches = (ordered ? 1 : 0) + 1 + (n_library > 0 ? 1 : 0) + 2 + (register_path ? 1 : 0) + walks + 2 * k.blocks + appends;
    return k;
}

}  // namespace tsc
