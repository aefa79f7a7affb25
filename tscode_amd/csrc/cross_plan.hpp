// cross_plan.hpp -- what a cross-set RMSD call (cross.hip: queries against a library) launches, as numbers: the padded atom count and the
// path it selects, the width and number of the column segments, the grid, the size of the partial array of the `nearest` epilogue and the
// query rows one launch may take under a byte budget.  Plain functions that include nothing of HIP and make no HIP call: cross.hip launches
// what they say, tools/probe/cross_plan_check.cpp checks them without a GPU.
#pragma once

#include <cstdint>

namespace tsc {

constexpr int CX_ROWS = 16;            // query rows of a work item (one wavefront: a lane is a library column, rmsd_tile.hpp: k_rmsd_tile)
constexpr int CX_WAVES = 4;            // work items of a workgroup: four consecutive row tiles on one column segment
constexpr int CX_MAX_HP = 32;          // padded compared atoms the register path holds (96 doubles per lane); beyond: the general path
constexpr int CX_SEG_MAX = 4096;       // columns of a segment where the rows alone fill the chip: a long walk amortises a work item's setup
constexpr int CX_MAX_SEGS = 65535;     // grid.y
constexpr int64_t CX_TARGET_ITEMS = 4096;   // work items wanted: 256 compute units x 4 SIMDs x 2 wavefronts in flight, twice over
constexpr int64_t CX_MAX_GROUPS_X = 1 << 20;   // grid.x: the kernels stride over the row tiles beyond it
constexpr int64_t CX_PARTIAL_BYTES = int64_t(64) << 20;   // the partial array of one launch of the `nearest` epilogue at most
constexpr int64_t CX_PARTIAL_ENTRY = 8 + 8 + 4;           // rmsd f64, maxdev f64, index i32 per (segment, query row)

static inline int64_t cx_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t cx_round_up(int64_t a, int64_t b) { return cx_ceil_div(a, b) * b; }

// Compared atoms padded to the register kernel's instantiations (4 .. 32 in steps of 4), 0: more than 32, the general path
static inline int cross_padded_atoms(int h) { return h <= CX_MAX_HP ? int(cx_round_up(h < 1 ? 1 : h, 4)) : 0; }
// doubles per packed structure row: the padded atoms on the register path, the atoms themselves on the general path
static inline int cross_pitch(int h) { return 3 * (cross_padded_atoms(h) ? cross_padded_atoms(h) : h); }
// structures per coordinate row of the transposed copy (and entries of the squared norms): whole 64-column tiles
static inline int64_t cross_ld(int64_t n) { return cx_round_up(n < 1 ? 1 : n, 64); }

struct CrossPlan {
    int64_t n_tiles;     // row tiles of CX_ROWS queries
    int seg_cols;        // columns per segment, a multiple of 64
    int n_seg;           // segments = grid.y
    unsigned grid_x;     // workgroups along the rows
    int64_t partial;     // entries of the `nearest` partial arrays: n_seg x nq
};

// nq x nl pairs, nq >= 1 and nl >= 1 (the entry points return before planning where either is 0), both below 2^31.
//   * enough rows (n_tiles >= CX_TARGET_ITEMS: 65 536 queries): segments of CX_SEG_MAX columns, the rows fill the chip -- 10^5 queries
//     against a few hundred make 6250 work items of one segment each;
//   * few rows: the library is cut until rows x segments reach CX_TARGET_ITEMS, down to one 64-column tile per item -- one query against
//     10^6 makes 3907 items of 256 columns;
//   * a library so long that 65 535 segments of that width do not cover it gets wider segments.
static inline CrossPlan cross_plan(int64_t nq, int64_t nl) {
    CrossPlan p;
    p.n_tiles = cx_ceil_div(nq, CX_ROWS);
    const int64_t want_seg = p.n_tiles >= CX_TARGET_ITEMS ? 1 : cx_ceil_div(CX_TARGET_ITEMS, p.n_tiles);
    int64_t cols = cx_round_up(cx_ceil_div(nl, want_seg), 64);
    if (cols > CX_SEG_MAX) cols = CX_SEG_MAX;
    const int64_t floor_cols = cx_round_up(cx_ceil_div(nl, CX_MAX_SEGS), 64);
    if (cols < floor_cols) cols = floor_cols;
    p.seg_cols = int(cols);
    p.n_seg = int(cx_ceil_div(nl, cols));
    const int64_t gx = cx_ceil_div(p.n_tiles, CX_WAVES);
    p.grid_x = unsigned(gx < CX_MAX_GROUPS_X ? gx : CX_MAX_GROUPS_X);
    p.partial = int64_t(p.n_seg) * nq;
    return p;
}

// Query rows one launch may take so that bytes_per_row x rows stays within max_bytes; never less than 1 (a single row that exceeds the
// budget is still computed) and never more than n_rows
static inline int64_t cross_rows_within(int64_t n_rows, int64_t bytes_per_row, int64_t max_bytes) {
    int64_t rows = bytes_per_row > 0 ? max_bytes / bytes_per_row : n_rows;
    if (rows < 1) rows = 1;
    return rows < n_rows ? rows : (n_rows < 1 ? 1 : n_rows);
}
// ... of the values epilogue: rmsd and maxdev, f64[rows, nl] each
static inline int64_t cross_value_rows(int64_t nq, int64_t nl, int64_t max_bytes) { return cross_rows_within(nq, 16 * nl, max_bytes); }
// ... of the nearest epilogue: its partial arrays hold an entry per (segment, row); the segments are those of the WHOLE call (planned on
// nq rows), so that the verdicts do not depend on how the rows are walked
static inline int64_t cross_nearest_rows(int64_t nq, int n_seg) { return cross_rows_within(nq, CX_PARTIAL_ENTRY * n_seg, CX_PARTIAL_BYTES); }

}  // namespace tsc
