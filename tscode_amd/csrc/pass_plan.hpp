// pass_plan.hpp -- what a pass of the prune launches, as numbers: which of the three shapes it takes (chunk-local, culled, walked) and
// every grid of each.  Plain functions of (n, k, rows, rank, world, the context's options (options.hpp), the run's kernel form) that return structs
// by value and make no HIP call: prune.hip launches what they say, tools/probe/pass_plan_check.cpp checks them without a GPU.
#pragma once

#include <algorithm>

#include "common.hpp"
#include "shapes.hpp"

using namespace tsc;

static_assert(OPT_LOCAL_MAX_CHUNK_MAX == LP_MAX_ROWS, "the range of \"local_max_chunk\" (options.hpp) ends at the longest chunk the chunk-local kernel takes");

// The chunks [c_lo, c_hi) and structures [s_lo, s_hi) a pass covers on this device: all of them, or a rank's share of a partitioned pass
struct PassRows {
    int64_t c_lo, c_hi, s_lo, s_hi;
};
static inline PassRows whole_pass(int64_t n, int64_t k) { return PassRows{0, k, 0, n}; }

// Chunks [c_lo, c_hi) of a pass of k chunks that START inside rank's block [n rank / world, n (rank + 1) / world) of the
// structure axis, and the structures [s_lo, s_hi) they cover (the last chunk of the pass runs to n, rmsd_pruning.py:141-144).
static inline PassRows partition_bounds(int64_t n, int64_t k, int rank, int world) {
    const int64_t cs = n / k;
    auto first_chunk = [&](int r) { return r <= 0 ? int64_t(0) : (r >= world ? k : std::min<int64_t>(ceil_div<int64_t>(n * r / world, cs), k)); };
    PassRows r;
    r.c_lo = first_chunk(rank), r.c_hi = first_chunk(rank + 1);
    r.s_lo = r.c_lo < k ? r.c_lo * cs : n, r.s_hi = r.c_hi < k ? r.c_hi * cs : n;
    return r;
}

// The pair kernel a sieve run's walked passes take: the 64-row matrix-core kernel (mm.hpp; groups of 64 rows dealt round-robin to the
// ranks), the 16-row matrix-core kernel (k_rmsd_sieve_mm16), or neither: the packed-fp32 kernel.  records: the run holds float16 records.
struct PairForm {
    bool mm, mm16;
};
static inline PairForm pair_form(const tsc_options &c, int algo, bool records, bool mm64) {
    return PairForm{algo == ALGO_SIEVE && records && mm64, algo == ALGO_SIEVE && records && !mm64 && c.sieve_cpl == 2 && c.sieve_trim != 0};
}

// ---- which shape ----
struct PassShape {
    int rows_ub;                // grids are sized for this upper bound of the rows; kernels read the true count from the state block
    int64_t chunk;              // n / k
    int64_t longest_of_pass;    // the last chunk takes the remainder (:141-142)
    int64_t longest_of_rank;    // ... of this rank's chunks, in a partitioned pass: the last chunk of the pass only if it is among them
    bool local;                 // the whole pass in one launch of the chunk-local kernel
    bool culled;                // candidate for the sorted layout (the device decides between culled and walked: k_cull_decide)
    bool fused;                 // the walked pair kernel applies the verdicts itself
    bool need_dc;               // k_open_rows writes the fp32 descriptors by position
};

// range = false: the rows dealt to (rank, world) by tiles, of all chunks; range = true: every row of rank's chunks `r` (world is 1 then)
static inline PassShape pass_shape(const tsc_options &c, int64_t n, int64_t k, int algo, bool records, bool mm64, bool det_desc, int world, bool range,
                                   const PassRows &r) {
    PassShape s;
    s.rows_ub = int(std::max<int64_t>(r.s_hi - r.s_lo, 1));
    s.chunk = n / k;
    s.longest_of_pass = n - (k - 1) * s.chunk;
    s.longest_of_rank = r.c_hi == k ? s.longest_of_pass : s.chunk;
    // Short chunks: the whole pass in one launch, a workgroup (or a few) per chunk (local_pass.hpp)
    // (measured on MI355X: a block of the chunk-local kernel is a chain of dependent memory round trips, so it wins where
    // chunks are a few row tiles long -- at 57k structures the passes k = 1000, 500 and 200 take 37, 39 and 50 us instead of
    // 52-58 -- and loses beyond: k = 100 takes 58 us there against 53 on the two-launch path; "local_max_chunk" moves the limit: 384)
    // (the longest chunk counts, i.e. the last one with its remainder: at 57 046 structures in 2 000 chunks -- 28 each, 1 074 in the last --
    // the chunk-local kernel was tried with the long chunk on workgroups of its own: 97 us against 37 for the two launches)
    s.local = algo == ALGO_SIEVE && world == 1 && c.local_pass != 0 &&
              std::max<int64_t>(s.longest_of_rank, s.chunk) <= std::min(LP_MAX_ROWS, c.local_max_chunk) && r.c_hi > r.c_lo;
    // Large passes: the structures laid out along a Morton curve, tile pairs skipped by bounding box (cull.hpp)
    // (the pairs a rank gets to look at: its chunks in a partitioned pass, its row tiles in a pass dealt by tiles -- the layout and
    // the boxes are made by every rank for itself and have to pay for themselves on that share)
    const double my_pairs = range ? double(r.s_hi - r.s_lo) * double(n / k) * 0.5 : double(n) * double(n / k) * 0.5 / double(world);
    // (row tiles dealt to several ranks: twice the threshold -- every rank lays the whole pass out for an eighth, say, of its tiles;
    // measured at 1M x 50 and eight ranks the culled k = 2 pass costs a rank 0.82 ms against 0.77 for the walk)
    // Row tiles of a pass dealt to several ranks (tsc_prune_pass_local / _rows with world > 1): the ranks deal the tiles of ONE sorted layout,
    // so every rank must hold bit-identical descriptors -- only runs created under "deterministic_basis" may be culled that way; the others
    // walk the pass in index order, every rank alike.  (Inside a pass partitioned by chunks a rank culls its own chunks with a layout of
    // its own: no such condition.)
    const bool shared_layout_ok = world == 1 || range || det_desc;
    s.culled = !s.local && algo == ALGO_SIEVE && c.cull != 0 && c.sieve_cpl == 2 && k < CULL_MAX_CHUNKS && shared_layout_ok &&
               my_pairs >= c.cull_min_pairs * ((world > 1 && !range) ? 2.0 : 1.0);
    s.fused = !s.local && algo == ALGO_SIEVE && world == 1 && (c.fused_apply != 0 || range);
    // (the fp32 rows by position: read by the packed-fp32 kernels, by level 2 of the 64-row matrix-core kernels where it is built in, and by a
    // culled pass's layout)
    s.need_dc = !(algo == ALGO_SIEVE && records && (mm64 ? !TSC_MM_LEVEL2 : (c.sieve_cpl == 2 && c.sieve_trim != 0)) && !s.culled);
    return s;
}

// ---- k_open_rows: a row tile of 16 per wavefront quarter, 16 tiles per workgroup ----
struct OpenPlan {
    unsigned n_tiles, blocks;
    int stamp_blocks;   // (-DTSC_DBG_STAMPS: workgroups the stamp buffer is sized for)
};
static inline OpenPlan plan_open_rows(int rows_ub) {
    return OpenPlan{unsigned(ceil_div(rows_ub, 16)), unsigned(ceil_div(ceil_div(rows_ub, 16), 16)), ceil_div(ceil_div(rows_ub, 16), 4)};
}

// ---- the chunk-local pass ----
struct LocalPlan {
    int nb_regular;   // blocks per chunk for chunks 0 .. k-2
    int nb_last;      // blocks of the last chunk of the pass (0: it is another rank's)
    int n_reg;        // regular chunks of this launch
    int64_t blocks;
};
static inline LocalPlan plan_local(int64_t n, int64_t k, const PassRows &r) {
    const int cs = int(n / k);
    LocalPlan l;
    l.nb_regular = std::max(1, ceil_div(ceil_div(cs, LP_TI), LP_TILES_PER_BLOCK));
    l.nb_last = r.c_hi == k ? std::max(1, ceil_div(ceil_div(int(n - (k - 1) * cs), LP_TI), LP_TILES_PER_BLOCK)) : 0;
    l.n_reg = int(std::min<int64_t>(r.c_hi, k - 1) - r.c_lo);
    l.blocks = int64_t(l.n_reg) * l.nb_regular + l.nb_last;
    return l;
}

// ---- the walked pass: rows dealt round-robin over ranks in tiles of 16, columns cut into segments for load balance ----
struct WalkedPlan {
    int rows;         // what the kernels COUNT arrivals by: rows_ub, which k_open_rows was launched with
    int n_tiles;      // row tiles of the pass
    int max_range;    // columns a row can have: the longest chunk of the pass, or all the rows there are
    int seg_cols, n_seg;
    int mm16_waves;   // work items per workgroup of the 16-row matrix-core kernel
    dim3 grid;
};
// ---- the 16-row matrix-core kernel's work item: columns per segment and items per workgroup, from the columns a row of the pass can have ----
// The rule (measured per pass on MI355X at 57 046 structures, tools/sweep_items.py; MEASURED.md 33):
//   * segments of 1 024 columns where a row's range holds eight of them (max_range >= 8 192), else 512, halved to 256 while the range is
//     shorter than four segments.  An item's screen is 1 us per 128 columns; from 11 410 columns a row on, 1 024 ends a pass 4 - 5 us sooner
//     than 512 (half the items, each paying prologue and tail once), at 5 705 it ends it 2 us later (a pass ends with its longest item), and
//     2 048 loses everywhere but in the last pass.  One segment per row tile (ranges up to 4 032) was measured too: level at 570 and 1 140
//     columns a row, 6 us worse at 1 074 (the long last chunk of a pass of short chunks), 15 us worse at 2 853 -- not taken.
//   * two items per workgroup; four where most workgroups are empty and the launch is its dispatch -- a range of more than MM16_LONG_SEGS
//     segments of 512 columns (of the segment length itself where "seg_cols" set a shorter one), whatever length the segments have: the
//     one-chunk pass of 57 046 takes 50 us with four items on 1 024 columns, 55 with two, 59 with four on 512.  One item per workgroup was
//     measured as well (within 1 us of two in every pass): there is no such instantiation.
// The sweep was of ONE run size (57 046 structures: the kernel takes runs below "mm_min_n" = 100 000).  The row tiles of the pass and the
// wavefronts the device holds decide nothing in it -- shapes that bring the items of a pass under the 4 096 wavefront slots gained nothing
// -- so the rule is of max_range alone.  A run this kernel is given beyond 100 000 structures ("sieve_mm" = 0, a higher "mm_min_n") was not
// measured: by_n_cols, the length plan_walked has for a run of that size (1 024, 4 096 beyond 400 000), stays the floor there, as it was.
// Queue entries carry the column offset inside the segment in MM16_OFFSET_BITS bits: no segment is longer than 4 096 columns.
struct Mm16Shape {
    int seg_cols, waves;
};
constexpr int MM16_OFFSET_BITS = 12;
constexpr int MM16_WIDE_RANGE = 8 * 1024;
// (for variant builds of a sweep, tools/build_variant.py + tools/sweep_items.py: -DTSC_MM16_ITEMS=2 or 4 gives every pass that many items per
// workgroup, -DTSC_MM16_SEG=cols every pass of this kernel that segment length, unhalved; 0: the rule)
#ifndef TSC_MM16_ITEMS
#define TSC_MM16_ITEMS 0
#endif
#ifndef TSC_MM16_SEG
#define TSC_MM16_SEG 0
#endif
static_assert(TSC_MM16_ITEMS == 0 || TSC_MM16_ITEMS == 2 || TSC_MM16_ITEMS == 4, "k_rmsd_sieve_mm16 is instantiated for 2 and 4 items per workgroup");
static_assert(TSC_MM16_SEG >= 0 && TSC_MM16_SEG <= (1 << MM16_OFFSET_BITS) && TSC_MM16_SEG % 128 == 0, "whole column tiles, within the offset bits");
static inline int mm16_items_per_workgroup(int max_range, int seg_cols) {
    if (TSC_MM16_ITEMS) return TSC_MM16_ITEMS;
    return max_range + 64 > MM16_LONG_SEGS * std::min(seg_cols, 512) ? 4 : 2;
}
static inline Mm16Shape mm16_item_shape(int max_range, int by_n_cols = 512) {
    Mm16Shape m;
    m.seg_cols = std::max(by_n_cols, max_range >= MM16_WIDE_RANGE ? 1024 : 512);
    while (m.seg_cols > 256 && max_range < m.seg_cols * 4) m.seg_cols /= 2;
    if (TSC_MM16_SEG) m.seg_cols = TSC_MM16_SEG;
    m.waves = mm16_items_per_workgroup(max_range, m.seg_cols);
    return m;
}

// rows_ub: upper bound of the rows of the pass on this device (n; in a rank-partitioned pass the structures of this rank's chunks)
// rows_now (< 0: not known; else <= rows_ub is meant): the rows the pass really has, where the host has learnt it (a pass that waited for
// k_cull_decide): the grid is sized for them; everything else stays with rows_ub
static inline WalkedPlan plan_walked(const tsc_options &c, int64_t n, int64_t k, int rank, int world, int64_t rows_ub, int64_t rows_now, PairForm f) {
    WalkedPlan w;
    const int A = w.rows = int(std::max<int64_t>(rows_ub, 1));
    const int64_t longest_of_pass = n - (k - 1) * (n / k);
    w.n_tiles = ceil_div(A, TILE_ROWS);
    w.max_range = int(std::min<int64_t>(A, longest_of_pass));
    // a wavefront walks its segment tile by tile: short segments keep the critical path short when a pass has little
    // work (many small chunks), long ones amortise the per-item setup when it has a lot
    // (the packed-fp32 kernel, measured on MI355X, tools/sweep.py: 512 columns at 57k structures, 1024 at 126k, 4096 at 483k; "seg_cols" overrides)
    const int by_n_cols = n <= 100000 ? 512 : (n <= 400000 ? 1024 : 4096);
    w.seg_cols = c.seg_cols > 0 ? c.seg_cols : by_n_cols;
    while (w.seg_cols > 256 && w.max_range < w.seg_cols * 4) w.seg_cols /= 2;
    // the screen on the matrix cores (mm.hpp): 64 rows per work item and segments of their own length
    if (f.mm) w.seg_cols = c.mm_seg_cols > 0 ? c.mm_seg_cols : (w.max_range >= 2048 ? 1024 : 512);
    // the 16-row matrix-core kernel: lengths of its own as well (mm16_item_shape; "seg_cols" overrides, as above)
    if (f.mm16 && c.seg_cols <= 0) w.seg_cols = mm16_item_shape(w.max_range, by_n_cols).seg_cols;
    static_assert((1 << MM16_OFFSET_BITS) >= 4096, "the longest segment a rule of this file returns");
    w.n_seg = ceil_div(w.max_range + 64, w.seg_cols);  // + 64: a segment starts at the 64-aligned column below r0 + 1
    const int my_tiles = (w.n_tiles - rank + world - 1) / world;
    // (mm: groups of 64 rows dealt round-robin to the ranks; the 16-row matrix-core kernel: two items per workgroup, four where most workgroups are
    // empty -- mm16_items_per_workgroup)
    w.mm16_waves = f.mm16 ? mm16_items_per_workgroup(w.max_range, w.seg_cols) : 4;
    const int A_grid = rows_now >= 0 ? int(std::min<int64_t>(std::max<int64_t>(rows_now, 1), A)) : A;
    const int grid_tiles = (ceil_div(A_grid, TILE_ROWS) - rank + world - 1) / world;
    w.grid = dim3(std::max(1, f.mm ? ceil_div((ceil_div(A_grid, MM_ROWS) - rank + world - 1) / world, MM_WAVES) : ceil_div(std::min(my_tiles, grid_tiles), w.mm16_waves)),
                  w.n_seg);
    return w;
}

// ---- the culled pass: this rank's row tiles (or groups of 64 rows: cull_mm) of the sorted layout x segments of the columns behind them ----
constexpr int CULL_SEG_COLS = 4096;   // columns per work item of k_rmsd_sieve_sorted
struct CulledPlan {
    int tile_block;     // several ranks: consecutive tiles of the sorted layout per rank and turn ("cull_tile_block"); else 1
    int my_tiles, n_seg;
    unsigned sgrid;     // workgroups of k_rmsd_sieve_sorted
    int n_groups, n_seg_mm;   // cull_mm: this rank's groups of 64 rows, segments of CMM_SEG columns
    int64_t grid_mm;    // ... and the workgroups of k_rmsd_sieve_sorted_mm (one wavefront each; launched with at least 1)
};
static inline CulledPlan plan_culled(const tsc_options &c, int rows_ub, int64_t longest_of_rank, int rank, int world, bool cull_mm) {
    CulledPlan p;
    const int A = rows_ub;
    const int tb = p.tile_block = world > 1 ? std::max(1, c.cull_tile_block) : 1;
    const int n_tiles = ceil_div(A, TILE_ROWS);
    // (slots of this rank: one by one, or whole runs of tb tiles -- an upper bound; slots beyond the last tile leave at once)
    p.my_tiles = tb <= 1 ? (n_tiles - rank + world - 1) / world : (n_tiles / (tb * world) + 1) * tb;
    // columns of a row tile: from its own 128-aligned position to the end of its (last row's) chunk -- a chunk and a tile more at most
    p.n_seg = ceil_div(int(std::min<int64_t>(A, longest_of_rank)) + 2 * CULL_COLS, CULL_SEG_COLS);
    const int64_t items = int64_t(ceil_div(p.my_tiles, 4)) * p.n_seg;
    // ("cull_xcd": one work item per workgroup, runs of row groups keyed to XCDs -- 8 XCDs x segments x the runs an XCD holds of a segment)
    const int64_t xitems = int64_t(8) * p.n_seg * ceil_div(ceil_div(ceil_div(p.my_tiles, 4), CULL_XCD_RUN), 8) * CULL_XCD_RUN;
    p.sgrid = unsigned(std::max<int64_t>(1, c.cull_xcd ? xitems : std::min<int64_t>(items, c.cull_grid)));
    p.n_groups = p.n_seg_mm = 0, p.grid_mm = 0;
    if (cull_mm) {
        // (one wavefront per workgroup; several ranks: this rank's share of the groups, in runs of tile_block / 4 -- an upper bound)
        const int all_groups = ceil_div(A, MM_ROWS), tbg = std::max(1, tb / 4);
        const int wgs = p.n_groups = world <= 1 ? all_groups : (all_groups / (tbg * world) + 1) * tbg;
        p.n_seg_mm = ceil_div(int(std::min<int64_t>(A, longest_of_rank)) + 2 * CULL_COLS, CMM_SEG);
        p.grid_mm = c.cull_xcd ? int64_t(8) * p.n_seg_mm * ceil_div(ceil_div(wgs, CULL_XCD_RUN), 8) * CULL_XCD_RUN : int64_t(wgs) * p.n_seg_mm;
    }
    return p;
}

// ---- the thresholds every pair kernel takes (rmsd_pruning.py:95: maxdev_thr = 2 thr) ----
struct Thresholds {
    double thr, maxdev_thr;
    double half_h_thr2;   // h * thr^2 / 2
    double two_thr2;      // 2 thr^2 when the near-duplicate test applies (h >= 4), else -1
    double desc_limit;    // h thr^2: exact squared descriptor distance above which a pair is certainly dissimilar
};
static inline Thresholds thresholds(int h, double thr) {
    return Thresholds{thr, 2 * thr, 0.5 * double(h) * thr * thr, h >= 4 ? 2.0 * thr * thr : -1.0, double(h) * thr * thr};
}
