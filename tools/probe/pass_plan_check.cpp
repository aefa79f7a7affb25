// pass_plan_check.cpp -- the sizing functions of csrc/pass_plan.hpp (which shape a prune pass takes, every grid of each shape) run by a
// stand-alone program at shapes worked out by hand from the formulas, so that they can be checked without a GPU and built with
// AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library; tools/pass_plan_check.py builds and runs it.  No HIP runtime
// call is made (the functions take the options, a plain struct).  Grids marked [trace] were also seen in a kernel trace of
// tools/pass_shapes.py (MEASURED.md 17).
//
//   pass_plan_check        (exit status 0 and a line "pass_plan_check: N checks passed", or the first failed check and status 1)
#include <cstdio>

#include "../../tscode_amd/csrc/pass_plan.hpp"

static int g_checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                            \
        }                                                        \
    } while (0)

static bool is_grid(dim3 g, unsigned x, unsigned y) { return g.x == x && g.y == y && g.z == 1; }

static const PairForm PACKED{false, false}, MM16{false, true}, MM64{true, false};

static int forms() {
    tsc_options c;
    // a sieve run with float16 records: the 64-row kernels where the run chose them, else the 16-row form -- which exists for the default
    // screen (sieve_cpl 2, trimmed) only; no records, or the register-tiled kernel: neither
    CHECK(pair_form(c, ALGO_SIEVE, true, true).mm && !pair_form(c, ALGO_SIEVE, true, true).mm16);
    CHECK(!pair_form(c, ALGO_SIEVE, true, false).mm && pair_form(c, ALGO_SIEVE, true, false).mm16);
    CHECK(!pair_form(c, ALGO_SIEVE, false, false).mm16 && !pair_form(c, ALGO_SIEVE, false, true).mm && !pair_form(c, ALGO_TILE, true, true).mm);
    c.sieve_trim = 0;
    CHECK(!pair_form(c, ALGO_SIEVE, true, false).mm16 && pair_form(c, ALGO_SIEVE, true, true).mm);
    c.sieve_trim = 1, c.sieve_cpl = 4;
    CHECK(!pair_form(c, ALGO_SIEVE, true, false).mm16);
    return 0;
}

static int walked() {
    tsc_options c;   // default options
    {   // 57 046 structures in 5 chunks: 57 046 / 5 = 11 409, the last chunk 57 046 - 4 x 11 409 = 11 410; ceil(57 046 / 16) = 3 566 row tiles;
        // the 16-row matrix-core kernel: 11 410 >= 8 192 columns a row: 1 024 columns; ceil((11 410 + 64) / 1 024) = ceil(11.2) = 12 segments;
        // 11 474 <= 64 x 512: two items per workgroup, 3 566 / 2 = 1 783
        const WalkedPlan w = plan_walked(c, 57046, 5, 0, 1, 57046, -1, MM16);
        CHECK(w.rows == 57046 && w.n_tiles == 3566 && w.max_range == 11410 && w.seg_cols == 1024 && w.n_seg == 12 && w.mm16_waves == 2);
        CHECK(is_grid(w.grid, 1783, 12));
        // the packed-fp32 kernel: n <= 100 000: 512 columns, and 11 410 >= 4 x 512 keeps them; ceil(11 474 / 512) = 23; four wavefronts: 892
        const WalkedPlan q = plan_walked(c, 57046, 5, 0, 1, 57046, -1, PACKED);
        CHECK(q.seg_cols == 512 && q.n_seg == 23 && is_grid(q.grid, 892, 23));
        CHECK(pass_shape(c, 57046, 5, ALGO_SIEVE, true, false, false, 1, false, whole_pass(57046, 5)).longest_of_pass == 11410);
        CHECK(pass_shape(c, 57046, 5, ALGO_SIEVE, true, false, false, 1, false, whole_pass(57046, 5)).chunk == 11409);
    }
    {   // ... in 2 000 chunks of 28: the last is 57 046 - 1 999 x 28 = 1 074 long; 1 074 < 4 x 512 halves the segments to 256, where the
        // halving stops; ceil((1 074 + 64) / 256) = ceil(4.45) = 5
        const WalkedPlan w = plan_walked(c, 57046, 2000, 0, 1, 57046, -1, MM16);
        CHECK(w.max_range == 1074 && w.seg_cols == 256 && w.n_seg == 5 && w.mm16_waves == 2 && is_grid(w.grid, 1783, 5));
    }
    {   // a range of more than MM16_LONG_SEGS = 64 segments of 512 columns: max_range + 64 > 32 768, i.e. a chunk of 32 705, which the
        // one-chunk pass of 32 705 structures is the smallest run to have: four items per workgroup, whatever the segments' own length
        // (1 024: ceil(32 769 / 1 024) = 33); ceil(32 705 / 16) = 2 045 tiles: ceil(2 045 / 4) = 512
        const WalkedPlan w = plan_walked(c, 32705, 1, 0, 1, 32705, -1, MM16);
        CHECK(w.seg_cols == 1024 && w.n_seg == 33 && w.mm16_waves == 4 && w.n_tiles == 2045 && is_grid(w.grid, 512, 33));
        // ... one structure fewer: 32 768 / 1 024 = 32 segments, two items: 2 044 / 2 = 1 022
        const WalkedPlan v = plan_walked(c, 32704, 1, 0, 1, 32704, -1, MM16);
        CHECK(v.n_seg == 32 && v.mm16_waves == 2 && is_grid(v.grid, 1022, 32));
        // the packed-fp32 kernel: four wavefronts per workgroup whatever the segments
        CHECK(plan_walked(c, 32704, 1, 0, 1, 32704, -1, PACKED).mm16_waves == 4 && is_grid(plan_walked(c, 32704, 1, 0, 1, 32704, -1, PACKED).grid, 511, 64));
    }
    {   // 9 000 structures, 563 tiles, two items per workgroup: 282; 20 chunks of 450: 256 columns, ceil(514 / 256) = 3  [trace]; 10 chunks of
        // 900: ceil(964 / 256) = 4  [trace]; rank 1 of 3: (563 - 1 + 2) / 3 = 188 tiles, 94 workgroups  [trace]; the 64-row form:
        // ceil(141 groups / 4) = 36 workgroups, ceil(514 / 512) = 2 segments  [trace]
        CHECK(is_grid(plan_walked(c, 9000, 20, 0, 1, 9000, -1, MM16).grid, 282, 3) && is_grid(plan_walked(c, 9000, 10, 0, 1, 9000, -1, MM16).grid, 282, 4));
        CHECK(is_grid(plan_walked(c, 9000, 20, 1, 3, 9000, -1, MM16).grid, 94, 3) && is_grid(plan_walked(c, 9000, 20, 0, 1, 9000, -1, MM64).grid, 36, 2));
    }
    {   // the 64-row form: segments of 1 024 columns where a row's range reaches 2 048, else 512 (whatever the halving above left);
        // 2 047 rows: ceil(2 111 / 512) = 5 segments, ceil(2 047 / 64) = 32 groups in workgroups of MM_WAVES = 4: 8
        const WalkedPlan a = plan_walked(c, 2047, 1, 0, 1, 2047, -1, MM64);
        CHECK(a.seg_cols == 512 && a.n_seg == 5 && is_grid(a.grid, 8, 5));
        // 2 048 rows: ceil(2 112 / 1 024) = 3 segments, 32 groups again
        const WalkedPlan b = plan_walked(c, 2048, 1, 0, 1, 2048, -1, MM64);
        CHECK(b.seg_cols == 1024 && b.n_seg == 3 && is_grid(b.grid, 8, 3));
        tsc_options o;
        o.mm_seg_cols = 2048, o.seg_cols = 128;   // the options override: "mm_seg_cols" the 64-row form, "seg_cols" the others (no halving below 256)
        CHECK(plan_walked(o, 2048, 1, 0, 1, 2048, -1, MM64).seg_cols == 2048 && plan_walked(o, 2048, 1, 0, 1, 2048, -1, MM16).seg_cols == 128);
    }
    {   // 126 000 and 483 000 structures: 1 024 and 4 096 columns (k = 1: nothing to halve)
        CHECK(plan_walked(c, 126000, 1, 0, 1, 126000, -1, PACKED).seg_cols == 1024 && plan_walked(c, 483000, 1, 0, 1, 483000, -1, PACKED).seg_cols == 4096);
        // 483 000 in 100 chunks of 4 830: 4 830 < 4 x 4 096 and < 4 x 2 048, not < 4 x 1 024: 1 024 columns
        CHECK(plan_walked(c, 483000, 100, 0, 1, 483000, -1, PACKED).seg_cols == 1024);
    }
    {   // rank 2 of 3 on the 3 566 tiles of the first case (3 566 = 3 x 1 188 + 2): the tiles 2, 5, ... 3 563 are (3 566 - 2 + 2) / 3 = 1 188,
        // in workgroups of four: 297; rank 0 has the tiles 0, 3, ... 3 564: (3 566 + 2) / 3 = 1 189 -> 298
        CHECK(is_grid(plan_walked(c, 57046, 5, 2, 3, 57046, -1, PACKED).grid, 297, 23) && is_grid(plan_walked(c, 57046, 5, 0, 3, 57046, -1, PACKED).grid, 298, 23));
        // the 64-row form deals groups: ceil(57 046 / 64) = 892, rank 2 of 3 takes (892 - 2 + 2) / 3 = 297 -> ceil(297 / 4) = 75 workgroups;
        // 11 410 >= 2 048: ceil(11 474 / 1 024) = 12 segments
        CHECK(is_grid(plan_walked(c, 57046, 5, 2, 3, 57046, -1, MM64).grid, 75, 12));
    }
    {   // rows_now sizes the grid's x only: no row and one row are one tile, one workgroup; 33 rows are three tiles, two workgroups of two
        // items; more rows than the bound are the bound
        for (int64_t now : {0, 1}) {
            const WalkedPlan w = plan_walked(c, 57046, 5, 0, 1, 57046, now, MM16);
            CHECK(is_grid(w.grid, 1, 12) && w.rows == 57046 && w.n_tiles == 3566);
        }
        CHECK(is_grid(plan_walked(c, 57046, 5, 0, 1, 57046, 33, MM16).grid, 2, 12) && is_grid(plan_walked(c, 57046, 5, 0, 1, 57046, 60000, MM16).grid, 1783, 12));
        CHECK(is_grid(plan_walked(c, 57046, 5, 0, 1, 57046, 65, MM64).grid, 1, 12));   // (two groups of 64 rows: one workgroup)
        // a pass without rows (a rank of a partitioned pass that has no chunk): sized as one row
        const WalkedPlan e = plan_walked(c, 9000, 2, 0, 1, 0, -1, MM16);
        CHECK(e.rows == 1 && e.n_tiles == 1 && e.max_range == 1 && is_grid(e.grid, 1, 1));
    }
    {   // mm16_item_shape on either side of its thresholds.  8 191 columns a row: 512, ceil(8 255 / 512) = 17; 8 192: 1 024, ceil(8 256 / 1 024) = 9
        const Mm16Shape a = mm16_item_shape(8191), b = mm16_item_shape(8192);
        CHECK(a.seg_cols == 512 && a.waves == 2 && b.seg_cols == 1024 && b.waves == 2);
        CHECK(plan_walked(c, 8191, 1, 0, 1, 8191, -1, MM16).n_seg == 17 && plan_walked(c, 8192, 1, 0, 1, 8192, -1, MM16).n_seg == 9);
        // the halving: 2 048 columns keep 512 (four segments), 2 047 take 256, and so does everything shorter
        CHECK(mm16_item_shape(2048).seg_cols == 512 && mm16_item_shape(2047).seg_cols == 256 && mm16_item_shape(1).seg_cols == 256);
        // 57 046 structures: 10 chunks of 5 704, the last 5 710: 512, ceil(5 774 / 512) = 12; 2 chunks of 28 523: 1 024, ceil(28 587 / 1 024) = 28, two
        // items; one chunk: ceil(57 110 / 1 024) = 56 segments, 57 110 > 32 768: four items, ceil(3 566 / 4) = 892 workgroups
        const WalkedPlan k10 = plan_walked(c, 57046, 10, 0, 1, 57046, -1, MM16), k2 = plan_walked(c, 57046, 2, 0, 1, 57046, -1, MM16), k1 = plan_walked(c, 57046, 1, 0, 1, 57046, -1, MM16);
        CHECK(k10.max_range == 5710 && k10.seg_cols == 512 && k10.n_seg == 12 && k10.mm16_waves == 2);
        CHECK(k2.max_range == 28523 && k2.seg_cols == 1024 && k2.n_seg == 28 && k2.mm16_waves == 2 && is_grid(k2.grid, 1783, 28));
        CHECK(k1.seg_cols == 1024 && k1.n_seg == 56 && k1.mm16_waves == 4 && is_grid(k1.grid, 892, 56));
        // "seg_cols" = 256 on 16 321 structures in one chunk: ceil(16 385 / 256) = 65 segments, 16 385 > 64 x 256: four items, 1 021 tiles in
        // ceil(1 021 / 4) = 256 workgroups; one structure fewer: 64 segments, two items, 1 020 / 2 = 510
        tsc_options o;
        o.seg_cols = 256;
        const WalkedPlan s = plan_walked(o, 16321, 1, 0, 1, 16321, -1, MM16), t = plan_walked(o, 16320, 1, 0, 1, 16320, -1, MM16);
        CHECK(s.seg_cols == 256 && s.n_seg == 65 && s.mm16_waves == 4 && is_grid(s.grid, 256, 65));
        CHECK(t.n_seg == 64 && t.mm16_waves == 2 && is_grid(t.grid, 510, 64));
        o.seg_cols = 512;   // ... = 512: ceil(16 385 / 512) = 33 segments, two items
        CHECK(plan_walked(o, 16321, 1, 0, 1, 16321, -1, MM16).n_seg == 33 && plan_walked(o, 16321, 1, 0, 1, 16321, -1, MM16).mm16_waves == 2);
    }
    {   // the shapes of tests/test_walked_items.py: {structures, "seg_cols", the length and the segments its k = 1 pass must have}.  A forced length
        // is halved while the range is shorter than four segments: the "end" cases stand at n + 64 = m x length - 1, + 0, + 1 with n >= 4 x length
        const int cases[][4] = {{191, 256, 256, 1}, {192, 256, 256, 1}, {193, 256, 256, 2}, {447, 256, 256, 2}, {448, 256, 256, 2}, {449, 256, 256, 3},
                                {2495, 512, 512, 5}, {2496, 512, 512, 5}, {2497, 512, 512, 6}, {3007, 512, 512, 6}, {3008, 512, 512, 6}, {3009, 512, 512, 7},
                                {5055, 1024, 1024, 5}, {5056, 1024, 1024, 5}, {5057, 1024, 1024, 6}, {6079, 1024, 1024, 6}, {6080, 1024, 1024, 6},
                                {6081, 1024, 1024, 7}, {10175, 2048, 2048, 5}, {10176, 2048, 2048, 5}, {10177, 2048, 2048, 6},
                                {1000, 256, 256, 5}, {4200, 1024, 1024, 5}, {8256, 2048, 2048, 5},
                                // the rule's own choice: 1 000, 2 047 -> 256; 2 048, 2 111, 3 000, 8 191 -> 512; 8 192, 9 000 -> 1 024
                                {1000, 0, 256, 5}, {2047, 0, 256, 9}, {2048, 0, 512, 5}, {2111, 0, 512, 5}, {3000, 0, 512, 6}, {8191, 0, 512, 17},
                                {8192, 0, 1024, 9}, {9000, 0, 1024, 9}, {16321, 256, 256, 65}};
        const int ks[] = {2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1};
        for (const auto &cs : cases) {
            tsc_options o;
            o.seg_cols = cs[1];
            const WalkedPlan k1 = plan_walked(o, cs[0], 1, 0, 1, cs[0], -1, MM16);
            CHECK(k1.max_range == cs[0] && k1.seg_cols == cs[2] && k1.n_seg == cs[3]);
            // every pass of the schedule (rmsd_pruning.py:186-192: k chunks while 20 k < n): the segments cover a row's range from the 64-aligned
            // column below it, and a column offset inside a segment fits MM16_OFFSET_BITS bits
            for (int k : ks) {
                if (k != 1 && 20 * k >= cs[0]) continue;
                const WalkedPlan w = plan_walked(o, cs[0], k, 0, 1, cs[0], -1, MM16);
                CHECK(int64_t(w.n_seg) * w.seg_cols >= w.max_range + 64 && w.seg_cols <= (1 << MM16_OFFSET_BITS) && w.seg_cols >= 1);
                CHECK((w.mm16_waves == 2 || w.mm16_waves == 4) && w.grid.y == unsigned(w.n_seg) && int(w.grid.x) * w.mm16_waves >= w.n_tiles);
            }
        }
        // the dense case's k = 2 pass (chunks of 4 128): the forced 2 048 halved to 1 024, ceil(4 192 / 1 024) = 5
        tsc_options o;
        o.seg_cols = 2048;
        CHECK(plan_walked(o, 8256, 2, 0, 1, 8256, -1, MM16).seg_cols == 1024 && plan_walked(o, 8256, 2, 0, 1, 8256, -1, MM16).n_seg == 5);
    }
    {   // a run beyond 100 000 structures on the 16-row kernel keeps the length of its size as the floor: 126 000 in one chunk 1 024, 483 000 4 096;
        // 483 000 in 100 chunks of 4 830: 4 096 halved twice, 1 024 (as the packed-fp32 kernel's above)
        CHECK(plan_walked(c, 126000, 1, 0, 1, 126000, -1, MM16).seg_cols == 1024 && plan_walked(c, 483000, 1, 0, 1, 483000, -1, MM16).seg_cols == 4096);
        CHECK(plan_walked(c, 483000, 100, 0, 1, 483000, -1, MM16).seg_cols == 1024 && mm16_item_shape(5000, 1024).seg_cols == 1024 && mm16_item_shape(5000).seg_cols == 512);
    }
    return 0;
}

static int chunk_local() {
    tsc_options c;
    auto shape = [&](int64_t n, int64_t k, const PassRows &r, bool range) { return pass_shape(c, n, k, ALGO_SIEVE, true, false, false, 1, range, r); };
    {   // 9 000 in 200 chunks of 45 (the last: 9 000 - 199 x 45 = 45): three row tiles a chunk, one block of LP_TILES_PER_BLOCK = 4: 200 blocks  [trace]
        const LocalPlan l = plan_local(9000, 200, whole_pass(9000, 200));
        CHECK(shape(9000, 200, whole_pass(9000, 200), false).local && l.nb_regular == 1 && l.nb_last == 1 && l.n_reg == 199 && l.blocks == 200);
        // 100 chunks of 90: ceil(90 / 16) = 6 tiles, two blocks a chunk: 99 x 2 + 2 = 200  [trace]
        const LocalPlan m = plan_local(9000, 100, whole_pass(9000, 100));
        CHECK(shape(9000, 100, whole_pass(9000, 100), false).local && m.nb_regular == 2 && m.nb_last == 2 && m.n_reg == 99 && m.blocks == 200);
        // 50 chunks of 180: 12 tiles, three blocks: 150  [trace]
        const LocalPlan s = plan_local(9000, 50, whole_pass(9000, 50));
        CHECK(shape(9000, 50, whole_pass(9000, 50), false).local && s.nb_regular == 3 && s.nb_last == 3 && s.n_reg == 49 && s.blocks == 150);
        // 20 chunks of 450 > local_max_chunk = 384: not local -- nor is anything with "local_pass" off, dealt to several ranks, or of the
        // register-tiled kernel
        CHECK(!shape(9000, 20, whole_pass(9000, 20), false).local);
        CHECK(!pass_shape(c, 9000, 200, ALGO_SIEVE, true, false, false, 2, false, whole_pass(9000, 200)).local);
        CHECK(!pass_shape(c, 9000, 200, ALGO_TILE, false, false, false, 1, false, whole_pass(9000, 200)).local);
        tsc_options off;
        off.local_pass = 0;
        CHECK(!pass_shape(off, 9000, 200, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 200)).local);
    }
    {   // the pass of 200 chunks partitioned over 2 ranks: rank 1's block starts at structure 4 500 = chunk 100, so rank 0 has the chunks
        // [0, 100) -- all regular, the last chunk of the pass is not its own: 100 blocks -- and rank 1 [100, 200): 99 regular and the last
        const PassRows r0 = partition_bounds(9000, 200, 0, 2), r1 = partition_bounds(9000, 200, 1, 2);
        CHECK(r0.c_lo == 0 && r0.c_hi == 100 && r0.s_lo == 0 && r0.s_hi == 4500 && r1.c_lo == 100 && r1.c_hi == 200 && r1.s_lo == 4500 && r1.s_hi == 9000);
        const LocalPlan a = plan_local(9000, 200, r0), b = plan_local(9000, 200, r1);
        CHECK(a.nb_last == 0 && a.n_reg == 100 && a.blocks == 100 && b.nb_last == 1 && b.n_reg == 99 && b.blocks == 100);
        CHECK(shape(9000, 200, r0, true).local && shape(9000, 200, r0, true).rows_ub == 4500 && shape(9000, 200, r0, true).longest_of_rank == 45);
        // 300 ranks: rank 2's block [60, 90) holds no chunk start (chunks start at 45 and 90): c_lo == c_hi == 2, no rows, not local
        const PassRows none = partition_bounds(9000, 200, 2, 300);
        CHECK(none.c_lo == 2 && none.c_hi == 2 && none.s_lo == 90 && none.s_hi == 90);
        CHECK(!shape(9000, 200, none, true).local && shape(9000, 200, none, true).rows_ub == 1);
    }
    {   // the longest chunk counts: 767 structures in 2 chunks are 383 and 384 -- local, 24 tiles = 6 blocks each --; 769 are 384 and 385: not.
        // To a rank that holds only the first chunk of the 769 its own longest, 384, counts.
        const PassShape a = shape(767, 2, whole_pass(767, 2), false), b = shape(769, 2, whole_pass(769, 2), false);
        CHECK(a.local && a.chunk == 383 && a.longest_of_pass == 384 && a.longest_of_rank == 384);
        CHECK(!b.local && b.chunk == 384 && b.longest_of_pass == 385);
        CHECK(plan_local(767, 2, whole_pass(767, 2)).nb_regular == 6 && plan_local(767, 2, whole_pass(767, 2)).nb_last == 6 && plan_local(767, 2, whole_pass(767, 2)).blocks == 12);
        const PassShape h = shape(769, 2, PassRows{0, 1, 0, 384}, true);
        CHECK(h.local && h.longest_of_rank == 384 && h.longest_of_pass == 385);
    }
    return 0;
}

static int culled() {
    tsc_options c;
    c.cull = 2, c.cull_min_pairs = 5e6;
    {   // 9 000 in 5 chunks of 1 800: 9 000 x 1 800 / 2 = 8.1e6 pairs >= 5e6: a candidate; in 10 chunks 4.05e6: not
        CHECK(pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 5)).culled);
        CHECK(!pass_shape(c, 9000, 10, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 10)).culled);
        // one rank: ceil(9 000 / 16) = 563 tiles, ceil((1 800 + 256) / 4 096) = 1 segment, ceil(563 / 4) = 141 items; keyed to XCDs:
        // ceil(141 / 32) = 5 runs, ceil(5 / 8) = 1 per XCD: 8 x 1 x 1 x 32 = 256 workgroups  [trace]; else one per item: 141
        const CulledPlan q = plan_culled(c, 9000, 1800, 0, 1, false);
        CHECK(q.tile_block == 1 && q.my_tiles == 563 && q.n_seg == 1 && q.sgrid == 256 && q.n_groups == 0 && q.grid_mm == 0);
        // the matrix-core form: ceil(9 000 / 64) = 141 groups, ceil(2 056 / 1 024) = 3 segments: 8 x 3 x 1 x 32 = 768  [trace]; else 141 x 3 = 423
        const CulledPlan m = plan_culled(c, 9000, 1800, 0, 1, true);
        CHECK(m.n_groups == 141 && m.n_seg_mm == 3 && m.grid_mm == 768 && m.sgrid == 256);
        c.cull_xcd = 0;
        CHECK(plan_culled(c, 9000, 1800, 0, 1, false).sgrid == 141 && plan_culled(c, 9000, 1800, 0, 1, true).grid_mm == 423);
        c.cull_grid = 100;   // "cull_grid" caps the workgroups of the form that walks its items
        CHECK(plan_culled(c, 9000, 1800, 0, 1, false).sgrid == 100);
        c.cull_grid = 1 << 30, c.cull_xcd = 1;
    }
    {   // 5 ranks, runs of 16 tiles: (563 / 80 + 1) x 16 = 128 slots a rank, whichever: 32 items; keyed: 8 x 1 x ceil(1 / 8) x 32 = 256  [trace]
        c.cull_tile_block = 16;
        for (int rank : {0, 4}) {
            const CulledPlan q = plan_culled(c, 9000, 1800, rank, 5, false);
            CHECK(q.tile_block == 16 && q.my_tiles == 128 && q.n_seg == 1 && q.sgrid == 256);
            // groups in runs of 16 / 4 = 4: (141 / 20 + 1) x 4 = 32; 8 x 3 x 1 x 32 = 768  [trace]
            const CulledPlan m = plan_culled(c, 9000, 1800, rank, 5, true);
            CHECK(m.n_groups == 32 && m.n_seg_mm == 3 && m.grid_mm == 768);
        }
        c.cull_xcd = 0;
        CHECK(plan_culled(c, 9000, 1800, 3, 5, false).sgrid == 32 && plan_culled(c, 9000, 1800, 3, 5, true).grid_mm == 96);
        // tiles one by one: rank 2 has the tiles 2, 7, ... 562: (563 - 2 + 4) / 5 = 113 -> ceil(113 / 4) = 29 items; a block of 0 counts as 1
        c.cull_tile_block = 1;
        CHECK(plan_culled(c, 9000, 1800, 2, 5, false).my_tiles == 113 && plan_culled(c, 9000, 1800, 2, 5, false).sgrid == 29);
        c.cull_tile_block = 0;
        CHECK(plan_culled(c, 9000, 1800, 2, 5, false).tile_block == 1 && plan_culled(c, 9000, 1800, 2, 5, true).n_groups == (141 / 5 + 1));
        c.cull_tile_block = 256, c.cull_xcd = 1;
    }
    {   // row tiles dealt to 5 ranks: a rank looks at 8.1e6 / 5 = 1.62e6 pairs and needs TWICE the threshold -- 0.8e6 passes (1.6e6), 0.82e6
        // does not (1.64e6) -- and descriptors that are the same bits on every rank
        c.cull_min_pairs = 0.8e6;
        CHECK(pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, true, 5, false, whole_pass(9000, 5)).culled);
        CHECK(!pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 5, false, whole_pass(9000, 5)).culled);
        c.cull_min_pairs = 0.82e6;
        CHECK(!pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, true, 5, false, whole_pass(9000, 5)).culled);
        // a rank's own chunks of a partitioned pass: its share against the threshold itself, no condition on the descriptors --
        // rank 1 of 5 holds chunk 1, 1 800 structures x 1 800 / 2 = 1.62e6 >= 0.82e6
        const PassRows r = partition_bounds(9000, 5, 1, 5);
        CHECK(r.c_lo == 1 && r.c_hi == 2 && r.s_lo == 1800 && r.s_hi == 3600);
        CHECK(pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 1, true, r).culled);
        c.cull_min_pairs = 1.63e6;
        CHECK(!pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 1, true, r).culled);
    }
    {   // every pass of fewer than CULL_MAX_CHUNKS = 64 chunks that is not chunk-local: 50 chunks yes, 64 no; never with cull = 0, another
        // screen shape or the register-tiled kernel
        c.cull_min_pairs = 0, c.local_pass = 0;
        CHECK(pass_shape(c, 9000, 50, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 50)).culled);
        CHECK(!pass_shape(c, 9000, 64, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 64)).culled);
        CHECK(!pass_shape(c, 9000, 5, ALGO_TILE, false, false, false, 1, false, whole_pass(9000, 5)).culled);
        c.local_pass = 1;
        const PassShape l = pass_shape(c, 9000, 50, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 50));
        CHECK(l.local && !l.culled && !l.fused);
        c.sieve_cpl = 4;
        CHECK(!pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 5)).culled);
        c.sieve_cpl = 2, c.cull = 0;
        CHECK(!pass_shape(c, 9000, 5, ALGO_SIEVE, true, false, false, 1, false, whole_pass(9000, 5)).culled);
    }
    return 0;
}

static int decisions() {
    tsc_options c;
    c.cull = 2, c.cull_min_pairs = 5e6;
    auto shape = [&](int64_t k, int algo, bool records, bool mm64, int world, bool range) {
        return pass_shape(c, 9000, k, algo, records, mm64, false, world, range, whole_pass(9000, k));
    };
    // the fp32 descriptors by position: not for a matrix-core kernel's walked pass (k = 10), but for its culled pass (k = 5: the layout
    // reads them), and for the packed-fp32 kernels either way; the register-tiled kernel's k_open_rows is handed the buffer it has not
    CHECK(!shape(10, ALGO_SIEVE, true, false, 1, false).need_dc && !shape(10, ALGO_SIEVE, true, true, 1, false).need_dc);
    CHECK(shape(5, ALGO_SIEVE, true, false, 1, false).need_dc && shape(5, ALGO_SIEVE, true, true, 1, false).need_dc);
    CHECK(shape(10, ALGO_SIEVE, false, false, 1, false).need_dc && shape(5, ALGO_SIEVE, false, false, 1, false).need_dc);
    CHECK(shape(10, ALGO_TILE, false, false, 1, false).need_dc);
    c.sieve_trim = 0;   // (no 16-row matrix-core kernel for this screen: the packed-fp32 one, which reads them)
    CHECK(shape(10, ALGO_SIEVE, true, false, 1, false).need_dc && !shape(10, ALGO_SIEVE, true, true, 1, false).need_dc);
    c.sieve_trim = 1;
    // the pair kernel applies the verdicts: one rank's sieve pass under "fused_apply", and a partitioned pass whatever the option
    CHECK(shape(10, ALGO_SIEVE, true, false, 1, false).fused && !shape(10, ALGO_SIEVE, true, false, 3, false).fused && !shape(10, ALGO_TILE, false, false, 1, false).fused);
    c.fused_apply = 0;
    CHECK(!shape(10, ALGO_SIEVE, true, false, 1, false).fused && shape(10, ALGO_SIEVE, true, false, 1, true).fused);
    // k_open_rows: 9 000 rows are 563 tiles in ceil(563 / 16) = 36 workgroups  [trace]; one row is one of each
    CHECK(plan_open_rows(9000).n_tiles == 563 && plan_open_rows(9000).blocks == 36 && plan_open_rows(9000).stamp_blocks == 141);
    CHECK(plan_open_rows(1).n_tiles == 1 && plan_open_rows(1).blocks == 1 && plan_open_rows(257).n_tiles == 17 && plan_open_rows(257).blocks == 2);
    // the thresholds: maxdev_thr = 2 thr (:95); the near-duplicate test from four heavy atoms on
    const Thresholds t = thresholds(30, 0.5), u = thresholds(3, 0.5);
    CHECK(t.thr == 0.5 && t.maxdev_thr == 1.0 && t.half_h_thr2 == 3.75 && t.two_thr2 == 0.5 && t.desc_limit == 7.5);
    CHECK(u.two_thr2 == -1.0 && u.half_h_thr2 == 0.375 && u.desc_limit == 0.75 && thresholds(4, 0.5).two_thr2 == 0.5);
    return 0;
}

int main() {
    if (forms() || walked() || chunk_local() || culled() || decisions()) return 1;
    printf("pass_plan_check: %d checks passed\n", g_checks);
    return 0;
}
