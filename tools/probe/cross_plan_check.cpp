// cross_plan_check.cpp -- the sizing functions of csrc/cross_plan.hpp (padded atom counts, segment width and count, grid, partial array, rows
// under a byte budget of a cross-set RMSD call) run by a stand-alone program at sizes worked out by hand, so that they can be checked
// without a GPU and built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library; tools/cross_plan_check.py builds
// and runs it.  No HIP runtime call is made.  The last part replays the indexing of the rectangle's work items on host arrays of exactly
// the sizes cross.hip allocates: every column a lane loads, every value, partial entry and row an item writes must lie inside them, which is
// what ASan watches.
//
//   cross_plan_check   (exit status 0 and a line "cross_plan_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <vector>

#include "../../tscode_amd/csrc/cross_plan.hpp"

using namespace tsc;

static int g_checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                            \
        }                                                        \
    } while (0)

static bool is_plan(const CrossPlan &p, int64_t n_tiles, int seg_cols, int n_seg, unsigned grid_x, int64_t partial) {
    return p.n_tiles == n_tiles && p.seg_cols == seg_cols && p.n_seg == n_seg && p.grid_x == grid_x && p.partial == partial;
}

static int layouts() {
    // padded atoms: 4 .. 32 in steps of 4, the general path beyond; the row pitch; whole 64-column tiles
    CHECK(cross_padded_atoms(1) == 4 && cross_padded_atoms(3) == 4 && cross_padded_atoms(4) == 4 && cross_padded_atoms(5) == 8);
    CHECK(cross_padded_atoms(29) == 32 && cross_padded_atoms(32) == 32 && cross_padded_atoms(33) == 0 && cross_padded_atoms(200) == 0);
    CHECK(cross_pitch(3) == 12 && cross_pitch(30) == 96 && cross_pitch(32) == 96 && cross_pitch(33) == 99 && cross_pitch(200) == 600);
    CHECK(cross_ld(1) == 64 && cross_ld(64) == 64 && cross_ld(65) == 128 && cross_ld(700) == 704 && cross_ld(2147483647LL) == 2147483648LL);
    return 0;
}

static int plans() {
    // one query against 10^6: 1 row tile, 4096 segments wanted, ceil(10^6 / 4096) = 245 -> 256 columns, ceil(10^6 / 256) = 3907 segments
    CHECK(is_plan(cross_plan(1, 1000000), 1, 256, 3907, 1, 3907));
    // 5 queries: still one tile
    CHECK(is_plan(cross_plan(5, 1000000), 1, 256, 3907, 1, 5 * 3907));
    // 64 queries against 100 000: 4 tiles, 1024 segments wanted, ceil(10^5 / 1024) = 98 -> 128 columns, 782 segments, one workgroup of rows
    CHECK(is_plan(cross_plan(64, 100000), 4, 128, 782, 1, 64 * 782));
    // 10^5 queries against 300: 6250 tiles fill the chip, one segment of 320 columns, 1563 workgroups
    CHECK(is_plan(cross_plan(100000, 300), 6250, 320, 1, 1563, 100000));
    // 10^5 against 1000: one segment of 1024
    CHECK(is_plan(cross_plan(100000, 1000), 6250, 1024, 1, 1563, 100000));
    // 4096 x 4096: 256 tiles, 16 segments wanted, 256 columns each
    CHECK(is_plan(cross_plan(4096, 4096), 256, 256, 16, 64, 16 * 4096));
    // the threshold: 65 520 queries are 4095 tiles (two segments wanted), 65 521 are 4096 (one)
    CHECK(is_plan(cross_plan(65520, 10000), 4095, 4096, 3, 1024, 3 * 65520));
    CHECK(is_plan(cross_plan(65521, 10000), 4096, 4096, 3, 1024, 3 * 65521));
    CHECK(is_plan(cross_plan(65520, 4000), 4095, 2048, 2, 1024, 2 * 65520));
    CHECK(is_plan(cross_plan(65521, 4000), 4096, 4032, 1, 1024, 65521));
    // the smallest: one pair; a segment never has less than one 64-column tile
    CHECK(is_plan(cross_plan(1, 1), 1, 64, 1, 1, 1));
    CHECK(is_plan(cross_plan(1, 65), 1, 64, 2, 1, 2));
    CHECK(is_plan(cross_plan(16, 63), 1, 64, 1, 1, 16));
    CHECK(is_plan(cross_plan(17, 64), 2, 64, 1, 1, 17));
    CHECK(is_plan(cross_plan(33, 130), 3, 64, 3, 1, 99));
    CHECK(is_plan(cross_plan(5, 700), 1, 64, 11, 1, 55));
    CHECK(is_plan(cross_plan(40, 3), 3, 64, 1, 1, 40));
    // the largest: 2^31 - 1 on a side.  Rows: 134 217 728 tiles, 33 554 432 workgroups wanted, 2^20 launched (the kernels stride).
    // Columns: ceil((2^31 - 1) / 65 535) = 32 769 -> 32 832 columns, ceil((2^31 - 1) / 32 832) = 65 409 segments
    CHECK(is_plan(cross_plan(2147483647LL, 300), 134217728LL, 320, 1, 1u << 20, 2147483647LL));
    CHECK(is_plan(cross_plan(1, 2147483647LL), 1, 32832, 65409, 1, 65409));
    const CrossPlan big = cross_plan(2147483647LL, 2147483647LL);
    CHECK(big.n_seg == 65409 && big.n_seg <= CX_MAX_SEGS && big.grid_x == (1u << 20) && big.partial == 65409LL * 2147483647LL);
    return 0;
}

static int budgets() {
    // values: 16 bytes per pair.  1 GiB against 4096 columns: 2^30 / 65 536 = 16 384 rows; against 10^6: 67 rows (67.1); against 2^31 - 1: 1 row
    CHECK(cross_value_rows(100000, 4096, int64_t(1) << 30) == 16384 && cross_value_rows(5000, 4096, int64_t(1) << 30) == 5000);
    CHECK(cross_value_rows(100000, 1000000, int64_t(1) << 30) == 67);
    CHECK(cross_value_rows(100000, 2147483647LL, int64_t(1) << 30) == 1 && cross_value_rows(7, 130, 0) == 1);
    // 33 rows of 130 columns under 25 000 bytes: 2080 bytes a row, 12 rows -- three blocks of 12, 12 and 9
    CHECK(cross_value_rows(33, 130, 25000) == 12);
    // nearest: 20 bytes per (segment, row), 64 MiB per launch: one query against 10^6 in one launch; 2^31 - 1 queries against 300 (one segment)
    // take 3 355 443 rows a launch (3 355 443.2); against 2^31 - 1 (65 409 segments, 1 308 180 bytes a row) 51 rows (51.3)
    CHECK(cross_nearest_rows(1, 3907) == 1 && cross_nearest_rows(100000, 1) == 100000);
    CHECK(cross_nearest_rows(2147483647LL, 1) == 3355443 && cross_nearest_rows(2147483647LL, 65409) == 51);
    return 0;
}

// The indexing of a launch (cross.hpp: k_cross_tile / k_cross_general and the nearest epilogue's partial arrays) on host arrays of the
// sizes cross.hip allocates.  grid_x_cap: workgroups along the rows (below the plan's: the stride over the row tiles is walked too).
// Returns the pairs visited, -1 where a pair is visited twice or a partial entry written twice.
static long long replay(int64_t nq, int64_t nl, unsigned grid_x_cap) {
    const CrossPlan p = cross_plan(nq, nl);
    const int64_t ld = cross_ld(nl);
    std::vector<unsigned char> col(size_t(ld), 0), seen(size_t(nq * nl), 0), part(size_t(p.partial), 0);
    const unsigned gx = p.grid_x < grid_x_cap ? p.grid_x : grid_x_cap;
    long long pairs = 0;
    for (int by = 0; by < p.n_seg; ++by)
        for (unsigned bx = 0; bx < gx; ++bx)
            for (int wid = 0; wid < CX_WAVES; ++wid) {
                const int64_t seg_lo = int64_t(by) * p.seg_cols, seg_hi = seg_lo + p.seg_cols < nl ? seg_lo + p.seg_cols : nl;
                for (int64_t tile = int64_t(bx) * CX_WAVES + wid; tile < p.n_tiles; tile += int64_t(gx) * CX_WAVES) {
                    const int64_t r0 = tile * CX_ROWS;
                    const int nrows = int(nq - r0 < CX_ROWS ? nq - r0 : CX_ROWS);
                    if (nrows < 1) return -1;
                    for (int64_t c0 = seg_lo; c0 < seg_hi; c0 += 64)
                        for (int lane = 0; lane < 64; ++lane) {
                            col[size_t(c0 + lane)] = 1;   // the lane's column load: inside the pack's ld columns
                            if (c0 + lane >= nl) continue;
                            for (int t = 0; t < nrows; ++t) {
                                unsigned char &s = seen[size_t((r0 + t) * nl + c0 + lane)];
                                if (s) return -1;
                                s = 1, ++pairs;
                            }
                        }
                    for (int t = 0; t < nrows; ++t) {
                        unsigned char &w = part[size_t(int64_t(by) * nq + r0 + t)];
                        if (w) return -1;
                        w = 1;
                    }
                }
            }
    for (unsigned char w : part)
        if (!w) return -1;
    return pairs;
}

static int replays() {
    // every pair once, every partial entry once, at the edges of the tiling: the test shapes, and strides over the row tiles
    CHECK(replay(1, 1, 1u << 20) == 1 && replay(1, 65, 1u << 20) == 65 && replay(16, 63, 1u << 20) == 16 * 63 && replay(17, 64, 1u << 20) == 17 * 64);
    CHECK(replay(33, 130, 1u << 20) == 33 * 130 && replay(5, 700, 1u << 20) == 3500 && replay(40, 3, 1u << 20) == 120 && replay(1, 700, 1u << 20) == 700);
    CHECK(replay(1000, 300, 3) == 300000);    // 63 tiles on 3 workgroups of 4: six turns, the last with 3 tiles
    CHECK(replay(129, 4097, 1) == 129 * 4097);
    return 0;
}

int main() {
    if (layouts() || plans() || budgets() || replays()) return 1;
    printf("cross_plan_check: %d checks passed\n", g_checks);
    return 0;
}
