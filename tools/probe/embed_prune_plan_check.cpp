// embed_prune_plan_check.cpp -- the sizing functions of csrc/embed_prune_plan.hpp (how an embed-and-prune run's device buffers grow as slabs
// append their kept poses, where a slab's rows start, what a row costs) run by a stand-alone program at sizes worked out by hand, so that they
// can be checked without a GPU and built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library;
// tools/embed_prune_plan_check.py builds and runs it.  No HIP call is made.  The last part replays a run's appends on host arrays standing
// for the device buffers: every copy and every write must stay inside what was allocated, which is what ASan watches.
//
//   embed_prune_plan_check   (exit status 0 and a line "embed_prune_plan_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tscode_amd/csrc/embed_prune_plan.hpp"

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

static int capacities() {
    // nothing wanted: nothing allocated, whatever is there stays
    CHECK(ep_grown_capacity(0, 0) == 0 && ep_grown_capacity(1024, 0) == 1024 && ep_grown_capacity(4096, 0) == 4096);
    // the first row takes the first allocation, EP_MIN_ROWS = 1024 rows, and so does every count up to it
    CHECK(EP_MIN_ROWS == 1024);
    CHECK(ep_grown_capacity(0, 1) == 1024 && ep_grown_capacity(0, 1023) == 1024 && ep_grown_capacity(0, 1024) == 1024);
    // one above: doubled once
    CHECK(ep_grown_capacity(0, 1025) == 2048 && ep_grown_capacity(1024, 1025) == 2048);
    // an exact power of two fits the capacity of that size, one above doubles it: 2^16 = 65 536
    CHECK(ep_grown_capacity(65536, 65536) == 65536 && ep_grown_capacity(65536, 65537) == 131072 && ep_grown_capacity(32768, 65536) == 65536);
    // while it fits nothing moves, also far below the capacity
    CHECK(ep_grown_capacity(2048, 1) == 2048 && ep_grown_capacity(2048, 2047) == 2048 && ep_grown_capacity(2048, 2048) == 2048);
    // a slab that brings more than twice what is there: doubled until it fits -- 1024 -> 2048 -> 4096 -> 8192 for 5000 rows
    CHECK(ep_grown_capacity(1024, 5000) == 8192 && ep_grown_capacity(0, 5000) == 8192);
    // config 5: 500 000 kept poses; 1024 * 2^9 = 524 288 is the first power-of-two multiple that holds them
    CHECK(ep_grown_capacity(0, 500000) == 524288 && ep_grown_capacity(262144, 500000) == 524288 && ep_grown_capacity(524288, 500000) == 524288);
    // the end of the range: the prune takes n < 2^31 - 1 - 4096, so EP_MAX_ROWS = 2 147 479 550; 2^30 doubles to 2^31 > EP_MAX_ROWS: clamped
    CHECK(EP_MAX_ROWS == 2147479550LL);
    CHECK(ep_grown_capacity(1LL << 30, (1LL << 30) + 1) == EP_MAX_ROWS && ep_grown_capacity(0, EP_MAX_ROWS) == EP_MAX_ROWS);
    CHECK(ep_grown_capacity(EP_MAX_ROWS, EP_MAX_ROWS) == EP_MAX_ROWS);
    // beyond it, and nonsense: refused
    CHECK(ep_grown_capacity(0, EP_MAX_ROWS + 1) == -1 && ep_grown_capacity(EP_MAX_ROWS, EP_MAX_ROWS + 1) == -1);
    CHECK(ep_grown_capacity(0, -1) == -1 && ep_grown_capacity(-1, 5) == -1 && ep_grown_capacity(0, INT64_MAX) == -1);
    return 0;
}

static int rows() {
    // config 5: 200 atoms, 120 heavy, three molecules: 24 * 120 + 100 * 3 = 3180 bytes per kept pose against 4800 of the pose itself
    CHECK(ep_row_bytes(120, 3) == 3180 && ep_row_bytes(1, 2) == 224 && ep_row_bytes(26, 2) == 824);
    // where a slab's rows start: row 0 at 0; row 500 000 of 360 doubles at 180 000 000; the last row the prune takes of a 600-double row
    // lies beyond 2^31 doubles (64-bit arithmetic): 2 147 479 549 * 600 = 1 288 487 729 400
    CHECK(ep_row_offset(0, 360) == 0 && ep_row_offset(1, 360) == 360 && ep_row_offset(500000, 360) == 180000000LL);
    CHECK(ep_row_offset(EP_MAX_ROWS - 1, 600) == 1288487729400LL);
    return 0;
}

// A run's life on host arrays: slabs of kept[i] rows appended one after the other, the buffer regrown as embed_prune_reserve regrows the
// device buffers (new block, the rows there so far copied, the old block dropped), each row filled with its own number.  Returns the
// number of regrowths, -1 where a row was lost.
static int replay(const std::vector<int64_t> &kept, int row_doubles, int64_t *final_cap) {
    std::vector<double> buf;
    int64_t cap = 0, n = 0;
    int grown = 0;
    for (int64_t k : kept) {
        const int64_t want = ep_grown_capacity(cap, n + k);
        if (want < 0) return -1;
        if (want != cap) {
            std::vector<double> next(size_t(want) * row_doubles);   // (exactly the capacity: one double past it is ASan's to find)
            if (n > 0) memcpy(next.data(), buf.data(), size_t(n) * row_doubles * sizeof(double));
            buf.swap(next);
            cap = want;
            ++grown;
        }
        double *at = buf.data() + ep_row_offset(n, row_doubles);
        for (int64_t r = 0; r < k; ++r)
            for (int w = 0; w < row_doubles; ++w) at[r * row_doubles + w] = double(n + r);
        n += k;
    }
    for (int64_t r = 0; r < n; ++r)
        for (int w = 0; w < row_doubles; ++w)
            if (buf[size_t(ep_row_offset(r, row_doubles)) + w] != double(r)) return -1;
    *final_cap = cap;
    return grown;
}

static int replays() {
    int64_t cap = -1;
    // nothing kept at all: nothing allocated
    CHECK(replay({0, 0, 0}, 9, &cap) == 0 && cap == 0);
    // one pose: one allocation of the first size
    CHECK(replay({1}, 9, &cap) == 1 && cap == 1024);
    // a slab that keeps nothing between two that do
    CHECK(replay({300, 0, 300}, 6, &cap) == 1 && cap == 1024);
    // exactly full, then one more: 1024 -> 2048, with 1024 rows to carry over
    CHECK(replay({1024}, 3, &cap) == 1 && cap == 1024);
    CHECK(replay({1024, 1}, 3, &cap) == 2 && cap == 2048);
    CHECK(replay({1000, 24, 1, 1023, 1}, 18, &cap) == 3 && cap == 4096);   // 1024 (full) | 1025 -> 2048 | 2048 (full) | 2049 -> 4096
    // many small slabs: 35 of 63 rows, 2205 in all -> 1024, 2048, 4096
    CHECK(replay(std::vector<int64_t>(35, 63), 78, &cap) == 3 && cap == 4096);
    // one slab far beyond the first size: allocated once, at the size that holds it
    CHECK(replay({70000}, 3, &cap) == 1 && cap == 131072);
    return 0;
}

int main() {
    if (capacities() || rows() || replays()) return 1;
    printf("embed_prune_plan_check: %d checks passed\n", g_checks);
    return 0;
}
