// leader_plan_check.cpp -- the sizing functions of csrc/leader_plan.hpp (blocks of a run, rows of a block, capacity and leading dimension of
// the growing library pack, grid of the in-block bits, launches and read-backs of a run) run by a stand-alone program at sizes worked out by
// hand, so that they can be checked without a GPU and built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library;
// tools/leader_plan_check.py builds and runs it.  No HIP runtime call is made.  The last part replays the indexing of a run on host arrays
// of exactly the sizes leader.hip allocates -- the bit words the work items write and the replay reads, the rows, columns and norms the
// append writes, the library walk's column loads -- which is what ASan watches.
//
//   leader_plan_check   (exit status 0 and a line "leader_plan_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <vector>

#include "../../tscode_amd/csrc/leader_plan.hpp"

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

static int sizes() {
    const int64_t B = LEADER_BLOCK, BIG = 2147483647LL;
    CHECK(B % 64 == 0 && LEADER_WORDS * 64 == B);
    // blocks and the rows of the last one at N = 1, B - 1, B, B + 1 and 2^31 - 1
    CHECK(leader_blocks(0) == 0 && leader_blocks(1) == 1 && leader_blocks(B - 1) == 1 && leader_blocks(B) == 1 && leader_blocks(B + 1) == 2);
    CHECK(leader_blocks(BIG) == (BIG + B - 1) / B);
    CHECK(leader_block_rows(1, 0) == 1 && leader_block_rows(B - 1, 0) == B - 1 && leader_block_rows(B, 0) == B);
    CHECK(leader_block_rows(B + 1, 0) == B && leader_block_rows(B + 1, 1) == 1);
    CHECK(leader_block_rows(BIG, 0) == B && leader_block_rows(BIG, leader_blocks(BIG) - 1) == int(BIG - (leader_blocks(BIG) - 1) * B));
    CHECK(leader_block_rows(BIG, leader_blocks(BIG) - 1) >= 1 && leader_block_rows(BIG, leader_blocks(BIG) - 1) <= B);
    // the pack: room for the library and every row; whole 64-column tiles
    CHECK(leader_capacity(0, 1) == 1 && leader_ld(0, 1) == 64 && leader_ld(0, 64) == 64 && leader_ld(1, 64) == 128);
    CHECK(leader_ld(0, B - 1) == B && leader_ld(0, B) == B && leader_ld(0, B + 1) == B + 64 && leader_ld(300, B) == cx_round_up(B + 300, 64));
    CHECK(leader_capacity(0, BIG) == BIG && leader_ld(0, BIG) == 2147483648LL && leader_ld(BIG - 5, 5) == 2147483648LL);
    // the bits grid: row tiles four to a workgroup, 64-column tiles
    CHECK(leader_bits_grid(1).x == 1 && leader_bits_grid(1).y == 1 && leader_bits_grid(64).x == 1 && leader_bits_grid(65).x == 2 && leader_bits_grid(65).y == 2);
    CHECK(leader_bits_grid(int(B)).x == unsigned(B / 64) && leader_bits_grid(int(B)).y == unsigned(B / 64));
    CHECK(leader_bits_grid(int(B) - 1).x == unsigned(B / 64) && leader_bits_grid(int(B) - 1).y == unsigned(B / 64));
    // launches: one block without library or order: pack, 2 fills (+1 on the register path), bits, replay = 5 (6); one read-back
    CHECK(leader_counts(1, 0, false, false).launches == 5 && leader_counts(1, 0, false, true).launches == 6 && leader_counts(1, 0, false, true).readbacks == 1);
    // B + 1 rows, ordered, with a library, register path: gather, 2 packs, 3 fills, 2 walks, 2 x (bits, replay), 1 append = 13
    CHECK(leader_counts(B + 1, 10, true, true).launches == 13 && leader_counts(B + 1, 10, true, true).blocks == 2);
    // ... without a library the first block has no walk
    CHECK(leader_counts(B + 1, 0, true, true).launches == 11);
    CHECK(leader_counts(0, 0, false, false).blocks == 0 && leader_counts(0, 0, false, false).readbacks == 0);
    return 0;
}

// One run on host arrays of the sizes leader.hip allocates.  keep_every: row s of the order is accepted iff s % keep_every == 0 (1: the
// worst case for the pack, everything kept).  Returns the rows kept, -1 on an inconsistency.
static long long replay(int64_t n, int64_t n_library, int pitch, int keep_every) {
    const int64_t capacity = leader_capacity(n_library, n), ld = leader_ld(n_library, n);
    std::vector<double> Lr(size_t(capacity) * pitch, 0.0), Lc(size_t(ld) * pitch, 0.0), Lg(size_t(ld), 0.0);
    std::vector<unsigned long long> bits(size_t(LEADER_BLOCK) * LEADER_WORDS, 0);
    std::vector<int> acc_pos(size_t(LEADER_BLOCK), 0), kept_src(size_t(n), -1);
    std::vector<unsigned char> filled(size_t(capacity), 0);
    for (int64_t l = 0; l < n_library; ++l) filled[size_t(l)] = 1;
    int64_t kept = 0;
    for (int64_t b = 0; b < leader_blocks(n); ++b) {
        const int64_t b0 = b * LEADER_BLOCK, nl = n_library + kept;
        const int nb = leader_block_rows(n, b);
        if (nb < 1 || nb > LEADER_BLOCK) return -1;
        // (a) the library walk loads whole 64-column tiles of the pack: inside ld, and every column below nl was appended
        if (nl > 0) {
            const CrossPlan p = cross_plan(nb, nl);
            for (int seg = 0; seg < p.n_seg; ++seg)
                for (int64_t c0 = int64_t(seg) * p.seg_cols; c0 < nl && c0 < int64_t(seg + 1) * p.seg_cols; c0 += 64)
                    for (int lane = 0; lane < 64; ++lane) {
                        Lg[size_t(c0 + lane)] += 0.0;
                        Lc[size_t(pitch - 1) * ld + c0 + lane] += 0.0;
                        if (c0 + lane < nl && !filled[size_t(c0 + lane)]) return -1;
                    }
        }
        // (b) the bits: every (row, word) the replay reads is written exactly once
        std::vector<unsigned char> written(size_t(LEADER_BLOCK) * LEADER_WORDS, 0);
        const LeaderBitsGrid g = leader_bits_grid(nb);
        for (unsigned by = 0; by < g.y; ++by)
            for (unsigned bx = 0; bx < g.x; ++bx)
                for (int wid = 0; wid < LD_WAVES; ++wid) {
                    const int64_t rt = int64_t(bx) * LD_WAVES + wid;
                    const int r0 = int(rt) * LD_ROWS, c0 = int(by) * 64;
                    if (r0 >= nb || c0 > r0) {
                        if (r0 < nb && leader_item_has_pairs(rt, by)) return -1;
                        continue;
                    }
                    if (!leader_item_has_pairs(rt, by)) return -1;
                    for (int t = 0; t < LD_ROWS && r0 + t < nb; ++t) {
                        unsigned char &w = written[size_t(r0 + t) * LEADER_WORDS + by];
                        if (w) return -1;
                        w = 1, bits[size_t(r0 + t) * LEADER_WORDS + by] = 0;
                    }
                }
        for (int s = 0; s < nb; ++s)
            for (int w = 0; w <= s / 64; ++w)
                if (!written[size_t(s) * LEADER_WORDS + w]) return -1;
        // (c) the replay's lists, (d) the append
        int n_acc = 0;
        for (int s = 0; s < nb; ++s)
            if ((b0 + s) % keep_every == 0) {
                acc_pos[size_t(n_acc)] = s;
                kept_src[size_t(kept + n_acc)] = int(b0 + s);
                ++n_acc;
            }
        for (int k = 0; k < n_acc; ++k) {
            const int64_t dst = nl + k;
            if (dst >= capacity || filled[size_t(dst)]) return -1;
            filled[size_t(dst)] = 1;
            for (int d = 0; d < pitch; ++d) Lr[size_t(dst) * pitch + d] = 1.0, Lc[size_t(d) * ld + dst] = 1.0;
            Lg[size_t(dst)] = 1.0;
        }
        kept += n_acc;
    }
    for (int64_t l = 0; l < n_library + kept; ++l)
        if (!filled[size_t(l)]) return -1;
    return kept;
}

static int replays() {
    const int64_t B = LEADER_BLOCK;
    CHECK(replay(1, 0, 12, 1) == 1 && replay(2, 0, 12, 2) == 1 && replay(B - 1, 0, 12, 1) == B - 1 && replay(B, 0, 12, 1) == B);
    CHECK(replay(B + 1, 0, 12, 1) == B + 1 && replay(2 * B + 1, 0, 12, 2) == B + 1 && replay(2 * B + 1, 0, 99, 1) == 2 * B + 1);
    CHECK(replay(B + 1, B + 2, 12, 1000000) == 1 && replay(3 * B + 17, 63, 84, 3) == (3 * B + 17 + 2) / 3 && replay(5, 700, 180, 1) == 5);
    CHECK(replay(70000, 1, 12, 1) == 70000);   // past the threshold where the library walk takes segments of CX_SEG_MAX columns
    return 0;
}

int main() {
    if (sizes() || replays()) return 1;
    printf("leader_plan_check: %d checks passed\n", g_checks);
    return 0;
}
