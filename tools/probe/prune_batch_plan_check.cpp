// prune_batch_plan_check.cpp -- the tables of csrc/prune_batch_plan.hpp (the segments of a many-ensembles RMSD prune with their offsets, every
// refusal of an argument list with its message, the launch order of the one-workgroup route, the work items and the schedule slots of the
// team route) run by a stand-alone program at sizes worked out by hand, so that they can be checked without a GPU and built with
// AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library; tools/prune_batch_plan_check.py builds and runs it.  No HIP
// runtime call is made.  The last part replays the indexing of the team route's kernels (prune_team.hpp) on host arrays standing for a
// segment's three bit arrays, each of exactly ceil(n / 64) words: every word an item or a row's step reads must lie inside them, which is
// what ASan watches.
//
//   prune_batch_plan_check   (exit status 0 and a line "prune_batch_plan_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../tscode_amd/csrc/prune_batch_plan.hpp"

static int g_checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                            \
        }                                                        \
    } while (0)

static const char *BATCH_CAP = "\"prune_batch_max_n\"", *TEAM_CAP = "TSC_PRUNE_TEAM_MAX_N";

// a batch of segments (n[s], h[s]) laid out back to back, threshold 0.5 each
struct Batch {
    std::vector<int32_t> n, h;
    std::vector<int64_t> offsets{0};
    std::vector<double> thr;
    Batch(std::vector<int32_t> n_, std::vector<int32_t> h_) : n(std::move(n_)), h(std::move(h_)), thr(n.size(), 0.5) {
        for (size_t s = 0; s < n.size(); ++s) offsets.push_back(offsets.back() + int64_t(n[s]) * h[s] * 3);
    }
    int plan(PbPlan *p, int mode = 0, int max_n = 2048, const char *name = BATCH_CAP) const {
        return segments("t", offsets.data(), n.data(), h.data(), thr.data(), int64_t(n.size()), mode, max_n, name, p);
    }
};

static bool refused(int rc, const char *message) { return rc == TSC_ERR_INVALID && strcmp(g_err, message) == 0; }

static int segment_tables() {
    // sizes on both sides of the 16-row item and the 64-column word, h = 1 .. 9:
    //   n            0  1  15  16  17  63   64   65  129
    //   words        0  1   1   1   1   1    1    2    3      ceil(n / 64): 11 in all
    //   items        0  1   1   1   2   4    4    5    9      ceil(n / 16): 27 in all
    //   moff         0  0   1  16  32  49  112  176  241      370 structures
    //   woff         0  0   1   2   3   4    5    6    8
    //   doubles      0  6 135 192 255 1134 1344 1560 3483     n h 3: 8109 in all
    const Batch b({0, 1, 15, 16, 17, 63, 64, 65, 129}, {1, 2, 3, 4, 5, 6, 7, 8, 9});
    const long long moff[9] = {0, 0, 1, 16, 32, 49, 112, 176, 241}, woff[9] = {0, 0, 1, 2, 3, 4, 5, 6, 8};
    const long long off[9] = {0, 0, 6, 141, 333, 588, 1722, 3066, 4626};
    const int items[9] = {0, 1, 1, 1, 2, 4, 4, 5, 9};
    PbPlan p;
    CHECK(b.plan(&p) == 0 && p.segs.size() == 9 && p.total_structs == 370 && p.total_words == 11 && p.total_doubles == 8109);
    CHECK(p.items.empty() && p.slots.empty());
    for (int s = 0; s < 9; ++s) {
        const PbSegment &g = p.segs[s];
        CHECK(g.off == off[s] && g.moff == moff[s] && g.woff == woff[s] && g.n == b.n[s] && g.h == b.h[s] && g.seg == s);
        // pass_plan.hpp, thresholds(): thr, 2 thr, h thr^2 / 2, and 2 thr^2 from four heavy atoms on
        CHECK(g.thr == 0.5 && g.maxdev_thr == 1.0 && g.half_h_thr2 == 0.125 * b.h[s] && g.two_thr2 == (b.h[s] >= 4 ? 0.5 : -1.0));
    }
    CHECK(team_tables("t", &p) == 0 && p.items.size() == 27);
    int count[9] = {0};
    for (const int2 &it : p.items) {
        CHECK(it.x >= 0 && it.x < 9 && it.y == count[it.x]);   // (the tiles of one segment keep their order: their weight falls with the tile)
        ++count[it.x];
    }
    for (int s = 0; s < 9; ++s) CHECK(count[s] == items[s] && count[s] <= PT_PER_WORD * ceil_div(b.n[s], 64));
    CHECK(PT_ROWS == 16 && PT_PER_WORD == 4);
    // the heaviest item first: segment 8's first tile has 129 structures behind it, 9 heavy atoms each
    CHECK(p.items[0].x == 8 && p.items[0].y == 0 && p.slots == std::vector<int>({5, 2, 1}));   // 20 x 5 < 129 <= 20 x 10

    // an empty batch: nothing is read, nothing is made; and a batch of empty segments
    PbPlan e;
    CHECK(segments("t", nullptr, nullptr, nullptr, nullptr, 0, 0, 2048, BATCH_CAP, &e) == 0 && team_tables("t", &e) == 0);
    CHECK(e.segs.empty() && e.items.empty() && e.slots.empty() && e.total_structs == 0 && e.total_doubles == 0 && e.total_words == 0);
    PbPlan z;
    CHECK(Batch({0, 0}, {3, 3}).plan(&z) == 0 && team_tables("t", &z) == 0 && z.segs.size() == 2 && z.items.empty() && z.slots.empty() && z.total_words == 0);
    return 0;
}

static int refusals() {
    PbPlan p;
    char want[256];
    // one past each cap, the cap named as the route names it
    CHECK(Batch({2048}, {3}).plan(&p) == 0);
    CHECK(refused(Batch({5, 2049}, {3, 3}).plan(&p), "t: segment 1 has 2049 structures, more than \"prune_batch_max_n\" = 2048"));
    CHECK(Batch({TSC_PRUNE_TEAM_MAX_N}, {1}).plan(&p, 0, TSC_PRUNE_TEAM_MAX_N, TEAM_CAP) == 0);
    snprintf(want, sizeof(want), "t: segment 0 has %d structures, more than TSC_PRUNE_TEAM_MAX_N = %d", TSC_PRUNE_TEAM_MAX_N + 1, TSC_PRUNE_TEAM_MAX_N);
    CHECK(refused(Batch({TSC_PRUNE_TEAM_MAX_N + 1}, {1}).plan(&p, 0, TSC_PRUNE_TEAM_MAX_N, TEAM_CAP), want));
    CHECK(refused(Batch({4, 4}, {3, 0}).plan(&p), "t: segment 1 has 0 heavy atoms (at least 1)"));
    CHECK(refused(Batch({-1}, {3}).plan(&p), "t: segment 0 has -1 structures"));
    Batch span({2, 4}, {3, 3});   // 18 and 36 doubles
    span.offsets[1] = 10;
    CHECK(refused(span.plan(&p), "t: offsets[0] .. offsets[1] span 10 doubles, segment is 2 x 3 x 3"));
    span.offsets[1] = 18, span.offsets[2] = 55;
    CHECK(refused(span.plan(&p), "t: offsets[1] .. offsets[2] span 37 doubles, segment is 4 x 3 x 3"));
    Batch shifted({2}, {3});
    shifted.offsets[0] = 5, shifted.offsets[1] = 23;
    CHECK(refused(shifted.plan(&p), "t: offsets[0] = 5, not 0"));
    Batch nan({2, 2}, {3, 3}), inf({2}, {3});
    nan.thr[1] = std::numeric_limits<double>::quiet_NaN(), inf.thr[0] = std::numeric_limits<double>::infinity();
    CHECK(refused(nan.plan(&p), "t: thr[1] is not finite") && refused(inf.plan(&p), "t: thr[0] is not finite"));
    const Batch ok({2}, {3});
    CHECK(ok.plan(&p, 1) == 0 && refused(ok.plan(&p, 2), "t: mode 2 (0 = reference-exact, 1 = cache-free)") && refused(ok.plan(&p, -1), "t: mode -1 (0 = reference-exact, 1 = cache-free)"));
    // null tables, each of the four; none is needed for no segments (segment_tables), where the mode is still checked
    CHECK(refused(segments("t", nullptr, ok.n.data(), ok.h.data(), ok.thr.data(), 1, 0, 2048, BATCH_CAP, &p), "t: null argument"));
    CHECK(refused(segments("t", ok.offsets.data(), nullptr, ok.h.data(), ok.thr.data(), 1, 0, 2048, BATCH_CAP, &p), "t: null argument"));
    CHECK(refused(segments("t", ok.offsets.data(), ok.n.data(), nullptr, ok.thr.data(), 1, 0, 2048, BATCH_CAP, &p), "t: null argument"));
    CHECK(refused(segments("t", ok.offsets.data(), ok.n.data(), ok.h.data(), nullptr, 1, 0, 2048, BATCH_CAP, &p), "t: null argument"));
    CHECK(refused(segments("t", nullptr, nullptr, nullptr, nullptr, 0, 2, 2048, BATCH_CAP, &p), "t: mode 2 (0 = reference-exact, 1 = cache-free)"));
    // the segment count: every segment has TSC_MAX_PASSES = 18 statistics records, indexed by int: 2^31 - 1 = 18 x 119 304 647 + 1
    CHECK(refused(segments("t", nullptr, nullptr, nullptr, nullptr, -1, 0, 2048, BATCH_CAP, &p), "t: -1 segments"));
    CHECK(refused(segments("t", nullptr, nullptr, nullptr, nullptr, 119304648, 0, 2048, BATCH_CAP, &p), "t: 119304648 segments"));
    CHECK(refused(segments("t", nullptr, nullptr, nullptr, nullptr, 119304647, 0, 2048, BATCH_CAP, &p), "t: null argument"));
    // the item count is a grid size: four items per word, 200 000 structures are 3125 words, 171 799 such segments 536 871 875 words and
    // 2 147 487 500 items, 3853 more than 2^31 - 1 (one segment fewer fits: 2 147 475 000)
    static_assert(TSC_PRUNE_TEAM_MAX_N == 200000, "the sizes below are worked out for this cap");
    PbPlan big;
    CHECK(Batch(std::vector<int32_t>(171799, 200000), std::vector<int32_t>(171799, 1)).plan(&big, 0, TSC_PRUNE_TEAM_MAX_N, TEAM_CAP) == 0);
    CHECK(big.total_words == 536871875LL && big.total_structs == 34359800000LL && big.segs.back().woff == 536868750LL);
    CHECK(refused(team_tables("t", &big), "t: 2147487500 work items in all") && big.items.empty());
    return 0;
}

static std::vector<int> slots_of(int n_max) {
    PbPlan p;
    if (Batch({3, n_max, 7}, {2, 2, 2}).plan(&p, 0, 8192) != 0 || team_tables("t", &p) != 0) return {-1};
    return p.slots;
}

static int schedule() {
    // :186-188 and the gate of :192 with nothing removed yet: k == 1, or 20 k < the longest segment
    CHECK(sizeof(KS) / sizeof(KS[0]) == 18 && KS[0] == 500000 && KS[1] == 200000 && KS[11] == 100 && KS[15] == 5 && KS[16] == 2 && KS[17] == 1);
    for (int s = 0; s + 1 < 18; ++s) CHECK(KS[s] > KS[s + 1]);
    CHECK(pass_gate(1, 0) && pass_gate(1, 1) && !pass_gate(2, 40) && pass_gate(2, 41) && !pass_gate(500000, 10000000) && pass_gate(500000, 10000001));
    CHECK(pass_gate(500000, 1LL << 40));   // (64-bit arithmetic: 20 x 500 000 fits an int, the count of a single-ensemble run need not)
    CHECK(slots_of(20) == std::vector<int>({1}) && slots_of(21) == std::vector<int>({1}));
    CHECK(slots_of(40) == std::vector<int>({1}) && slots_of(41) == std::vector<int>({2, 1}));
    CHECK(slots_of(2100) == std::vector<int>({100, 50, 20, 10, 5, 2, 1}) && slots_of(2101) == std::vector<int>({100, 50, 20, 10, 5, 2, 1}));
    CHECK(slots_of(2000) == std::vector<int>({50, 20, 10, 5, 2, 1}) && slots_of(2001) == std::vector<int>({100, 50, 20, 10, 5, 2, 1}));
    // the chunk of a row: 1003 structures in 10 chunks of 100, the last one 103 long (:141-144)
    int f = -1, l = -1;
    CHECK(chunk_of_row(0, 1003, 10, 100, f, l) == 0 && f == 0 && l == 100);
    CHECK(chunk_of_row(99, 1003, 10, 100, f, l) == 0 && f == 0 && l == 100);
    CHECK(chunk_of_row(100, 1003, 10, 100, f, l) == 1 && f == 100 && l == 200);
    CHECK(chunk_of_row(899, 1003, 10, 100, f, l) == 8 && f == 800 && l == 900);
    CHECK(chunk_of_row(900, 1003, 10, 100, f, l) == 9 && f == 900 && l == 1003);
    CHECK(chunk_of_row(1002, 1003, 10, 100, f, l) == 9 && f == 900 && l == 1003);   // (1002 / 100 = 10: still the last chunk)
    CHECK(chunk_of_row(7, 8, 1, 8, f, l) == 0 && f == 0 && l == 8);
    return 0;
}

static int orders() {
    //            n   h   n^2 h   items: (n - 16 t) h
    //   A  (0)  32   2   2048    64 32
    //   B  (1)  16   8   2048    128
    //   C  (2)  64   1   4096    64 48 32 16
    const Batch b({32, 16, 64}, {2, 8, 1});
    PbPlan p;
    CHECK(b.plan(&p) == 0 && team_tables("t", &p) == 0);
    // the team route: the segments stay in the caller's order; B's tile, then the two of 64 (A before C: the caller's order), 48, the two of 32, 16
    const int want[7][2] = {{1, 0}, {0, 0}, {2, 0}, {2, 1}, {0, 1}, {2, 2}, {2, 3}};
    CHECK(p.items.size() == 7 && p.segs[0].seg == 0 && p.segs[1].seg == 1 && p.segs[2].seg == 2);
    for (int q = 0; q < 7; ++q) CHECK(p.items[q].x == want[q][0] && p.items[q].y == want[q][1]);
    // the one-workgroup route: C first, then the tie in the caller's order; a segment keeps its offsets and its index
    launch_order(&p);
    CHECK(p.segs[0].seg == 2 && p.segs[1].seg == 0 && p.segs[2].seg == 1);
    CHECK(p.segs[0].moff == 48 && p.segs[0].off == 576 && p.segs[0].n == 64 && p.segs[1].moff == 0 && p.segs[1].off == 0 && p.segs[2].moff == 32 && p.segs[2].off == 192);
    return 0;
}

// The indexing of k_team_prologue, k_team_rows and k_team_finish on one plan: per segment three arrays of exactly ceil(n / 64) words (what
// `st.in + woff` and its like point at: the next segment's words begin right behind).  Every structure active, every slot the segment's N
// opens: the walks at their longest.  Returns the pt_bits reads made, -1 where a step did not see the columns it has.
static long long replay(const PbPlan &p) {
    long long reads = 0;
    std::vector<std::vector<unsigned long long>> in(p.segs.size()), view(p.segs.size());
    for (size_t s = 0; s < p.segs.size(); ++s) {
        const int nw = ceil_div(p.segs[s].n, 64);
        if (s + 1 < p.segs.size() && p.segs[s + 1].woff - p.segs[s].woff != nw) return -1;
        in[s].assign(size_t(nw), ~0ull), view[s].assign(size_t(nw), 0ull);
    }
    for (const int2 &it : p.items) {
        const PbSegment &g = p.segs[size_t(it.x)];
        const int N = g.n, r0 = it.y * PT_ROWS;
        unsigned long long *bits = in[size_t(it.x)].data();
        if (r0 >= N) return -1;
        if (it.y % PT_PER_WORD == 0) {   // k_team_prologue: the first item of a word writes it
            const int rem = N - r0;
            bits[it.y / PT_PER_WORD] = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
        }
    }
    for (const int2 &it : p.items) {
        const PbSegment &g = p.segs[size_t(it.x)];
        const int N = g.n, nw = ceil_div(N, 64), r0 = it.y * PT_ROWS;
        const unsigned long long *bits = in[size_t(it.x)].data(), *vw = view[size_t(it.x)].data();
        const unsigned rows = unsigned(bits[r0 >> 6] >> (r0 & 63)) & ((1u << PT_ROWS) - 1u);   // k_team_rows: the item's rows
        if (rows != (N - r0 >= PT_ROWS ? (1u << PT_ROWS) - 1u : (1u << (N - r0)) - 1u)) return -1;
        for (int k : p.slots) {
            if (!pass_gate(k, N)) continue;
            const int cs = N / k;
            for (int i = r0; i < r0 + PT_ROWS; ++i) {
                if (!((rows >> (i - r0)) & 1u)) continue;
                int f, l;
                chunk_of_row(i, N, k, cs, f, l);
                for (int j0 = i + 1; j0 < l; j0 += 64) {
                    const int left = l - j0;
                    unsigned long long vm = pt_bits(bits, nw, j0);
                    if (left < 64) vm &= (1ull << left) - 1ull;
                    if (vm != (left < 64 ? (1ull << left) - 1ull : ~0ull)) return -1;
                    if (pt_bits(vw, nw, f + (j0 - i)) != 0ull) return -1;
                    reads += 2;
                }
            }
        }
        for (int t = r0; t < r0 + PT_ROWS && t < N; ++t)   // k_team_finish
            if (!((bits[t >> 6] >> (t & 63)) & 1ull)) return -1;
    }
    return reads;
}

static int replays() {
    PbPlan p;
    // the sizes of segment_tables, and the shapes with several slots: 1003 structures (a remainder chunk), 2100 (seven slots)
    CHECK(Batch({0, 1, 15, 16, 17, 63, 64, 65, 129}, {1, 2, 3, 4, 5, 6, 7, 8, 9}).plan(&p) == 0 && team_tables("t", &p) == 0);
    // one slot per segment (k = 1) but for 65 (k = 2, 1: rows 0 .. 31 have 31 .. 0 columns, rows 32 .. 64 have 32 .. 0; then 64 .. 0) and 129:
    // a row with c columns takes ceil(c / 64) steps of two reads
    CHECK(replay(p) > 0);
    PbPlan q;
    CHECK(Batch({1003, 0, 2100, 64}, {3, 3, 2, 5}).plan(&q, 0, 8192) == 0 && team_tables("t", &q) == 0 && q.slots.size() == 7);
    CHECK(replay(q) > 0);
    // two structures, one slot: row 0 has one column, one step, two reads; row 1 none
    PbPlan two;
    CHECK(Batch({2}, {3}).plan(&two) == 0 && team_tables("t", &two) == 0 && replay(two) == 2);
    // 65 structures alone: k = 2 (chunks [0, 32) and [32, 65)) and k = 1.  k = 2: rows with 1 .. 31 and 1 .. 32 columns, one step each, 63
    // steps; k = 1: rows 0 .. 63 have 64 .. 1 columns, one step each, 64 steps.  127 steps, 254 reads.
    PbPlan s65;
    CHECK(Batch({65}, {3}).plan(&s65) == 0 && team_tables("t", &s65) == 0 && s65.slots == std::vector<int>({2, 1}) && replay(s65) == 254);
    // 130 structures alone, k = 5, 2, 1.  k = 1: row i has 129 - i columns: row 0 has 129 (3 steps), rows 1 .. 64 have 128 .. 65 (2 steps), rows
    // 65 .. 128 one: 3 + 128 + 64 = 195.  k = 2, chunks of 65: 64 rows of one step each, twice: 128.  k = 5, chunks of 26: 25 x 5 = 125.
    PbPlan s130;
    CHECK(Batch({130}, {3}).plan(&s130) == 0 && team_tables("t", &s130) == 0 && s130.slots == std::vector<int>({5, 2, 1}) && replay(s130) == 2 * (195 + 128 + 125));
    return 0;
}

int main() {
    if (segment_tables() || refusals() || schedule() || orders() || replays()) return 1;
    printf("prune_batch_plan_check: %d checks passed\n", g_checks);
    return 0;
}
