// pass_cursor_check.cpp -- the host's bookkeeping of a stepped prune run (csrc/pass_cursor.hpp: PassCursor, the run's layout numbers) driven
// by a stand-alone program through every call order, so that the hand-over rule -- which kernel closes a pass on the device and opens the
// next -- can be checked without a GPU and built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library;
// tools/pass_cursor_check.py builds and runs it.  No HIP runtime call is made.  The device is a small model: per schedule slot, how often
// its state block was opened and how often its record was closed, bumped as the cursor's transitions say a kernel would (csrc/prune.hip
// makes the same calls, with the launches beside them).
//
//   pass_cursor_check        (exit status 0 and a line "pass_cursor_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tscode_amd/csrc/pass_cursor.hpp"

using namespace tsc;

static long long g_checks = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        ++g_checks;                                                    \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)
#define TRY(call)              \
    do {                       \
        if ((call) != 0) {     \
            fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); \
            return 1;          \
        }                      \
    } while (0)

// ---- the layout numbers, against values worked out by hand ----
static int layout() {
    // a bit copy of the mask, n / 64 + 40 words:  1 / 64 = 0 -> 40;  63 / 64 = 0 -> 40;  64 / 64 = 1 -> 41;  65 535 / 64 = 1 023 -> 1 063;
    // 65 536 / 64 = 1 024 -> 1 064;  57 046 / 64 = 891 (891 x 64 = 57 024) -> 931
    CHECK(bit_words_of(1) == 40 && bit_words_of(63) == 40 && bit_words_of(64) == 41);
    CHECK(bit_words_of(65535) == 1063 && bit_words_of(65536) == 1064 && bit_words_of(57046) == 931);
    // its summary, bit_words / 1024 + 4:  40, 41 and 931 are below 1 024 -> 4;  1 063 / 1 024 = 1 and 1 064 / 1 024 = 1 -> 5
    CHECK(dsum_words_of(40) == 4 && dsum_words_of(41) == 4 && dsum_words_of(931) == 4 && dsum_words_of(1063) == 5 && dsum_words_of(1064) == 5);
    // a view with its summary:  40 + 4 = 44;  41 + 4 = 45;  931 + 4 = 935;  1 063 + 5 = 1 068;  1 064 + 5 = 1 069
    CHECK(view_stride(40) == 44 && view_stride(41) == 45 && view_stride(931) == 935 && view_stride(1063) == 1068 && view_stride(1064) == 1069);
    // views, one per pass with k = 1 or 20 k < n:  n = 1: k = 1 alone;  n = 63 and 64: k = 2 (40 < 63) and 1, not 5 (100);  n = 65 535, 65 536
    // and 57 046: 20 x 2 000 = 40 000 is below all three, 20 x 5 000 = 100 000 is not: k = 2 000, 1 000, 500, 200, 100, 50, 20, 10, 5, 2, 1 -> 11
    CHECK(n_views_of(1, 0) == 1 && n_views_of(63, 0) == 2 && n_views_of(64, 0) == 2);
    CHECK(n_views_of(65535, 0) == 11 && n_views_of(65536, 0) == 11 && n_views_of(57046, 0) == 11);
    // the exchange buffer, bits + 8 + views:  n = 1: 40 + 8 + 1 x 44 = 92;  n = 57 046: 931 + 8 + 11 x 935 = 939 + 10 285 = 11 224;
    // n = 65 536: 1 064 + 8 + 11 x 1 069 = 1 072 + 11 759 = 12 831;  cache-free: no views, 48 / 939 / 1 072
    CHECK(exchange_words_of(1, 0) == 92 && exchange_words_of(57046, 0) == 11224 && exchange_words_of(65536, 0) == 12831);
    CHECK(exchange_words_of(1, 1) == 48 && exchange_words_of(57046, 1) == 939 && exchange_words_of(65536, 1) == 1072);
    for (long long n : {1ll, 20ll, 21ll, 63ll, 64ll, 450ll, 57046ll, 65535ll, 65536ll, 10000001ll}) {
        CHECK(n_views_of(n, 1) == 0 && views_words_of(n, 1) == 0);
        CHECK(views_words_of(n, 0) == (long long)n_views_of(n, 0) * (long long)view_stride(bit_words_of(n)));
    }
    return 0;
}

// ---- the model of the device ----
struct Device {
    int opened[TSC_MAX_PASSES] = {0}, closed[TSC_MAX_PASSES] = {0};
};

static std::vector<int> runnable(long long n) {
    std::vector<int> slots;
    for (int s = 0; s < TSC_MAX_PASSES; ++s)
        if (pass_can_run(n, s)) slots.push_back(s);
    return slots;
}

// a kernel opens slot `s`; closing: the slot the same kernel closes, -1 for none.  The runnable slot in front of `s` must be closed by then
static int dev_open(Device &d, long long n, int s, int closing) {
    if (s < 0) return 0;
    CHECK(pass_can_run(n, s) && d.opened[s] == 0 && d.closed[s] == 0);
    int before = -1;
    for (int q = 0; q < s; ++q)
        if (pass_can_run(n, q)) before = q;
    CHECK(before < 0 || d.closed[before] == 1 || before == closing);
    ++d.opened[s];
    return 0;
}
static int dev_close(Device &d, int s) {
    CHECK(s >= 0 && d.opened[s] == 1 && d.closed[s] == 0);   // once, and no earlier than it was opened
    ++d.closed[s];
    return 0;
}
// one launch closes h.prev and opens h.next
static int dev_hand_over(Device &d, long long n, const Handover &h) {
    TRY(dev_open(d, n, h.next, h.prev));
    TRY(dev_close(d, h.prev));
    return 0;
}

static bool same(const PassCursor &a, const PassCursor &b) {
    return a.n == b.n && a.scan_from == b.scan_from && a.slot == b.slot && a.k == b.k && memcmp(a.ran, b.ran, sizeof(a.ran)) == 0 && a.exported == b.exported &&
           a.phase == b.phase && a.kind == b.kind && a.range == b.range && a.opened == b.opened && a.left == b.left && a.left_local == b.left_local &&
           a.closes == b.closes && a.closes_local == b.closes_local && a.rows_known_for == b.rows_known_for && a.split == b.split;
}

// ---- the call order: every entry point's message, where it is refused and where it is not ----
static const StepCall ALL_CALLS[] = {StepCall::NextPass,    StepCall::Estimate, StepCall::PassLocal, StepCall::Partitioned,   StepCall::PassRange,
                                     StepCall::PassMerge,   StepCall::ViewsPtr, StepCall::ViewsMerged, StepCall::PassRows,    StepCall::BestPtr,
                                     StepCall::UseBestBuffer, StepCall::SetPartition, StepCall::PassFinish, StepCall::Stats};

// what the library answers today (csrc/prune.hip before the cursor), from the state the cursor is in: null = the call goes through
static const char *todays_message(const PassCursor &c, StepCall call) {
    const bool idle = c.phase == PassPhase::Idle, open = c.phase == PassPhase::Open, launched = c.phase == PassPhase::Launched;
    switch (call) {
        case StepCall::NextPass: return idle ? nullptr : "tsc_prune_next_pass: previous pass not finished";                       // next while open
        case StepCall::Estimate: return idle ? "tsc_prune_pass_estimate: no pass open" : nullptr;
        case StepCall::PassLocal: return open ? nullptr : "tsc_prune_pass_local: no pass open (call tsc_prune_next_pass)";       // launch while idle, launch twice
        case StepCall::Partitioned: return idle ? "tsc_prune_pass_partitioned: no pass open" : nullptr;
        case StepCall::PassRange: return open ? nullptr : "tsc_prune_pass_range: no pass open (call tsc_prune_next_pass)";
        case StepCall::PassMerge: return launched && c.range ? nullptr : "tsc_prune_pass_merge: tsc_prune_pass_range has not run";  // merge without range
        case StepCall::ViewsPtr: return idle ? "tsc_prune_views_ptr: no pass open" : nullptr;
        case StepCall::ViewsMerged: return idle ? "tsc_prune_views_merged: no pass open" : nullptr;
        case StepCall::PassRows:                                                                                                   // rows on a local or fused pass
            return launched && c.kind == PassKind::Behind ? nullptr : "tsc_prune_pass_rows: needs an open pass whose tsc_prune_pass_local ran with world_size > 1";
        case StepCall::BestPtr: return idle ? "tsc_prune_best_ptr: no pass open" : nullptr;
        case StepCall::UseBestBuffer: return idle && c.scan_from == 0 ? nullptr : "tsc_prune_use_best_buffer: call it right after tsc_prune_create";
        case StepCall::SetPartition: return idle && c.scan_from == 0 ? nullptr : "tsc_prune_set_partition: call it right after tsc_prune_create";
        case StepCall::PassFinish:                                                                                                 // finish before launch, on a range pass
            if (!launched) return "tsc_prune_pass_finish: tsc_prune_pass_local has not run";
            return c.range ? "tsc_prune_pass_finish: a rank-partitioned pass is closed by tsc_prune_pass_merge" : nullptr;
        case StepCall::Stats: return idle ? nullptr : "tsc_prune_stats: a pass is still open";                                    // stats while open
    }
    return nullptr;
}

// every call made now: the message of today, or none; a refused call leaves the cursor as it was.  n_refused: how many are refused here
static int call_order(const PassCursor &c, int n_refused) {
    const PassCursor before = c;
    int refused = 0;
    for (StepCall call : ALL_CALLS) {
        const char *want = todays_message(c, call), *got = c.refusal(call);
        CHECK((want == nullptr) == (got == nullptr));
        CHECK(!want || strcmp(want, got) == 0);
        refused += got ? 1 : 0;
    }
    CHECK(refused == n_refused && same(before, c));
    return 0;
}

// ---- one run ----
struct Step {
    PassKind kind;
    bool range;   // tsc_prune_pass_range / _merge where the pass is partitioned
};
constexpr int PART_MIN_K = 10;   // the probe's partition: passes of at least this many chunks (tsc_prune_set_partition: min_chunks x world)
static bool partitioned(int slot) { return slot >= 0 && KS[slot] >= PART_MIN_K; }

// small_blocks: the prefix of the scan blocks fits k_open_rows' LDS array, so the first kernel of a walked pass can derive as well;
// stats_between: tsc_prune_stats after every pass (the export closes what was left open, the run goes on)
static int run(long long n, const std::vector<Step> &steps, bool small_blocks, bool stats_between) {
    const std::vector<int> slots = runnable(n);
    CHECK(steps.size() == slots.size());
    PassCursor c;
    Device d;
    c.start(n);
    CHECK(c.opened == (slots.empty() ? -1 : slots[0]) && c.fresh());
    TRY(dev_open(d, n, c.opened, -1));   // (k_init_run)
    TRY(call_order(c, 10));              // idle, fresh: all but next, use-best-buffer, set-partition and stats
    bool merged_before = false;
    for (size_t i = 0; i < slots.size(); ++i) {
        const int s = c.next_slot();
        CHECK(s == slots[i] && c.refusal(StepCall::NextPass) == nullptr);
        c.begin(s);
        CHECK(c.phase == PassPhase::Open && c.slot == s && c.k == KS[s] && !c.fresh());
        TRY(call_order(c, 7));   // open: next, merge, rows, use-best-buffer, set-partition, finish, stats
        CHECK(c.rows_ready() == (merged_before && partitioned(s)));
        // pass_launch
        const Step st{steps[i].kind, steps[i].range && partitioned(s)};
        const bool can_derive = !st.range && (st.kind == PassKind::Local || small_blocks);
        const int left_before = c.left;
        const Handover h = c.open_slot(st.range, can_derive);
        CHECK(h.how != Opener::Nothing);   // exactly one of the four outcomes; the error never in a legal sequence
        if (h.how == Opener::Opened) {
            CHECK(d.opened[s] == 1 && d.closed[s] == 0 && h.prev == -1 && left_before == -1 && c.closes == -1);
        } else {
            CHECK(h.prev == left_before && h.prev >= 0 && h.next == s && (h.how == Opener::Derives) == can_derive);
            CHECK(c.closes == (can_derive ? h.prev : -1));   // (what derive_args hands the first kernel)
            TRY(dev_hand_over(d, n, h));
        }
        CHECK(c.opened == s && c.left == -1 && c.range == st.range && c.phase == PassPhase::Open);
        c.launched(st.kind);
        CHECK(c.phase == PassPhase::Launched && c.ran[s]);
        CHECK(c.left == ((st.range || st.kind == PassKind::Behind) ? -1 : s) && (c.left < 0 || c.left_local == (st.kind == PassKind::Local)));
        // launched: next, local, range, use-best-buffer, set-partition, stats; merge or finish; rows unless applied behind
        TRY(call_order(c, 7 + (st.kind == PassKind::Behind ? 0 : 1)));
        if (st.range) {   // tsc_prune_pass_range has run: the views are this rank's alone until they are merged
            c.split_views();
            CHECK(c.refusal(StepCall::PassMerge) == nullptr && c.refusal(StepCall::PassFinish) != nullptr);
            const int nxt = c.next_slot();
            if (partitioned(nxt)) c.range_ready(nxt);
            TRY(dev_close(d, s));   // (k_pass_merge)
            c.closed_on_device();
            CHECK(c.opened == nxt);
            TRY(dev_open(d, n, c.opened, s));
        } else {
            CHECK(c.refusal(StepCall::PassFinish) == nullptr && c.refusal(StepCall::PassMerge) != nullptr);
            if (st.kind == PassKind::Behind) {   // (k_apply_pass)
                TRY(dev_close(d, s));
                c.closed_on_device();
                TRY(dev_open(d, n, c.opened, s));
            }
        }
        c.end_pass();
        merged_before = st.range;
        if (merged_before && !partitioned(c.next_slot())) c.merged_views();   // (tsc_prune_views_merged in front of the first pass of the other kind)
        CHECK(c.phase == PassPhase::Idle && c.slot == -1 && c.k == 0 && !c.exported && !c.range);
        TRY(call_order(c, 12));   // idle between passes: all but next and stats
        if (stats_between) {
            const Handover e = c.close_for_export();
            CHECK((e.how == Opener::Step) == (!st.range && st.kind != PassKind::Behind) && e.next == (e.how == Opener::Step ? c.next_slot() : -1));
            if (e.how == Opener::Step) TRY(dev_hand_over(d, n, e));
            c.exported = true;
            CHECK(c.left == -1 && c.close_for_export().how == Opener::Opened);   // (a second export has nothing to close)
        }
    }
    // the schedule is exhausted; the end-of-run close
    CHECK(c.next_slot() == -1);
    c.begin(-1);
    CHECK(c.phase == PassPhase::Idle && c.scan_from == TSC_MAX_PASSES && c.next_slot() == -1);
    const Handover e = c.close_for_export();
    CHECK(e.next == -1);
    if (e.how == Opener::Step) TRY(dev_hand_over(d, n, e));
    c.exported = true;
    CHECK(c.left == -1 && c.opened == -1);   // nothing is left open
    for (int s = 0; s < TSC_MAX_PASSES; ++s) {
        const int once = pass_can_run(n, s) ? 1 : 0;
        CHECK(d.opened[s] == once && d.closed[s] == once && c.ran[s] == (once == 1));
    }
    TRY(call_order(c, 12));
    return 0;
}

// every sequence of pass kinds over the runnable slots (at most five of them), partitioned or not, the first kernel able to derive or not,
// statistics read between the passes or not
static int exhaustive(long long n, size_t n_slots) {
    const std::vector<int> slots = runnable(n);
    CHECK(slots.size() == n_slots && n_slots <= 5);
    size_t combos = 1;
    for (size_t i = 0; i < n_slots; ++i) combos *= 3;
    for (size_t code = 0; code < combos; ++code)
        for (int flags = 0; flags < 8; ++flags) {
            std::vector<Step> steps;
            size_t rest = code;
            for (size_t i = 0; i < n_slots; ++i, rest /= 3) steps.push_back(Step{PassKind(rest % 3), (flags & 1) != 0});
            TRY(run(n, steps, (flags & 2) != 0, (flags & 4) != 0));
        }
    return 0;
}

// l / f / b: a chunk-local pass, a walked pass that applies its own rows, a pass applied behind its pair kernels; a capital: on this rank's
// chunks where the pass is partitioned.  One letter per runnable slot, from the first; a shorter schedule takes the front of the line
static const char *const MIXED[] = {
    "llllllllllllllllll", "ffffffffffffffffff", "bbbbbbbbbbbbbbbbbb", "LLLLLLLLLLLLLLLLLL", "FFFFFFFFFFFFFFFFFF", "BBBBBBBBBBBBBBBBBB",
    "lfblfblfblfblfblfb", "bflbflbflbflbflbfl", "LFBlfbLFBlfbLFBlfb", "lLfFbBlLfFbBlLfFbB", "FFFFFFFFlllllbbbff", "BBBBLLLLffffllllbf",
    "llllllllfffffffbbb", "fbfbfbfbfbfLLLLLLl", "LlLlLlLlLlLlLlLlLl", "bbbbbbbbbbbbbbbbbl", "lbbbbbbbbbbbbbbbbb", "FbFbFbFbFlFlFlFlFf",
};

static int mixed(long long n, size_t n_slots) {
    CHECK(runnable(n).size() == n_slots);
    for (const char *line : MIXED) {
        CHECK(strlen(line) == size_t(TSC_MAX_PASSES));
        std::vector<Step> steps;
        for (size_t i = 0; i < n_slots; ++i) {
            const char ch = line[i], low = char(ch | 0x20);
            steps.push_back(Step{low == 'l' ? PassKind::Local : low == 'f' ? PassKind::Fused : PassKind::Behind, ch != low});
        }
        for (int flags = 0; flags < 4; ++flags) TRY(run(n, steps, (flags & 1) != 0, (flags & 2) != 0));
    }
    return 0;
}

// a pass whose slot nobody has opened and in front of which nothing was left open: the error outcome, and the cursor stays as it was
static int nothing_to_open_from() {
    PassCursor c;
    c.start(450);
    c.begin(c.next_slot());
    c.opened = -1;   // (cannot come about through the transitions)
    const PassCursor before = c;
    CHECK(c.open_slot(false, true).how == Opener::Nothing && same(before, c));
    CHECK(c.open_slot(true, false).how == Opener::Nothing && same(before, c));
    return 0;
}

int main() {
    if (layout()) return 1;
    // n = 20 and n = 21: k = 1 alone (pass_gate lets k = 1 through at any size; 20 x 2 = 40 is not below either); n = 450: k = 20, 10, 5, 2, 1
    if (exhaustive(1, 1) || exhaustive(20, 1) || exhaustive(21, 1) || exhaustive(41, 2) || exhaustive(450, 5)) return 1;
    // n = 57 046: k = 2 000 ... 1; n = 10 000 001: every slot of KS (20 x 500 000 is just below it)
    if (mixed(450, 5) || mixed(57046, 11) || mixed(10000001, TSC_MAX_PASSES)) return 1;
    if (nothing_to_open_from()) return 1;
    printf("pass_cursor_check: %lld checks passed\n", g_checks);
    return 0;
}
