// pass_cursor.hpp -- the host's bookkeeping of one prune run as it is stepped (tsc_prune_next_pass ... tsc_prune_stats): where the run is in the
// schedule, what has been launched of the open pass, and which kernel closes a pass on the device and opens the next one (pass_state.hpp:
// pass_derive, pass_step_wave).  And the run's layout numbers.  Plain functions and one plain struct: no kernel, no HIP call, so that
// tools/probe/pass_cursor_check.cpp drives every call order through it on the CPU.
//
// The hand-over rule.  A slot's state block is written ("opened") by exactly one kernel and its record finished ("closed") by exactly one:
//   - the first runnable slot is opened by the run's first kernel (start);
//   - a pass applied behind its pair kernels (culled, dealt by tiles) and a rank-partitioned pass are closed by their last kernel -- the one that
//     applies the rows, the merge --, which opens the next runnable slot in the same round trip (closed_on_device);
//   - a chunk-local pass and a walked pass whose pair kernel applies its own rows end without a closing wavefront: they are LEFT OPEN (launched),
//     and whoever needs the next slot first closes them behind a kernel boundary -- the first kernel of the next pass where it can
//     (Opener::Derives), a one-block step launch where it cannot (Opener::Step), or the step launch in front of the export (close_for_export).
#pragma once

#include <cstddef>
#include <cstdint>

#include "prune_schedule.hpp"

namespace tsc {

// ---- the layout numbers of a run over n structures (64-bit words) ----
// a bit copy of the mask: k_open_rows reads the 32 words of a whole scan block, also of the last, partial one
static inline size_t bit_words_of(int64_t n) { return size_t(n / 64 + 40); }
// one summary bit per 1024 cache-view bits, kept right behind the view
static inline size_t dsum_words_of(size_t bit_words) { return bit_words / 1024 + 4; }
static inline size_t view_stride(size_t bit_words) { return bit_words + dsum_words_of(bit_words); }
constexpr int EXCH_STAT_WORDS = 8;   // the statistics of a rank-partitioned pass, behind the removed-row bits of the exchange buffer

// Can the pass of schedule slot `slot` (KS) ever run on n structures?  count_nonzero(mask) <= n, so a pass with 20 k >= n can never pass the
// gate of :192; the others are enqueued and gated on the device.
static inline bool pass_can_run(int64_t n, int slot) { return pass_gate(KS[slot], n); }
// cache views: one per pass that can run, none in cache-free mode
static inline int n_views_of(int64_t n, int mode) {
    int v = 0;
    for (int slot = 0; slot < TSC_MAX_PASSES; ++slot) v += (mode == 0 && pass_can_run(n, slot)) ? 1 : 0;
    return v;
}
static inline int64_t views_words_of(int64_t n, int mode) { return int64_t(n_views_of(n, mode)) * int64_t(view_stride(bit_words_of(n))); }
// the exchange buffer: the removed-row bits of a pass, its statistics, then -- reference-exact mode -- the storage of every cache view (so
// that the host can sum the views of the remaining passes over the ranks in place, as part of a buffer it owns)
static inline int64_t exchange_words_of(int64_t n, int mode) { return int64_t(bit_words_of(n)) + EXCH_STAT_WORDS + views_words_of(n, mode); }

// ---- the cursor ----
enum class PassPhase { Idle, Open, Launched };   // no pass open; handed out by next_pass; its kernels enqueued
// how the rows of the launched pass are applied: by the chunk-local kernel, by the walked pair kernel itself, or by a kernel behind the pair
// kernels (a culled pass, a pass dealt to ranks by row tiles)
enum class PassKind { Local, Fused, Behind };
enum class Opener { Opened, Derives, Step, Nothing };   // open_slot: already opened; the first kernel derives; launch k_pass_step; error
struct Handover {
    Opener how;
    int prev;          // the slot to close (Derives, Step), -1 otherwise
    bool prev_local;   // ... ran in the chunk-local kernel (its record says so)
    int next;          // the slot opened with it, -1 for none
};
enum class StepCall { NextPass, Estimate, PassLocal, Partitioned, PassRange, PassMerge, ViewsPtr, ViewsMerged, PassRows, BestPtr, UseBestBuffer, SetPartition, PassFinish, Stats };

struct PassCursor {
    int64_t n = 0;
    // the walk through the schedule
    int scan_from = 0;   // next index into KS to consider
    int slot = -1;       // the open pass (-1 = none) and its k
    int64_t k = 0;
    bool ran[TSC_MAX_PASSES] = {false};
    bool exported = false;   // the records have been read back since the last pass ended
    // the open pass
    PassPhase phase = PassPhase::Idle;
    PassKind kind = PassKind::Behind;   // (of the launched pass)
    bool range = false;         // run on this rank's chunks (tsc_prune_pass_range), closed by tsc_prune_pass_merge
    // the hand-over
    int opened = -1;            // slot whose state block the device has already written
    int left = -1;              // slot of the pass that was left open on the device
    bool left_local = false;
    int closes = -1;            // the slot the open pass's first kernel closes (Opener::Derives), -1: it has nothing to close
    bool closes_local = false;
    int rows_known_for = -1;    // slot whose row range the device already holds (written by the merge in front of it)
    bool split = false;         // partitioned passes have run: the cache views of the remaining passes hold this rank's keys only

    int next_runnable(int from) const {
        for (int s = from; s < TSC_MAX_PASSES; ++s)
            if (pass_can_run(n, s)) return s;
        return -1;
    }
    int next_slot() const { return next_runnable(scan_from); }   // what next_pass will hand out next (the pass behind the open one)
    bool fresh() const { return phase == PassPhase::Idle && scan_from == 0; }

    // a run over n_ structures: its first kernel opens the first runnable slot
    void start(int64_t n_) { n = n_, opened = next_runnable(0); }
    // next_pass: the open pass is `s` (from next_slot); -1: the schedule is exhausted
    void begin(int s) {
        scan_from = s < 0 ? TSC_MAX_PASSES : s + 1;
        if (s < 0) return;
        slot = s, k = int64_t(KS[s]), phase = PassPhase::Open, range = false, closes = -1;
    }
    // pass_launch: who opens the open pass's slot.  can_derive: the first kernel of the pass can close the pass in front of it
    Handover open_slot(bool range_, bool can_derive) {
        if (opened != slot && left < 0) return Handover{Opener::Nothing, -1, false, -1};
        range = range_, closes = -1;
        if (opened == slot) return Handover{Opener::Opened, -1, false, slot};
        const Handover h{can_derive ? Opener::Derives : Opener::Step, left, left_local, slot};
        if (can_derive) closes = left, closes_local = left_local;
        opened = slot, left = -1;
        return h;
    }
    // pass_launch, at its end: the kernels of the open pass are enqueued
    void launched(PassKind kind_) {
        phase = PassPhase::Launched, kind = kind_, ran[slot] = true;
        if (!range && kind != PassKind::Behind) left_open(kind == PassKind::Local);
    }
    void left_open(bool local) { left = slot, left_local = local; }
    // the last kernel of the launched pass closed it and opened next_slot()
    void closed_on_device() { left = -1, opened = next_slot(); }
    // the pass ends on the host (pass_finish, pass_merge)
    void end_pass() { phase = PassPhase::Idle, slot = -1, k = 0, range = false, exported = false; }
    // stats: a pass left open is closed by a step launch, which opens next_slot() where the run goes on
    Handover close_for_export() {
        if (left < 0) return Handover{Opener::Opened, -1, false, -1};
        const Handover h{Opener::Step, left, left_local, next_slot()};
        left = -1, opened = h.next;
        return h;
    }
    void range_ready(int s) { rows_known_for = s; }   // the merge in front of slot s left this rank's rows of it on the device
    bool rows_ready() const { return rows_known_for == slot; }
    void split_views() { split = true; }
    void merged_views() { split = false; }

    // the call `c` made now: null where it is allowed, else the message it is refused with (TSC_ERR_STATE)
    const char *refusal(StepCall c) const {
        const bool open = phase != PassPhase::Idle, launched = phase == PassPhase::Launched;
        switch (c) {
            case StepCall::NextPass: return open ? "tsc_prune_next_pass: previous pass not finished" : nullptr;
            case StepCall::Estimate: return open ? nullptr : "tsc_prune_pass_estimate: no pass open";
            case StepCall::PassLocal: return phase == PassPhase::Open ? nullptr : "tsc_prune_pass_local: no pass open (call tsc_prune_next_pass)";
            case StepCall::Partitioned: return open ? nullptr : "tsc_prune_pass_partitioned: no pass open";
            case StepCall::PassRange: return phase == PassPhase::Open ? nullptr : "tsc_prune_pass_range: no pass open (call tsc_prune_next_pass)";
            case StepCall::PassMerge: return launched && range ? nullptr : "tsc_prune_pass_merge: tsc_prune_pass_range has not run";
            case StepCall::ViewsPtr: return open ? nullptr : "tsc_prune_views_ptr: no pass open";
            case StepCall::ViewsMerged: return open ? nullptr : "tsc_prune_views_merged: no pass open";
            case StepCall::PassRows:
                return launched && kind == PassKind::Behind ? nullptr : "tsc_prune_pass_rows: needs an open pass whose tsc_prune_pass_local ran with world_size > 1";
            case StepCall::BestPtr: return open ? nullptr : "tsc_prune_best_ptr: no pass open";
            case StepCall::UseBestBuffer: return fresh() ? nullptr : "tsc_prune_use_best_buffer: call it right after tsc_prune_create";
            case StepCall::SetPartition: return fresh() ? nullptr : "tsc_prune_set_partition: call it right after tsc_prune_create";
            case StepCall::PassFinish:
                if (!launched) return "tsc_prune_pass_finish: tsc_prune_pass_local has not run";
                return range ? "tsc_prune_pass_finish: a rank-partitioned pass is closed by tsc_prune_pass_merge" : nullptr;
            case StepCall::Stats: return open ? "tsc_prune_stats: a pass is still open" : nullptr;
        }
        return nullptr;
    }
};

}  // namespace tsc
