// prune_host.hpp -- the host-side state of one prune run (tsc_prune) and the launchers of its pair kernels, which live in translation
// units of their own (pairs_tile.hip, pairs_sieve.hip, pairs_sorted.hip: the template instantiations are most of the library's build time).
#pragma once

#include "cull_mm.hpp"
#include "local_pass.hpp"
#include "pass_cursor.hpp"
#include "pass_plan.hpp"
#include "pass_state.hpp"
#include "prune_api.hpp"
#include "prune_schedule.hpp"
#include "rmsd_tile.hpp"
#include "scan.hpp"

// --------------------------------------------------------------------------------------------------
// K3: prune_conformers_rmsd
//
// A run is a sequence of passes over the schedule of rmsd_pruning.py:186-188.  Nothing in a pass waits for the
// host: the gate of :192 is evaluated on the device (k_pass_step) and every pass that COULD run (20 k < N) is
// enqueued with grids sized for N structures; kernels of a pass that is gated off, and blocks beyond the number
// of still-active structures, return at once.  The host reads the per-pass records once, at the end.

static_assert(MAX_SLOTS == TSC_MAX_PASSES, "one cache view per schedule slot");

struct tsc_prune : Owned {
    explicit tsc_prune(tsc_ctx *c) : Owned(c) {}
    ~tsc_prune() override;   // (prune.hip: the run's events go back to the context's pool)
    void unlisted() override;   // (prune.hip: its pinned flag word and its hold on the context's xd_* buffers)
    const double *heavy = nullptr;
    int64_t n = 0, npad = 0;
    int h = 0, hp = 0;
    double thr = 0;
    int mode = 0;
    int algo = ALGO_SIEVE;  // pair kernel of this run
    // device state
    uint8_t *mask = nullptr;
    int32_t *act = nullptr, *cend = nullptr, *best = nullptr;
    int32_t *bsum = nullptr, *boff = nullptr, *tile_cmax = nullptr, *tile_done = nullptr;
    int32_t *known = nullptr;              // per structure: every still-active column before this position was found dissimilar to it (rmsd.hpp, k_open_rows)
    int32_t *cbeg = nullptr;               // ... as the first column a row of the open pass still has to look at (a tile's smallest: tile_cmax[2 t + 1])
    int n_blocks = 0;                      // scan blocks (SCAN_TILE structures each) the mask is ranked by
    unsigned long long *bits = nullptr;    // two bit copies of the mask (the pass in flight reads one, clears removed rows in the other)
    unsigned long long *views = nullptr;   // cache view of every pass of the schedule, each followed by its summary (pass_state.hpp, CacheViews)
    ViewPass *view_pass = nullptr;         // device: the pass of each view (chunk count, chunk size, its division constants)
    int view_of_slot[TSC_MAX_PASSES] = {};  // schedule slot -> view index (-1: the pass can never run)
    int n_views = 0;
    size_t bit_words = 0, dsum_words = 0;   // (pass_cursor.hpp: bit_words_of, dsum_words_of)
    double *Xr = nullptr, *Xc = nullptr, *G = nullptr;                       // register-tiled kernel
    float *Dall = nullptr;   // sieve kernel: fp32 descriptors of every structure, [n][DW]
    float *Dc = nullptr;     // ... in active order, rewritten by k_open_rows every pass: what the pair kernel reads
    bool mm64 = false;                      // this run takes the 64-row matrix-core kernels (mm.hpp, cull_mm.hpp); else, with records, the 16-row form
    _Float16 *Dh = nullptr;                 // ... and as the float16 records of the matrix-core screen (mm.hpp), in active order too ("sieve_mm")
    _Float16 *Drec = nullptr;               // ... and by STRUCTURE index, written once per run: what the chunk-local pass screens with ("sieve_mm16", local_pass.hpp)
    double *Gall = nullptr;
    struct Tickets {
        PassTickets pass;
        LocalTickets local;
    } *tickets = nullptr;  // arrival counters of the fused pair kernel and of the chunk-local pass kernel
    // culled passes (cull.hpp): allocated when the first one comes up
    int32_t *morton_order = nullptr, *rank_of = nullptr, *crank = nullptr, *cbase = nullptr, *cfill = nullptr, *blk_cnt = nullptr;
    float *Ds = nullptr, *cbox = nullptr, *rbox = nullptr;
    int32_t *cstruct = nullptr;                // the structure at every sorted position (cull_mm.hpp)
    _Float16 *Dhs = nullptr;                   // the float16 records of the matrix-core screen by sorted position (cull_mm.hpp)
    float *heavy32 = nullptr;            // float32 copy of the heavy atoms for stage 1 of the pair kernels (pair_stages.hpp: pair_stage1)
    bool morton_sorted = false;          // the run's Morton order exists (made when the first pass is really culled)
    // rank-partitioned passes (rmsd.hpp, k_pass_merge): set by tsc_prune_set_partition
    int part_rank = 0, part_world = 1, part_min_chunks = 0;
    unsigned long long *exch = nullptr;  // caller-owned exchange buffer: bit_words words of removed rows + 8 of statistics
    uint8_t *export_mask_host = nullptr;  // set by prune_run: pinned host buffer that receives the mask with the statistics
    unsigned *dmax_bits = nullptr;  // device scalar: largest |descriptor component| as float bits (zeroed by k_init_run)
    PassCounters *counters_all = nullptr;  // [TSC_MAX_PASSES]: a slot's counters are zeroed once, by k_init_run, and only ever added to
    PruneState *state_all = nullptr;       // [TSC_MAX_PASSES]: a slot's state block is written by whoever opens the slot, read by its kernels
    PassCounters *counters = nullptr;      // the entries of the pass in flight (pass_launch) -- what every kernel of a pass is handed
    PruneState *state = nullptr;
    PassRecord *records = nullptr;  // [TSC_MAX_PASSES]
    // host state
    PassCursor cur;   // where the run is in the schedule, what is launched of the open pass, who closes and opens a slot on the device
    hipEvent_t ev[TSC_MAX_PASSES][4] = {{nullptr}};  // per slot: pass begin, pair kernel begin, pair kernel end, pass end
    tsc_pass_stats stats[TSC_MAX_PASSES] = {};
    int n_passes = 0;
    bool borrows_xd = false;   // the descriptors (and the float32 copy) are the context's xd_* buffers, written by tsc_embed_masked_dev: the context
                               // must not release them while this run lives (tsc_ctx::xd_borrowers)
    bool det_desc = false;     // the descriptors were built with fixed-order sums ("deterministic_basis"): every rank of a sharded run that fed
                               // its run the same sample holds the same bits -- what row tiles of a SORTED layout dealt among ranks rely on
    bool auto_tile = false;    // ALGO_TILE was this run's own choice (screen_is_useless on its own basis estimate), not the caller's
    int flag_slot = -1;        // this run's word in the context's pinned buffer (the culled-or-walked verdict of a candidate pass)
};

// The pass that follows the open one (what tsc_prune_next_pass will hand out next): the kernel that finishes a pass also closes it and opens
// this one on the device.  local: the open pass runs in the chunk-local kernel (its record says so)
static inline StepArgs next_step_args(const tsc_prune *p, bool local = false) {
    const int nxt = p->cur.next_slot();
    return StepArgs{p->cur.slot, nxt, nxt >= 0 ? (long long)KS[nxt] : 0ll, p->algo, local ? ALGO_LOCAL : -1};
}
// a k_pass_step launch: closes h.prev, opens h.next
static inline StepArgs step_args_of(const tsc_prune *p, const Handover &h) {
    return StepArgs{h.prev, h.next, h.next >= 0 ? (long long)KS[h.next] : 0ll, p->algo, h.prev_local ? ALGO_LOCAL : -1};
}

// range_close: the context of the kernels of a rank-partitioned pass -- their last unit leaves the statistics in the exchange buffer
// instead of closing the pass (pass_step_wave)
// prev / cur: the slots a step closes / opens (StepArgs), -1 for none
static inline StepCtx step_ctx_of(const tsc_prune *p, int prev, int cur) {
    const int of = prev >= 0 ? prev : cur;
    return StepCtx{p->state_all + of, cur >= 0 ? p->state_all + cur : nullptr, p->counters_all + of, p->records, p->bsum, p->boff, p->n_blocks,
                   reinterpret_cast<unsigned *>(p->tickets), int(sizeof(*p->tickets) / 128), nullptr};
}
// the step behind the open pass (next_step_args)
static inline StepCtx step_ctx(const tsc_prune *p, bool range_close = false) {
    StepCtx sc = step_ctx_of(p, p->cur.slot, p->cur.next_slot());
    if (range_close) sc.exch_tail = p->exch + p->bit_words;
    return sc;
}
// the first kernel of the open pass closes the pass that was left open in front of it (pass_state.hpp, pass_derive), or has nothing to close
static inline DeriveArgs derive_args(const tsc_prune *p) {
    DeriveArgs d;
    memset(&d, 0, sizeof(d));
    d.prev = d.cur = -1, d.prev_algo = -1;
    const int prev = p->cur.closes;
    if (prev < 0) return d;
    d.prev_st = p->state_all + prev, d.prev_cnt = p->counters_all + prev, d.rec = p->records;
    d.prev = prev, d.cur = p->cur.slot, d.k_cur = (long long)p->cur.k, d.algo_cur = p->algo;
    d.prev_algo = p->cur.closes_local ? ALGO_LOCAL : -1;
    return d;
}

static inline bool pass_is_partitioned(const tsc_prune *p, int64_t k) {
    return p->part_world > 1 && p->exch && p->algo == ALGO_SIEVE && k >= int64_t(p->part_min_chunks) * p->part_world;
}

// the view of the open pass and of those behind it (reference-exact mode)
static inline unsigned long long *view_of_open_pass(const tsc_prune *p) {
    return p->mode == 0 ? p->views + size_t(p->view_of_slot[p->cur.slot]) * view_stride(p->bit_words) : p->views;
}
// Views of the passes AFTER the open one (where the rows it removes leave their cache keys); none in cache-free mode.
static inline CacheViews later_views(const tsc_prune *p) {
    CacheViews cv;
    cv.views = p->views, cv.stride = (long long)view_stride(p->bit_words), cv.bit_words = int(p->bit_words), cv.n = int(p->n);
    cv.first = p->mode == 0 ? p->view_of_slot[p->cur.slot] + 1 : 0;
    cv.count = p->mode == 0 ? p->n_views : 0;
    cv.pass = p->view_pass;
    return cv;
}

static inline ApplyArgs apply_args(const tsc_prune *p) {
    ApplyArgs a;
    a.g = PassGeom{int(p->n), int(p->cur.k), int(p->n / p->cur.k)};
    a.act = p->act, a.cend = p->cend, a.best = p->best, a.mask = p->mask, a.bits = p->bits, a.bit_words = int(p->bit_words);
    a.bsum = p->bsum, a.block_items = SCAN_TILE, a.cv = later_views(p);
    a.exch = p->cur.range ? p->exch : nullptr;
    return a;
}

// ---- the pair kernels' launchers (plain arguments: the callers fill the argument blocks) ----
// k_rmsd_tile<hp, 16> (pairs_tile.hip); hp = 4, 8, ... 32
int launch_rmsd_tile(int hp, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *Xr, const double *Xc, const double *G, const int32_t *cend,
                     int32_t *best, PassCounters *counters, const PruneState *state, const TileArgs &a);
// k_rmsd_sieve<16, cpl, trim, fused, f32> (pairs_sieve.hip: fused, pairs_sieve_plain.hip: not); the shapes that exist: cpl 1 / 2 / 4 untrimmed, cpl 2
// trimmed, and cpl 2 trimmed with f32
int launch_rmsd_sieve_fused(int cpl, bool trim, bool f32, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act,
                            const double *Gall, const float *Dc, const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state,
                            const SieveArgs &a, const FusedApply &fa);
int launch_rmsd_sieve_plain(int cpl, bool trim, bool f32, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act,
                            const double *Gall, const float *Dc, const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state,
                            const SieveArgs &a, const FusedApply &fa);
// k_rmsd_sieve_mm<fused, f32> (pairs_mm.hip): the screen on the matrix cores, 64 rows per work item
int launch_rmsd_sieve_mm(bool fused, bool f32, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act, const double *Gall,
                         const float *Dc, const _Float16 *Dh, const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state, const SieveArgs &a,
                         const FusedApply &fa);
// k_rmsd_sieve_sorted<f32> and k_pass_chunks (pairs_sorted.hip)
int launch_rmsd_sieve_sorted(bool f32, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act, const double *Gall,
                             const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state, const SieveArgs &a, const CullArgs &ca,
                             int my_tiles, int n_seg);
// k_rmsd_sieve_mm16<fused, f32> (pairs_mm.hip): the matrix-core screen for 16-row items (k_rmsd_sieve's grid)
int launch_rmsd_sieve_mm16(bool fused, bool f32, int waves, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act, const double *Gall,
                           const _Float16 *Dh, const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state,
                           const SieveArgs &a, const FusedApply &fa);
// k_rmsd_sieve_sorted_mm<f32> (pairs_mm.hip): the culled pass with the screen on the matrix cores
int launch_rmsd_sieve_sorted_mm(bool f32, hipStream_t st, dim3 grid, hipEvent_t e0, hipEvent_t e1, const double *heavy, const int32_t *act, const double *Gall,
                                const int32_t *cend, int32_t *best, PassCounters *counters, const PruneState *state, const SieveArgs &a, const CullArgs &ca,
                                const CullMmArgs &cm, int n_groups, int n_seg);
// (mm: the screen on the matrix cores, from the records by structure in a.rec)
int launch_pass_chunks(bool mm, hipStream_t st, unsigned blocks, hipEvent_t e0, hipEvent_t e1, const PassGeom &g, const LocalPassArgs &a, PruneState *state, uint8_t *mask,
                       unsigned long long *bits, int bit_words, const unsigned long long *view, const double *heavy, const double *Gall, const float *Dall,
                       const CacheViews &cv, PassCounters *counters, int32_t *bsum, int block_items, const StepCtx &sc, const StepArgs &sa, LocalTickets *tickets,
                       const DeriveArgs &dv);
