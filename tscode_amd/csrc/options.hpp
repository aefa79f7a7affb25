// options.hpp -- the tunables of a context (tsc_ctx_set_option / tsc_ctx_get_option): their defaults as the member initialisers of
// tsc_options, and one table with a row per option -- name, member, rule -- that setting, reading and listing them walk.  A new option
// is a member with its default, a row, and an entry in the comment above tsc_ctx_set_option in include/tscode_hip.h (a test compares
// the names there with the table).  Host code without a HIP call: tools/probe/options_check.cpp runs it without a GPU.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/tscode_hip.h"

constexpr int OPT_LOCAL_MAX_CHUNK_MAX = 2048;   // the largest "local_max_chunk": LP_MAX_ROWS of local_pass.hpp (pass_plan.hpp asserts that they agree)

struct tsc_options {
    int prune_algo = 0;                   // 0 auto, 1 register-tiled, 2 sieve
    int seg_cols = 0;                     // columns per pair-kernel work item (0 = chosen from the problem size)
    int drain_min = 32;                   // sieve: queued pairs that trigger an evaluation batch between column tiles (swept 16..64 after the row
                                          // loop was trimmed: 32 is 1.3 % ahead of 64 at 1M structures, level elsewhere)
    int sieve_trim = 1;                   // pair kernel: the screen with fewer vector instructions per (row, tile) (norms folded into the fma chain, per-family compares)
    int sieve_mm = 1;                     // pair kernels of a one-rank run with the screen on the matrix cores, 64 rows per work item (mm.hpp, cull_mm.hpp): 0 never (the
                                          // packed-fp32 screen of sieve.hpp / cull.hpp), 1 for runs of at least mm_min_n structures, 2 always
    int64_t mm_min_n = 100000;            // (measured: at 57 000 structures a pass is a few thousand work items and bound by their chains of memory round trips, which
                                          // the longer 64-row items lengthen -- C3 0.80 - 0.89 ms against 0.79; at 483 000 the passes are bound by issue: C4 9.05 -> 7.8 ms)
    int sieve_mm16 = 1;                   // runs below mm_min_n: the walked passes' pair kernel with the matrix-core screen on 16-row items (mm.hpp: k_rmsd_sieve_mm16); 0: the packed-fp32 kernel
                                          // ... and, in runs of any size, the chunk-local pass (16-row tiles as well) with that screen (local_pass.hpp: k_pass_chunks<true>, float16
                                          // records by structure written once per run); 0: its packed-fp32 form
    int mm_seg_cols = 0;                  // ... columns per work item of the walked passes' kernel (0: 1024 where rows' ranges reach 2048 columns, else 512)
    int sieve_cpl = 2;                    // columns per lane of the pair kernel's screen: 2 = 128-column tiles at 5 waves/SIMD (default), 4 = 256-column tiles at 4, 1 = 64-column tiles at 6
    int64_t pca_min_n = 6000;             // below this many structures the descriptors use the identity basis (no principal-axis estimate)
    int fuse_descriptors = 1;             // ... and the descriptors by the kernel that embeds the passing poses (needs early_basis)
    int early_basis = 1;                  // tsc_pipeline_dev: descriptor basis from a sample of unfiltered poses, on its own stream
    int clash_first = 0;                  // ... whose chain is enqueued in front of the clash launch (0) or behind it (1: rounds 1 - 3)
    int cull_tile_block = 256;            // culled passes dealt by row tiles: consecutive tiles of the sorted layout per rank and turn
    int stage1_f32 = 1;                   // stage 1 of the pair kernels reads a float32 copy of the coordinates first (pair_stages.hpp: pair_stage1): 0 never, 2 always,
                                          // 1: from 128 MB of heavy atoms on -- and from 8 MB on where the matrix-core kernels run (want_heavy32 below)
    int local_max_chunk = 384;            // longest chunk (structures) of a pass that the chunk-local kernel takes
    int local_pass = 1;                   // passes with short chunks run in one launch (local_pass.hpp)
    int fused_apply = 1;                  // single-rank sieve passes: the pair kernel applies the verdicts tile by tile and closes the pass (sieve.hpp)
    int skip_known = 1;                   // walked passes of a one-rank run: a row starts behind the columns an earlier pass found dissimilar to it (rmsd.hpp: known[],
                                          // k_open_rows; honoured by the 16-row matrix-core kernel).  0: every row starts behind its diagonal, as the reference walks
    int open_lds_blocks = 1 << 30;        // k_open_rows stages the scan-block prefix in LDS up to this many blocks (tests lower it to take the other path)
    int clash_fp32 = 1;                   // clash verdicts (max_clashes = 0, no counts): packed-fp32 minimum with fp64 fallback
    int clash_lanes = 1;                  // ... of two fragments, the smaller of at most 32 atoms, fused with the embed: one pose per lane (k_clash_lanes)
    int deterministic_basis = 0;          // the descriptor basis from fixed-order sums (descriptor_kernels.hpp, k_feature_moments): a sharded run sets it -- its ranks
                                          // must derive bit-identical descriptors (the culled passes deal the tiles of a layout sorted by them)
    int cull = 1;                         // large passes of the sieve lay their structures out along a Morton curve and skip tile pairs by bounding box (cull.hpp)
    double cull_min_pairs = 2.0e9;        // ... passes of at least this many pairs (n * (n / k) / 2)
    int64_t cull_grid = 1 << 30;          // workgroups of the culled pair kernel at most (each walks work items with that stride)
    int cull_xcd = 1;                     // 1 (default): the culled pair kernel keys runs of 32 row groups to XCDs (workgroup b runs on XCD b % 8): the workgroups an
                                          // XCD has in flight share their column windows in its L2 (cull.hpp; an experiment of round 5)
    int prune_batch_max_n = 2048;         // tsc_prune_rmsd_batch: structures per segment at most (prune_batch.hpp: one workgroup owns a segment); provisional,
                                          // LP_MAX_ROWS -- the size up to which one workgroup already owns a chunk -- until the crossover is measured.
                                          // A longer segment is refused there: it belongs to tsc_prune_rmsd_team (prune_team.hpp: a team of workgroups per
                                          // segment, up to TSC_PRUNE_TEAM_MAX_N structures, no option) or to tsc_prune_rmsd on its own; the Python layer routes
    int pass_timing = 0;                  // HIP events per pass: 0 none, 1 on the pair kernel's dispatch, 2 also around the whole pass
#ifdef TSC_DBG_STAMPS
    int64_t dbg_stamp_k = -1;             // -DTSC_DBG_STAMPS builds: the pass (by its k; -k: its k_open_rows) whose wavefronts leave time stamps
#endif
};

// Does a run over `heavy_bytes` of heavy atoms (n * h * 24) keep the float32 copy that stage 1 of the pair kernels reads?  It pays where the
// candidates' gathers come from HBM (128 MB and more: C4 12.1 -> 10.6 ms in round 4) and where the pair kernel is a chain of round trips rather
// than VALU issue -- the matrix-core kernels: half the bytes and half the trips per evaluation batch (C3: 0.745 -> 0.704 ms); the packed-fp32
// kernel at C3's size lost 2 % to the conversions.
static inline bool want_heavy32(const tsc_options &o, double heavy_bytes) {
    if (o.stage1_f32 != 1) return o.stage1_f32 == 2;
    return heavy_bytes >= 128e6 || (heavy_bytes >= 8e6 && (o.sieve_mm != 0 || o.sieve_mm16 != 0));
}

namespace tsc {

// What a row accepts (a, b, m are the row's numbers; unused ones are 0).  A value that passes is stored converted to the member's type: fractions are cut off.
enum OptRule {
    OPT_ONE_OF,            // a, b or m (two values: b == m)
    OPT_RANGE,             // [a, b]
    OPT_ZERO_OR_MULTIPLE,  // 0, or a value in [a, b] whose whole part is a multiple of m
    OPT_WHOLE,             // a whole number in [a, b]
    OPT_AT_LEAST,          // a or more; stored as b where it is more than b
    OPT_FLAG,              // anything: non-zero is stored as 1
    OPT_ANY,               // anything
};

struct OptionRow {
    const char *name;
    double (*get)(const tsc_options &);
    void (*put)(tsc_options &, double);   // (converts to the member's type)
    OptRule rule;
    double a = 0, b = 0, m = 0;

    // is v accepted?  If not, msg says what is
    bool accepts(double v, char *msg, size_t len) const {
        switch (rule) {
        case OPT_ONE_OF:
            if (v == a || v == b || v == m) return true;
            if (b == m) snprintf(msg, len, "%s must be %g or %g (got %g)", name, a, b, v);
            else snprintf(msg, len, "%s must be %g, %g or %g (got %g)", name, a, b, m, v);
            return false;
        case OPT_RANGE: return (v >= a && v <= b) || (snprintf(msg, len, "%s must be in [%g, %g] (got %g)", name, a, b, v), false);
        case OPT_ZERO_OR_MULTIPLE:
            return v == 0 || (v >= a && v <= b && int(v) % int(m) == 0) ||
                   (snprintf(msg, len, "%s must be 0 (automatic) or a multiple of %g in [%g, %g] (got %g)", name, m, a, b, v), false);
        case OPT_WHOLE: return (v >= a && v <= b && v == double(int(v))) || (snprintf(msg, len, "%s must be a whole number in [%g, %g] (got %g)", name, a, b, v), false);
        case OPT_AT_LEAST: return v >= a || (snprintf(msg, len, "%s must be at least %g (got %g)", name, a, v), false);
        default: return true;
        }
    }
};

template <auto M> double option_member_get(const tsc_options &o) { return double(o.*M); }
template <auto M> void option_member_put(tsc_options &o, double v) { o.*M = std::remove_reference_t<decltype(o.*M)>(v); }
#define TSC_OPTION(member, ...) {#member, option_member_get<&tsc_options::member>, option_member_put<&tsc_options::member>, __VA_ARGS__}

inline const OptionRow OPTION_TABLE[] = {
    TSC_OPTION(prune_algo, OPT_ONE_OF, 0, 1, 2),
    TSC_OPTION(seg_cols, OPT_ZERO_OR_MULTIPLE, 256, 4096, 256),
    TSC_OPTION(drain_min, OPT_RANGE, 1, 64),
    TSC_OPTION(sieve_trim, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(sieve_mm, OPT_ONE_OF, 0, 1, 2),
    TSC_OPTION(mm_min_n, OPT_RANGE, 0, 4e9),
    TSC_OPTION(sieve_mm16, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(mm_seg_cols, OPT_ZERO_OR_MULTIPLE, 64, 1024, 64),
    TSC_OPTION(sieve_cpl, OPT_ONE_OF, 1, 2, 4),
    TSC_OPTION(pca_min_n, OPT_RANGE, 0, 1e9),
    TSC_OPTION(fuse_descriptors, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(early_basis, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(clash_first, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(cull_tile_block, OPT_RANGE, 1, 65536),
    TSC_OPTION(stage1_f32, OPT_ANY),
    TSC_OPTION(local_max_chunk, OPT_RANGE, 16, OPT_LOCAL_MAX_CHUNK_MAX),
    TSC_OPTION(local_pass, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(fused_apply, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(open_lds_blocks, OPT_AT_LEAST, 0, 1073741824.0),
    TSC_OPTION(clash_fp32, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(clash_lanes, OPT_ONE_OF, 0, 1, 1),
    TSC_OPTION(deterministic_basis, OPT_FLAG),
    TSC_OPTION(cull, OPT_ONE_OF, 0, 1, 2),
    TSC_OPTION(cull_min_pairs, OPT_AT_LEAST, 0, HUGE_VAL),
    TSC_OPTION(cull_grid, OPT_AT_LEAST, 1, HUGE_VAL),
    TSC_OPTION(cull_xcd, OPT_FLAG),
    TSC_OPTION(prune_batch_max_n, OPT_WHOLE, 1, TSC_PRUNE_BATCH_MAX_N),
    TSC_OPTION(pass_timing, OPT_ONE_OF, 0, 1, 2),
#ifdef TSC_DBG_STAMPS
    TSC_OPTION(dbg_stamp_k, OPT_ANY),
#endif
};
// A/B switches: set and read by name like the rows above, but not part of the listing (tsc_option_info, whose set of names
// tests/test_options.py pins value by value): they change how a result is reached, never the result, and exist to be measured against.
inline const OptionRow OPTION_SWITCHES[] = {
    TSC_OPTION(skip_known, OPT_ONE_OF, 0, 1, 1),
};

inline const OptionRow *find_option(const char *name, char *msg, size_t len) {
    for (const OptionRow &r : OPTION_TABLE)
        if (strcmp(name, r.name) == 0) return &r;
    for (const OptionRow &r : OPTION_SWITCHES)
        if (strcmp(name, r.name) == 0) return &r;
    snprintf(msg, len, "unknown option '%s'", name);
    return nullptr;
}

// The bodies of tsc_ctx_set_option, tsc_ctx_get_option and tsc_option_info; a refusal's message goes to msg[len].
inline int option_set(tsc_options &o, const char *name, double value, char *msg, size_t len) {
    const OptionRow *r = find_option(name, msg, len);
    if (!r || !r->accepts(value, msg, len)) return TSC_ERR_INVALID;
    r->put(o, r->rule == OPT_FLAG ? (value != 0.0 ? 1.0 : 0.0) : r->rule == OPT_AT_LEAST ? std::fmin(value, r->b) : value);
    return 0;
}
inline int option_get(const tsc_options &o, const char *name, double *value, char *msg, size_t len) {
    const OptionRow *r = find_option(name, msg, len);
    if (!r) return TSC_ERR_INVALID;
    *value = r->get(o);
    return 0;
}
inline int option_info(int index, const char **name, double *default_value) {
    if (index < 0 || index >= int(sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]))) return TSC_ERR_INVALID;
    if (name) *name = OPTION_TABLE[index].name;
    if (default_value) *default_value = OPTION_TABLE[index].get(tsc_options());
    return 0;
}

}  // namespace tsc
