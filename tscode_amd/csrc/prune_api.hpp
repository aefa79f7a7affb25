// prune_api.hpp -- what the units around the prune (pipeline.hip, adjacent.hip's embed-and-prune run, ctx.hip) use of it: the sizes of a
// descriptor basis and its moments, the places of a run's words in the context's pinned buffer, and the entry points prune.hip and
// pipeline.hip define for each other.  Host code and kernel-free headers only; the run itself (tsc_prune) is in prune_host.hpp.
#pragma once

#include "descriptor.hpp"
#include "host.hpp"
#include "shapes.hpp"

// Doubles of a descriptor basis: KD rows per feature family, then the DW projections of the mean feature vector (+ 1 spare)
// ... and, behind the DW projections, the two families' mean squared descriptor distance over the sample (k_descriptor_basis)
static inline size_t basis_doubles(int h) { return size_t(KD) * (n_features(h, 0) + n_features(h, 1)) + DW + NFAM + 1; }
static inline size_t basis_spread_offset(int h) { return size_t(KD) * (n_features(h, 0) + n_features(h, 1)) + DW; }
constexpr size_t PINNED_SPREAD_OFFSET = 8192;  // where a basis' two spread values land in the context's pinned buffer
constexpr size_t PINNED_FLAG_OFFSET = PINNED_SPREAD_OFFSET + 128;  // ... and the culled-or-walked verdicts of the context's runs, one 64-byte line each
constexpr int PINNED_FLAG_SLOTS = 64;
constexpr size_t PINNED_COUNT_OFFSET = PINNED_FLAG_OFFSET + 64 * size_t(PINNED_FLAG_SLOTS);  // ... and the pipeline's count of passing poses (scan.hpp: total_host)
constexpr int64_t AUTO_TILE_MIN_N = 30000;     // a prune of its own (no pipeline around it) spends a synchronisation on the question from here on

// "Would the screen let (almost) every pair through?"  Two structures of the sample lie 2 sum_k lambda_k apart, on average, in a
// family's squared descriptor distance; the screen drops a pair only where a family's distance exceeds h thr^2.  Where BOTH families'
// averages stay below that limit most pairs reach H = p^T q whatever the screen does, and the register-tiled all-pairs kernel, which
// forms H for every pair at 2.5e10 pairs/s, beats the sieve's evaluation stage at 5e9 (profiles/r03_hard_workloads.json: 8 ms
// against 46 on 100 000 structures whose descriptors coincide, cache-free mode).  Either kernel gives the same verdicts.
// Asked in the cache-free mode only: in the reference-exact mode the cache's stop columns end nearly every row early on such an ensemble
// (13 M pair evaluations where the cache-free mode makes 191 M), and with so few pairs the sieve's cheaper passes win (2.6 against 3.6 ms).
static inline bool screen_is_useless(const double *spread, int h, double thr) {
    const double limit = double(h) * thr * thr;
    return spread[0] < limit && spread[1] < limit;  // (false for NaN / +inf: no estimate)
}

// Basis of the descriptors: leading principal axes of the two feature families (descriptor.hpp) over `n_samples` structures
// heavy[stride * i], into d_Q (basis_doubles(h)).  Enqueued on `st`; the scratch it takes from `s` must outlive the kernels.
static inline size_t moment_doubles(int h) {  // (MOM_BLOCKS partial matrices per family: k_feature_moments)
    const size_t a = size_t(n_features(h, 0) + 1), b = size_t(n_features(h, 1) + 1);
    return size_t(MOM_BLOCKS) * (a * a + b * b) + 1;  // (+ the two arrival counters of k_feature_moments, in the last double)
}

// (prune.hip) d_moments (optional): moment_doubles(h) doubles already zeroed on `st` by the caller; otherwise taken from `s` and cleared there
int build_basis(tsc_ctx *c, hipStream_t st, Scratch &s, const double *heavy, int h, int n_samples, int64_t stride, double *d_Q,
                unsigned *zero_word = nullptr, double *d_moments = nullptr, double *spread_host = nullptr);

// Descriptors built outside the prune (tsc_pipeline_dev: by the kernel that embeds the passing poses)
struct ExternalDescriptors {
    float *D = nullptr;
    double *G = nullptr;
    unsigned *dmax_bits = nullptr;
    float *heavy32 = nullptr;  // (optional) the float32 copy of the heavy atoms, written by the kernel that embedded them
};

// (pipeline.hip) the basis that tsc_embed_clash_compact_dev left for the tsc_prune_create that follows, or null
const double *pending_basis(const tsc_ctx *c, int h);

// (prune.hip) one whole run on device data; mask_host (optional) also receives the verdicts, copied before the run's single
// synchronisation (the statistics read-back)
int prune_run(tsc_ctx *c, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask, uint8_t *mask_host,
              tsc_pass_stats *stats, int *n_passes, const double *basis = nullptr, const ExternalDescriptors *ext = nullptr, int force_algo = -1);
