/*
 * tscode_hip.h -- C ABI of libtscode_hip.so, the MI355X (gfx950) engine for TSCoDe's geometry hot path.
 *
 * The reference (ntampellini/TSCoDe v0.4.16) is pure Python + Numba: the path has no FFI or plugin
 * table, callers bind plain Python functions by name.  Each entry point below states the
 * reference function (file:line under the reference root) whose work it takes over; the Python
 * mirror that keeps the reference's call signatures is tscode_amd/ (see INTEGRATION.md for the
 * binding a TSCoDe maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types cross the boundary.
 *   - every function returns 0 on success and a negative tsc_status on failure; tsc_last_error()
 *     returns a thread-local, human-readable message for the last failure on the calling thread.
 *   - there is NO CPU path in this library: without a usable HIP device every call fails with
 *     TSC_ERR_NO_DEVICE.
 *   - all coordinates are C-contiguous float64 (Angstrom), index arrays int32 unless stated.
 *   - "host" entry points take host pointers, copy in/out and synchronise before returning;
 *     "_dev" entry points take device pointers valid on the context's device, enqueue on the
 *     context's stream and return without synchronising unless stated.
 *   - the caller owns every buffer it passes; the library keeps no pointer after return except
 *     inside a tsc_prune object, which borrows `heavy` until tsc_prune_destroy.
 *   - MULTI-GPU, a deliberate deviation from SURVEY.md 8(b): that sketch has "multi-GPU variants take a device list / an RCCL
 *     communicator held in tsc_ctx".  This library opens no communicator and spawns no process.  The path shards as one
 *     process per GPU, each with a context of its own, and the exchange steps (one all-gather of the surviving heavy-atom
 *     shards -- or none, when every rank embeds all poses itself: the host times both forms on its node -- and one
 *     all-reduce(MIN) over best[] per sharded pass) belong to the HOST that owns the process group: in this
 *     repository torch.distributed over RCCL (tscode_amd/pipeline.py::sharded_step), in a C host ncclAllGather /
 *     ncclAllReduce on the same device pointers.  What the C ABI provides for it is the part only the library can do: a
 *     rank's block of poses (tsc_embed_clash_compact_dev), the stepping form of the prune with the row tiles of a pass dealt to
 *     (rank, world_size) and best[] in a caller-owned buffer the collective can run on (tsc_prune_create ..
 *     tsc_prune_pass_local(rank, world_size) .. tsc_prune_use_best_buffer .. tsc_prune_pass_finish), and
 *     tsc_ctx_set_stream, so that kernels and collectives are ordered on one stream.  Linking RCCL into the library would tie
 *     it to one launcher and one communicator lifetime for no kernel's benefit.
 *   - a context (tsc_ctx: one device, its streams, its scratch cache) is for ONE thread at a time, like the reference's
 *     callers (single-threaded Python; multiembed.py uses processes): threads that want to work concurrently create a
 *     context each.  Any number of processes may use a device at once (tests/: three processes stepping one GPU).
 */
#ifndef TSCODE_HIP_H
#define TSCODE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSC_VERSION 100 /* 0.1.0 */

typedef enum {
    TSC_OK = 0,
    TSC_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, unsupported shape) */
    TSC_ERR_NO_DEVICE = -2, /* no HIP device / HIP runtime failure at context creation */
    TSC_ERR_HIP = -3,       /* a HIP call failed; message has the HIP error string */
    TSC_ERR_NOMEM = -4,     /* device or host allocation failed */
    TSC_ERR_STATE = -5      /* call sequence violated (prune stepping API) */
} tsc_status;

typedef struct tsc_ctx tsc_ctx;     /* one per (process, device); owns a stream and scratch memory */
typedef struct tsc_prune tsc_prune; /* state of one prune_conformers_rmsd run (stepping API) */
typedef struct tsc_rot_corr tsc_rot_corr; /* state of one prune_conformers_rmsd_rot_corr run */
typedef struct tsc_rot_corr_batch tsc_rot_corr_batch; /* ... of one run over many ensembles */

/* ---- library / context ------------------------------------------------------------------ */
int tsc_version(void);
const char *tsc_last_error(void);
/* SHA-256 (16 hex digits) of the kernel sources this binary was built from (tscode_amd/build.py passes it to the compiler;
 * "unrecorded" for a build by other means): lets a measurement tie its numbers to the binary that ran, not to the sources beside it. */
const char *tsc_build_digest(void);
int tsc_device_count(void); /* >= 0, or a negative tsc_status */
int tsc_ctx_create(int device, tsc_ctx **out);
/* (tsc_ctx_destroy takes the objects created from the context that are still alive with it: "objects created from a context", below) */
int tsc_ctx_destroy(tsc_ctx *ctx);
/* Run on a caller-provided hipStream_t; NULL = the library's own (non-blocking) stream.  Note that PyTorch's DEFAULT stream has
 * the handle 0 = NULL: to order this library's kernels with torch work (copies, RCCL collectives) make an explicit
 * torch.cuda.Stream current and pass its .cuda_stream here (tscode_amd/pipeline.py does). */
int tsc_ctx_set_stream(tsc_ctx *ctx, void *hip_stream);
int tsc_ctx_synchronize(tsc_ctx *ctx);
/* Tunables, one entry per option in the order of the table that defines them (csrc/options.hpp: name, default and what is accepted).
 * A value outside what an option accepts is refused (TSC_ERR_INVALID; the message names the option, what it takes and the value given)
 * and leaves the option as it was; fractions are cut off.
 *   "prune_algo": 0 = automatic (default), 1 = register-tiled all-pairs kernel (<= 32 heavy atoms), 2 = descriptor sieve (any size);
 *   "seg_cols": columns per pair-kernel work item (multiple of 256, at most 4096; 0 = automatic, the default);
 *   "drain_min": queued pairs that trigger an evaluation batch in the sieve kernel (1..64, default 32);
 *   "sieve_trim": 1 (default) = the screen's shorter instruction sequence, 0 = the other screen;
 *   "sieve_mm": the pair kernels with the descriptor screen on the matrix cores and 64 rows per work item (csrc/mm.hpp, cull_mm.hpp):
 *      0 never, 1 (default) in runs of at least mm_min_n structures, 2 always;
 *   "mm_min_n": the number of structures from which sieve_mm 1 takes the 64-row kernels (0 .. 4e9, default 100000);
 *   "sieve_mm16": 1 (default) = smaller runs take the matrix-core screen on 16-row work items (k_rmsd_sieve_mm16), 0 = the packed-fp32 screen;
 *      the one-launch chunk-local kernel (see local_pass below; 16-row tiles too) follows it in runs of any size: at 1 a run whose schedule can hold such a
 *      pass keeps a second set of float16 records, by structure index, written once when the run is created (64 bytes per structure);
 *      verdicts, masks and pairs_evaluated are the same either way;
 *   "mm_seg_cols": columns per work item of the walked passes' 64-row kernel (a multiple of 64 up to 1024; 0 = automatic, the default);
 *   "sieve_cpl": columns per lane of the sieve kernel's screen, 1, 2 (default) or 4 -- register footprint against occupancy;
 *   "pca_min_n": ensembles smaller than this (0 .. 1e9, default 6000) take the identity basis for their descriptors instead of estimated
 *      principal axes (three launches and about 45 us less per run; any basis gives the same verdicts);
 *   "fuse_descriptors": 1 (default) lets the kernel that embeds the passing poses write their descriptors as well, under early_basis
 *      (poses of up to about 80 heavy atoms; otherwise and with 0 a separate launch reads the coordinates back);
 *   "early_basis": 1 (default) lets tsc_pipeline_dev estimate the descriptor basis of the prune from a sample of the unfiltered
 *      poses on a side stream while the clash kernel runs (the choice of basis never changes a verdict); 0 = from the filtered
 *      structures, on the main stream;
 *   "clash_first": 0 (default) = tsc_pipeline_dev enqueues the chain that estimates the early basis in front of the clash launch,
 *      1 = behind it;
 *   "cull_tile_block" (1 .. 65536, default 256): a culled pass dealt to several ranks by row tiles (tsc_prune_pass_local(rank, world)) gives
 *      a rank runs of this many consecutive tiles of the sorted layout -- neighbours on the curve share their columns, and a row's early
 *      exit knows more of what was found;
 *   "stage1_f32": the pair kernels' first look at a pair that passed the screen (H = p^T q and the quartic tests) reads a float32 copy
 *      of the coordinates with the rounding bound that goes with it, the float64 coordinates only for what that leaves undecided:
 *      0 = never, 1 (default) = in runs with 128 MB of heavy-atom coordinates or more (where the gathers come from HBM) -- with 8 MB
 *      or more where the matrix-core kernels run --, 2 = always (the value is not checked: any other means never);
 *   "local_max_chunk": see local_pass (16 .. 2048, default 384);
 *   "local_pass": 1 (default) lets passes whose longest chunk has at most local_max_chunk structures run in the one-launch
 *      chunk-local kernel;
 *   "fused_apply": 1 (default) lets the sieve kernel of a single-rank pass apply a row tile's verdicts itself when the tile's last
 *      work item finishes and close the pass (two launches per pass); 0 = tsc_prune_pass_finish launches k_apply_pass (always so for
 *      the register-tiled kernel and for passes searched by several ranks);
 *   "open_lds_blocks": scan blocks (2048 structures each) up to which the per-row kernel stages their prefix in LDS (default: its
 *      capacity, 2048; 0 = always read it from memory; tests; not negative, and more than 2^30 is stored as 2^30);
 *   "clash_fp32": 1 (default) decides verdict-only clash masks by a packed-fp32 minimum with fp64 fallback;
 *   "clash_lanes": 1 (default) lets such a mask of two fragments, the smaller of at most 32 atoms, be decided by the kernel that embeds
 *      the poses, one pose per lane (k_clash_lanes); 0 = by the clash kernel;
 *   "deterministic_basis": 1 = the descriptor basis from fixed-order sums, so that every rank of a sharded run derives bit-identical
 *      descriptors and hence the same layout (default 0: atomics, 35 us faster; any non-zero value counts as 1).  A run remembers which
 *      of the two it was created under: only a run created under 1 culls a pass whose ROW TILES are dealt to several ranks
 *      (tsc_prune_pass_local / tsc_prune_pass_rows with world_size > 1 -- the ranks deal the tiles of ONE sorted layout); a run created
 *      under 0 walks such a pass in index order, and refuses it (TSC_ERR_STATE) when it had itself chosen the all-pairs kernel from its
 *      own basis estimate (prune_algo 0), a choice that ranks with different estimates could make differently;
 *   "cull": 1 (default) lets the large passes of the sieve (at least cull_min_pairs pairs, fewer than 64 chunks) lay their active
 *      structures out along a Morton curve of the descriptors and skip the tile pairs whose bounding boxes lie beyond the screen's limit,
 *      where the rows' ranges are long enough for that to pay (decided per pass on the device, one synchronisation); 0 = never,
 *      2 = every such pass (tests);
 *   "cull_min_pairs": the pairs n (n / k) / 2 from which a pass is large in the sense of cull (not negative, default 2e9);
 *   "cull_grid": workgroups of the culled pair kernel at most, each walking work items with that stride, where cull_xcd is 0
 *      (at least 1, default 2^30);
 *   "cull_xcd": 1 (default) = the culled pair kernel keys runs of 32 row groups to XCDs (workgroup b runs on XCD b % 8), so that the
 *      workgroups an XCD has in flight share their column windows in its L2; 0 = work items in plain order (any non-zero value counts as 1);
 *   "prune_batch_max_n": structures per segment that tsc_prune_rmsd_batch takes at most (a whole number, 1 .. 8192, default 2048; see there);
 *   "pass_timing": HIP events for tsc_pass_stats.gpu_ms / tile_ms and the pipeline's stage timings: 0 = none (default; an
 *      event record in the stream costs about 4 us on MI355X), 1 = the pair kernel's own start/stop events (tile_ms; passes run by the
 *      chunk-local kernel carry theirs at level 2 only), 2 = also around every whole pass (gpu_ms) and the stages of tsc_pipeline_dev.
 * (A library built with -DTSC_DBG_STAMPS has one more, dbg_stamp_k: tools/stamps.py.)
 * One A/B switch is set and read by name in the same way but is not listed by tsc_option_info -- it changes how a result is reached, never
 * the result: skip_known, 1 (default) = in the walked passes of a one-rank run a row starts behind the columns that an earlier pass of
 * the run already found dissimilar to it (a pair's verdict depends on its two structures alone, and the mask only shrinks), where the
 * pass's pair kernel takes the hint (the 16-row matrix-core kernel); 0 = every row starts behind its diagonal.  Masks, pairs_evaluated,
 * new_keys and the cache keys are the same either way; tsc_pass_stats.pairs_known says how many pairs a pass left out. */
int tsc_ctx_set_option(tsc_ctx *ctx, const char *name, double value);
/* The current value of a tunable as it is stored: every option can be read ("deterministic_basis" set to 5 reads 1). */
int tsc_ctx_get_option(tsc_ctx *ctx, const char *name, double *value);
/* The options by index, without a context: the name and the default of option `index` (either pointer may be NULL), TSC_ERR_INVALID
 * past the last one.  Lets a host or a test list the options without a list of its own. */
int tsc_option_info(int index, const char **name, double *default_value);
/* Device memory helpers for hosts that do not bring their own allocator (tests, C callers). */
int tsc_malloc(tsc_ctx *ctx, size_t bytes, void **dptr);
int tsc_free(tsc_ctx *ctx, void *dptr);
int tsc_memcpy_h2d(tsc_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
int tsc_memcpy_d2h(tsc_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
/* HIP-event timing of everything enqueued on the context's stream between begin and end (ms). */
int tsc_timer_begin(tsc_ctx *ctx);
int tsc_timer_end(tsc_ctx *ctx, float *elapsed_ms); /* synchronises */

/* ---- objects created from a context ------------------------------------------------------- */
/* Five kinds of object are created from a context, live longer than one call and hold memory of that context: tsc_prune
 * (tsc_prune_create), tsc_rot_corr (tsc_rot_corr_begin), tsc_rot_corr_batch (tsc_rot_corr_batch_begin), tsc_embed_prune
 * (tsc_embed_prune_create) and tsc_xchg (tsc_xchg_create).  One rule holds for all of them:
 *   - the context lists every such object while it lives;
 *   - tsc_<kind>_destroy takes the object off the list and frees it: its device blocks go back to the context's scratch cache, a prune
 *     run's events to the context's pool, an exchange closes the peers' mappings and frees its receive area.  NULL is success.  All but
 *     tsc_prune_destroy wait for the context's stream first; tsc_prune_destroy does not wait (its blocks are recycled in stream order,
 *     behind the kernels that still read them), so a run can be created and destroyed per step without a synchronisation;
 *   - tsc_ctx_destroy waits for the context's streams and then destroys the objects it still lists, newest first, before it frees anything
 *     of its own: a host whose finalisers run in no particular order leaks nothing and frees nothing twice;
 *   - a handle is dead after its destroy AND after the destroy of its context: do not hand it to tsc_<kind>_destroy, or to anything else,
 *     afterwards, and never destroy it twice.  Neither is detected. */

/* ---- K1: batched rigid-body embedding ------------------------------------------------------
 * Replaces get_embed (tscode/embeds.py:961-969) and transform_coords (tscode/algebra.py:390-400),
 * batched over poses:  out[s] = concat_m ( rot[s,m] @ X_m[conf_idx[s,m]].T ).T + pos[s,m].
 *   frags      f64, all fragments back to back; fragment m is [n_conf[m], n_atoms[m], 3] at frags + frag_off[m]
 *   frag_off   i64[n_mols] offsets into frags, in doubles
 *   conf_idx   i32[n_poses, n_mols];  rot f64[n_poses, n_mols, 3, 3];  pos f64[n_poses, n_mols, 3]
 *   out        f64[n_poses, sum(n_atoms), 3]
 * n_mols <= 8. */
int tsc_transform_batch(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                        const int32_t *n_conf, int n_mols, const int32_t *conf_idx, const double *rot,
                        const double *pos, int64_t n_poses, double *out);
int tsc_transform_batch_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off_host, const int32_t *n_atoms_host,
                            const int32_t *n_conf_host, int n_mols, const int32_t *conf_idx, const double *rot,
                            const double *pos, int64_t n_poses, double *out);

/* ---- K2: compenetration (clash) mask ---------------------------------------------------------
 * Replaces compenetration_check (tscode/numba_functions.py:59-105), count_clashes (:49-56) and the
 * all_dists it calls (tscode/algebra.py:98-157), batched as in compenetration_refining
 * (tscode/embedder.py:1243-1248):  mask[s] = compenetration_check(coords[s], ids, thresh, max_clashes).
 *   coords f64[n_poses, n_atoms, 3]; ids i32[n_ids] fragment lengths (contiguous ranges), n_ids in {0,2,3};
 *   n_ids == 0 is ids=None: count_clashes (ordered self pairs with 0 < d < 0.5; thresh is ignored).
 *   mask u8[n_poses] (1 = passes); counts (optional, may be NULL) i32[n_poses] = total pair count
 *   (for 3 fragments the count over all three fragment pairs: the reference's early exits do not
 *   change the verdict, total <= max_clashes). */
int tsc_clash_mask(tsc_ctx *ctx, const double *coords, int64_t n_poses, int n_atoms, const int32_t *ids, int n_ids,
                   double thresh, int64_t max_clashes, uint8_t *mask, int32_t *counts);
int tsc_clash_mask_dev(tsc_ctx *ctx, const double *coords, int64_t n_poses, int n_atoms, const int32_t *ids_host, int n_ids,
                       double thresh, int64_t max_clashes, uint8_t *mask, int32_t *counts);
/* Fused K1+K2: the clash verdict of every pose straight from its (rot, pos), no pose materialised
 * (the embed loops of tscode/embeds.py:116-118 and :713-714 do get_embed then compenetration_check). */
int tsc_embed_clash_mask_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off_host, const int32_t *n_atoms_host,
                             const int32_t *n_conf_host, int n_mols, const int32_t *conf_idx, const double *rot,
                             const double *pos, int64_t n_poses, double thresh, int64_t max_clashes, uint8_t *mask,
                             int32_t *counts);
/* All-distances matrix of one pair of point sets (tscode/algebra.py:98-157), for value parity tests. */
int tsc_all_dists(tsc_ctx *ctx, const double *a, int na, const double *b, int nb, double *out);

/* ---- ordered compaction helpers (device) --------------------------------------------------------
 * n_kept = count_nonzero(mask); dst[rank(s)] = src[s] for mask[s] != 0, order preserved (NumPy's
 * structures[mask], tscode/rmsd_pruning.py:206, tscode/embedder.py:1250-1251).  row_bytes % 8 == 0.
 * tsc_gather_heavy_dev additionally keeps only the listed atoms: dst[rank(s), a] = src[s, heavy_idx[a]]
 * (structures[:, atomnos != 1], tscode/rmsd_pruning.py:178-179); mask may be NULL (keep all). */
int tsc_compact_rows_dev(tsc_ctx *ctx, const void *src, const uint8_t *mask, int64_t n_rows, int64_t row_bytes, void *dst,
                         int64_t *n_kept_host);
int tsc_gather_heavy_dev(tsc_ctx *ctx, const double *coords, const uint8_t *mask, int64_t n_poses, int n_atoms,
                         const int32_t *heavy_idx_host, int n_heavy, double *heavy_out, int64_t *n_kept_host);
/* The first half of tsc_pipeline_dev on its own (one rank's block of the pose axis in the sharded protocol): fused
 * embed + clash verdicts, ordered compaction, then the passing poses embedded straight into `structures` (all atoms,
 * may be NULL) and `heavy` (their heavy atoms, f64[n_pass, n_heavy, 3]) -- rejected poses are never materialised.
 * n_pass_host receives the count (the call synchronises for it while the embed runs).  With "early_basis" (default) the call also
 * estimates a descriptor basis from a sample of these poses on a side stream; the next tsc_prune_create on this context with
 * the same heavy-atom count uses it (once) instead of estimating its own -- a choice that never changes a verdict. */
int tsc_embed_clash_compact_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf,
                                int n_mols, const int32_t *conf_idx, const double *rot, const double *pos, int64_t n_poses,
                                const int32_t *heavy_idx, int n_heavy, double clash_thresh, int64_t max_clashes, uint8_t *clash_mask,
                                double *structures, double *heavy, int64_t *n_pass_host);

/* The two halves of the above as calls of their own, for a front half that is spread over ranks differently (tscode_amd/pipeline.py,
 * front = "hybrid": every rank takes the clash verdicts of ITS block of poses -- tsc_embed_clash_mask_dev --, the verdicts are
 * summed over the ranks, one byte per pose, and every rank then embeds the heavy atoms of ALL passing poses itself: recomputing a
 * pose from its 100 bytes of parameters costs less than moving its 24 n_heavy bytes of coordinates over xGMI).
 * tsc_basis_from_poses_dev: forks the estimate of the prune's descriptor basis from a sample of these poses onto the context's side
 *   stream (about 50 us that whatever is enqueued next on the main stream hides); consumed once, by tsc_embed_masked_dev or
 *   tsc_prune_create on this context.
 * tsc_embed_masked_dev: the poses selected by mask u8[n_poses] (device), embedded in order: structures f64[n_sel, n_atoms, 3]
 *   and / or heavy f64[n_sel, n_heavy, 3] (either may be NULL).  With `heavy` and a pending basis the kernel writes the prune's
 *   descriptors as well, and the next tsc_prune_create on this context over the same `heavy` takes them instead of reading the
 *   coordinates back.  n_sel_host (optional): count of selected poses (the call then synchronises for it while the embed runs).
 *   That run BORROWS the context's descriptor buffers until tsc_prune_destroy: a later tsc_embed_masked_dev on the same context that
 *   would have to regrow them while it lives fails with TSC_ERR_STATE instead of pulling them from under it. */
int tsc_basis_from_poses_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf, int n_mols,
                             const int32_t *conf_idx, const double *rot, const double *pos, int64_t n_poses, const int32_t *heavy_idx, int n_heavy);
int tsc_embed_masked_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf, int n_mols,
                         const int32_t *conf_idx, const double *rot, const double *pos, int64_t n_poses, const uint8_t *mask,
                         const int32_t *heavy_idx, int n_heavy, double *structures, double *heavy, int64_t *n_sel_host);

/* ---- K3: Kabsch RMSD (no centring) ------------------------------------------------------------
 * Replaces rmsd_and_max_numba (tscode/rmsd_pruning.py:6-41) on listed pairs of one heavy-atom array:
 * (rmsd[k], maxdev[k]) = rmsd_and_max_numba(heavy[pairs[k,0]], heavy[pairs[k,1]]).
 *   heavy f64[n_structs, h, 3]; pairs i32[n_pairs, 2]. */
int tsc_rmsd_pairs(tsc_ctx *ctx, const double *heavy, int64_t n_structs, int h, const int32_t *pairs, int64_t n_pairs,
                   double *rmsd, double *maxdev);
int tsc_rmsd_pairs_dev(tsc_ctx *ctx, const double *heavy, int64_t n_structs, int h, const int32_t *pairs, int64_t n_pairs,
                       double *rmsd, double *maxdev);

/* ---- Cross-set RMSD: queries against a library (csrc/cross.hpp) ---------------------------------
 * Every pair (query q, library l) is rmsd_and_max_numba(queries[q], library[l]) (tscode/rmsd_pruning.py:6-41): the optimal proper rotation
 * of the query onto the library structure, no centring, rmsd = sqrt(sum |Rp - q|^2 / h), maxdev = max_a |Rp_a - q_a|.
 *   queries f64[n_queries, n_atoms, 3]; library f64[n_library, n_atoms, 3], or NULL: the queries themselves (n_library == n_queries);
 *   idx i32[n_idx]: the atoms compared (:178-179 compares those with atomnos != 1), or NULL with n_idx = 0: all atoms (as :208-224);
 *   center != 0: every structure, queries and library alike, has the mean of its compared atoms subtracted first (not in the reference:
 *   its metric counts translation as deviation).  Up to 2^31 - 1 structures per side.
 * The forms on host arrays check idx, upload and return when the outputs are in the caller's arrays.  The _dev forms take device pointers
 * for every array (idx included: an index outside 0 .. n_atoms - 1 reads as the origin), upload nothing, enqueue on the context's stream and
 * return without waiting for it; coordinates that are not finite are the caller's business there (such a pair has no defined value, is
 * similar to nothing and nearest to nothing).
 * tsc_rmsd_cross: rmsd, maxdev f64[n_queries, n_library], contiguous along the library.  capacity: the doubles each output array has room
 *   for; a request beyond it is refused (TSC_ERR_INVALID) -- walking a large matrix in row blocks is the caller's job, and
 *   tsc_rmsd_cross_rows says how many query rows a call may take so that the two outputs stay within max_bytes (at least 1).
 * tsc_rmsd_cross_first: first i32[n_queries] = the lowest l with rmsd < thr and maxdev < 2 thr (:75, :208-224: _rmsd_similarity(query,
 *   library, thr) is first != INT32_MAX), or INT32_MAX.
 * tsc_rmsd_cross_nearest: index i32[n_queries] = the l of the smallest rmsd (ties: the lowest l), rmsd / maxdev f64[n_queries] its values
 *   (:6-41); n_library >= 1.  Two calls on the same input return the same bits. */
int tsc_rmsd_cross_rows(int64_t n_library, int64_t max_bytes, int64_t *rows);
int tsc_rmsd_cross(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                   const int32_t *idx, int n_idx, int center, double *rmsd, double *maxdev, int64_t capacity);
int tsc_rmsd_cross_dev(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                       const int32_t *idx, int n_idx, int center, double *rmsd, double *maxdev, int64_t capacity);
int tsc_rmsd_cross_first(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                         const int32_t *idx, int n_idx, int center, double thr, int32_t *first);
int tsc_rmsd_cross_first_dev(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                             const int32_t *idx, int n_idx, int center, double thr, int32_t *first);
int tsc_rmsd_cross_nearest(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                           const int32_t *idx, int n_idx, int center, int32_t *index, double *rmsd, double *maxdev);
int tsc_rmsd_cross_nearest_dev(tsc_ctx *ctx, const double *queries, int64_t n_queries, const double *library, int64_t n_library, int n_atoms,
                               const int32_t *idx, int n_idx, int center, int32_t *index, double *rmsd, double *maxdev);

/* ---- Energy-ordered RMSD prune: every cluster collapses to its first member (csrc/leader.hpp) -----
 * The greedy filter of the embed loops (tscode/embeds.py:715, :843) for a whole ensemble, with an optional library that is never removed:
 *     for s in order:  s is removed iff some row KEPT before it -- the library rows in index order, then this call's kept rows in the order
 *                      they were kept -- is similar to it: rmsd_and_max_numba(s, k) (tscode/rmsd_pruning.py:6-41: s turned onto k, no
 *                      centring) has rmsd < thr and maxdev < 2 thr (:75, :208-224); it is represented by the first such k.
 * A removed row never covers anything.  structures f64[n, n_atoms, 3]; library f64[n_library, n_atoms, 3] or NULL with n_library = 0; idx /
 * n_idx / center as the cross-set calls above take them; order i32[n], a permutation of 0 .. n - 1 (ascending energy), or NULL: the rows
 * as they lie.  n, n_library and n + n_library up to 2^31 - 1.  Outputs, indexed by the CALLER's rows: mask u8[n] (1: kept); rep i32[n]: a
 * kept row itself, a removed row the kept row of this call it fell to, -1 where a library row covered it; lib_rep i32[n]: that library
 * row, else -1; *n_kept (host): the rows kept.
 * tsc_prune_rmsd_ordered takes host arrays, checks idx and that order is a permutation, uploads and returns when the outputs are in the
 * caller's arrays.  tsc_prune_rmsd_ordered_dev takes device pointers for every array (order included, unchecked), uploads nothing and
 * enqueues on the context's stream; the rule is walked in blocks of tsc_leader_block() rows of the order and the kept count of a block
 * (4 bytes) comes back to the host before the next block is enqueued, so the stream is idle and the outputs complete when it returns.
 * Coordinates that are not finite are the caller's business there. */
int tsc_leader_block(void);
int tsc_prune_rmsd_ordered(tsc_ctx *ctx, const double *structures, int64_t n, const double *library, int64_t n_library, int n_atoms,
                           const int32_t *idx, int n_idx, int center, const int32_t *order, double thr, uint8_t *mask, int32_t *rep,
                           int32_t *lib_rep, int64_t *n_kept);
int tsc_prune_rmsd_ordered_dev(tsc_ctx *ctx, const double *structures, int64_t n, const double *library, int64_t n_library, int n_atoms,
                               const int32_t *idx, int n_idx, int center, const int32_t *order, double thr, uint8_t *mask, int32_t *rep,
                               int32_t *lib_rep, int64_t *n_kept);

/* The descriptor screen of the prune's pair kernel as the matrix cores compute it (csrc/mm.hpp), for tests: the screen values
 * S[fam][r][c] (two feature families, rows r < 64, columns c < n) of the first 64 of n descriptors against all n, in the units the
 * kernel compares them in -- out_scale^2 times |D_fam[r] - D_fam[c]|^2 up to the error bound of mm.hpp -- and the limit the kernel
 * holds them against for a squared-distance limit `limit` = h thr^2 (as a float's bit pattern; INT32_MAX - 1: nothing is dropped).
 *   D f32[n, 16] host (component 2 k + fam, as the library stores descriptors); S f32[2, 64, n] host. */
int tsc_screen_mm_values(tsc_ctx *ctx, const float *D, int64_t n, double limit, float *S, int32_t *limit_bits, float *out_scale);
/* The same screen's VERDICTS in the form the pair kernels compute them: the accumulator of every product starts at minus the limit and a
 * pair is kept where both families' results come out negative (their sign bits), so the limit is one of the summed terms and the rounding
 * is not that of comparing S with the limit afterwards.  Same inputs, records and operand loads; keep u8[64, n] host: 1 = kept. */
int tsc_screen_mm_keeps(tsc_ctx *ctx, const float *D, int64_t n, double limit, uint8_t *keep, int32_t *limit_bits, float *out_scale);

/* Torsion-fingerprint pruning (tscode/numba_functions.py:142-264).
 * tsc_torsion_fingerprints: _get_tf_mat -- out f32[n_structs, n_quads] of dihedral angles in degrees (tscode/algebra.py:24-55)
 * over quads i32[n_quads, 4]; coords f64[n_structs, n_atoms, 3].
 * tsc_tfd_first_similar: the pair search of one pass (:171-199) over fingerprints tf f32[n_structs, n_quads]: chunk `step`
 * is [d*step, d*(step+1)), the last one [d*(k-1), num_active); first i32[n_structs] = absolute index of the first j > i of
 * i's chunk with tfd_similarity(tf[i], tf[j], thresh) (:242-253), or -1.  The graph step that turns the matches into
 * rejects (:201-226) is the caller's (tscode_amd/numba_functions.py keeps the reference's networkx objects). */
int tsc_torsion_fingerprints(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const int32_t *quads, int n_quads,
                             float *out);
int tsc_tfd_first_similar(tsc_ctx *ctx, const float *tf, int64_t n_structs, int n_quads, int64_t d, int64_t k, int64_t num_active,
                          double thresh, int32_t *first);

/* The same for many small ensembles per call (tscode/numba_functions.py:142-231, one run of the schedule :160-226 per segment).
 * tsc_tfd_batch_fingerprints_dev: _get_tf_mat (:233-240) of n_segments ensembles in one launch.  Segment s has n_structs[s]
 * structures of n_atoms[s] atoms at coords + offsets[s] (offsets i64[n_segments + 1] in doubles, offsets[0] = 0) and n_quads[s]
 * quadruplets, its own, back to back in quads i32[sum n_quads, 4]; n_structs[s] = 0 and n_quads[s] = 0 are allowed.  coords, quads
 * and the tables are host arrays; tf f32[tf_count] is DEVICE memory (tsc_malloc) and receives the segments' fingerprints back to
 * back, tf_count = sum n_structs[s] * n_quads[s], where they stay for every schedule slot.
 * tsc_tfd_batch_pass_dev: the pair search of one schedule slot (:171-199) in one launch, for the n_open segments whose gate (:166)
 * is open in it.  Entry q: n_structs[q] >= 1 fingerprints of n_quads[q] angles at tf + elem0[q], pass geometry d[q], k[q],
 * num_active[q] and thresh[q] as tsc_tfd_first_similar takes them, rows [row0[q], row0[q] + n_structs[q]) of first, ascending and
 * disjoint.  first i32[total_rows] (host): first[row0[q] + i] is what tsc_tfd_first_similar gives row i of that segment alone --
 * an index inside the segment -- and -1 for every row of no open segment.  A row never looks at a column of another segment.
 * An invalid entry refuses the whole call before any launch; tsc_last_error() names it. */
int tsc_tfd_batch_fingerprints_dev(tsc_ctx *ctx, const double *coords, const int64_t *offsets, const int32_t *n_structs,
                                   const int32_t *n_atoms, const int32_t *quads, const int32_t *n_quads, int64_t n_segments, float *tf,
                                   int64_t tf_count);
int tsc_tfd_batch_pass_dev(tsc_ctx *ctx, const float *tf, int64_t tf_count, const int64_t *elem0, const int64_t *row0,
                           const int32_t *n_structs, const int32_t *n_quads, const int64_t *d, const int64_t *k, const int64_t *num_active,
                           const double *thresh, int64_t n_open, int64_t total_rows, int32_t *first);

/* Moments of inertia and embed scores.
 * tsc_inertia_moments: tscode/algebra.py:165-186 get_inertia_moments for every structure -- out f64[n_structs, 3], the
 * eigenvalues of the inertia tensor about the centre of mass ordered by absolute value; masses f64[n_atoms].
 * tsc_moi_first_similar: the pair search of tscode/algebra.py:188-205 -- first i32[n_structs] = first j > i whose three moments
 * all differ by less than max_deviation relative to structure i's, or -1 (the graph step of prune_by_moment_of_inertia,
 * tscode/optimization_methods.py:341-358, is the caller's).
 * tsc_embed_scores: tscode/numba_functions.py:273-288 _score_embed_poses (scores f32[n_structs], float32 accumulation) and the
 * signed error of fitness_check (tscode/optimization_methods.py:544-557; fitness_error f64[n_structs]); indices i32[n_structs,
 * n_c, 2], distances f64[n_structs, n_c] (NaN = no target).  Host pointers. */
int tsc_inertia_moments(tsc_ctx *ctx, const double *structures, int64_t n_structs, int n_atoms, const double *masses, double *out);
int tsc_moi_first_similar(tsc_ctx *ctx, const double *moments, int64_t n_structs, double max_deviation, int32_t *first);

/* The same for many ensembles per call (tscode/optimization_methods.py:327-358, one prune_by_moment_of_inertia per segment).
 * Segment s has n_structs[s] >= 0 structures of n_atoms[s] >= 1 atoms at structures + offsets[s] (offsets i64[n_segments + 1] in
 * doubles, offsets[0] = 0) and its own masses, back to back in masses f64[sum n_atoms].  Host arrays.
 * tsc_inertia_moments_batch: out f64[sum n_structs, 3], per segment what tsc_inertia_moments gives it alone, bit for bit.
 * tsc_moi_first_similar_batch: moments f64[sum n_structs, 3] of the segments back to back; first i32[sum n_structs]: per row what
 * tsc_moi_first_similar gives the segment alone with max_deviation[s] -- an index INSIDE the segment, or -1.  A row never looks at
 * a column of another segment. */
int tsc_inertia_moments_batch(tsc_ctx *ctx, const double *structures, const int64_t *offsets, const int32_t *n_structs,
                              const int32_t *n_atoms, const double *masses, int64_t n_segments, double *out);
int tsc_moi_first_similar_batch(tsc_ctx *ctx, const double *moments, const int32_t *n_structs, const double *max_deviation,
                                int64_t n_segments, int32_t *first);
int tsc_embed_scores(tsc_ctx *ctx, const double *structures, int64_t n_structs, int n_atoms, const int32_t *indices,
                     const double *distances, int n_c, float *scores, double *fitness_error);

/* Pose parameters of the string embed (tscode/embeds.py:98-116), for n_sites (conformer pair, reactive-
 * centre pair) combinations x n_angles angles, pose = site * n_angles + angle index:
 *   R0 = rotation_matrix_from_vectors(mol_vec, -ref_vec) (:108, tscode/utils.py:183-208);
 *   R = rot_mat_from_pointer(ref_vec, angle) @ R0 when angle != 0 (:110-112);  t = p1 - R @ p2 (:114);
 * molecule 0 keeps identity / origin.  p1, p2, ref_vec, mol_vec f64[n_sites, 3]; conf_pair i32[n_sites, 2];
 * angles f64[n_angles] degrees; rot f64[N, 2, 9], pos f64[N, 2, 3], conf_idx i32[N, 2] -- the inputs of
 * tsc_transform_batch / tsc_embed_clash_mask_dev / tsc_pipeline_dev.  Host-pointer and device-pointer (_dev) forms. */
int tsc_string_embed_params(tsc_ctx *ctx, const double *p1, const double *p2, const double *ref_vec, const double *mol_vec,
                            const int32_t *conf_pair, int64_t n_sites, const double *angles, int n_angles, double *rot, double *pos,
                            int32_t *conf_idx);
int tsc_string_embed_params_dev(tsc_ctx *ctx, const double *p1, const double *p2, const double *ref_vec, const double *mol_vec,
                                const int32_t *conf_pair, int64_t n_sites, const double *angles, int n_angles, double *rot,
                                double *pos, int32_t *conf_idx);

/* Pose parameters of the cyclical embed (tscode/embeds.py:676-713), one row per (pose, molecule):
 * alignment = align_vec_pair([end - start, direction], [pivot, meanpoint - mean(reactive atoms)]) (tscode/algebra.py:258-282),
 * step = rot_mat_from_pointer(alignment @ (r0 - r1) or alignment @ pivot, angle), rotation = step @ alignment,
 * position = centre - step @ centre + mean(start, end) - alignment @ meanpoint with centre = alignment @ mean(reactive atoms).
 * start, end, direction, pivot, meanpoint, r0, r1 f64[n, 3] (r1 ignored where n_reactive is 1); n_reactive i32[n] (1 or 2);
 * angle f64[n] degrees; rot f64[n, 9], pos f64[n, 3].  Host pointers. */
int tsc_cyclical_embed_params(tsc_ctx *ctx, const double *start, const double *end, const double *direction, const double *pivot,
                              const double *meanpoint, const double *r0, const double *r1, const int32_t *n_reactive,
                              const double *angle, int64_t n, double *rot, double *pos);

/* Conformational-search rotations.  tsc_csearch_rotate builds every candidate of
 * tscode/torsion_module.py:463-500 from one start structure: for each torsion t with angles[m][t] != 0 the atoms of
 * masks[t] turn about the bond torsions[t][1]-torsions[t][2] (tscode/utils.py:389-414 rotate_dihedral, in place, in
 * torsion order), a rotation that fails tscode/numba_functions.py:26-47 torsion_comp_check is walked back in 5-degree
 * steps (angle // 5 of them, Python floor division) until it passes.  coords f64[n_atoms, 3]; torsions i32[n_tors, 4];
 * masks u8[n_tors, n_atoms] (tscode/torsion_module.py:301-325 _get_rotation_mask, computed by the caller);
 * angles i32[n_cand, n_tors] degrees; out f64[n_cand, n_atoms, 3]; rotated_bonds i32[n_cand] (the reference keeps a
 * candidate iff this is non-zero, :505).  tsc_torsion_comp_check: ok i32[n_structs] = 1 / 0 for structures sharing one
 * torsion and mask.  Host-pointer and device-pointer (_dev) forms. */
int tsc_csearch_rotate(tsc_ctx *ctx, const double *coords, int n_atoms, const int32_t *torsions, const uint8_t *masks, int n_tors,
                       const int32_t *angles, int64_t n_cand, double thresh, int64_t max_clashes, double *out, int32_t *rotated_bonds);
int tsc_csearch_rotate_dev(tsc_ctx *ctx, const double *coords, int n_atoms, const int32_t *torsions, const uint8_t *masks, int n_tors,
                           const int32_t *angles, int64_t n_cand, double thresh, int64_t max_clashes, double *out,
                           int32_t *rotated_bonds);
/* The same candidates from MANY start structures and torsion sets in one launch: the loop over starting_points of
 * clustered_csearch (tscode/torsion_module.py:736-780, every start x the group's whole angle table) and the one random_csearch
 * per TS candidate of Embedder.csearch_augmentation (tscode/embedder.py:1907-1939, each with its own torsions, masks and
 * shuffled table).  starts f64[n_starts, n_atoms, 3].  The n_sets torsion sets lie back to back: torsions i32[set_off[n_sets], 4],
 * masks u8[set_off[n_sets], n_atoms], set k owning rows set_off[k] .. set_off[k + 1]; start s uses set start_set[s].  One angle
 * table angles i32[n_rows, t_max]: a set's rows are zero-padded to t_max (a zero angle is skipped by the loop itself, :480 / :754).
 * Candidate m = (start cand_start[m], row cand_row[m]); the candidates of one start are contiguous and cand_start ascends.
 * out f64[n_cand, n_atoms, 3], rotated_bonds i32[n_cand].  The LDS bound of tsc_csearch_rotate holds per set.
 * tsc_csearch_multi_plan (host arrays, no device work) cuts the candidates into the kernel's work items, which never straddle two
 * sets: items i32[n_items, 4]; items == NULL only counts them.  The _dev form takes every array on the device except set_off (a
 * host array: it sizes the launch) and the items of the plan, uploaded by the caller; the host form plans by itself. */
int tsc_csearch_multi_plan(const int32_t *cand_start, int64_t n_cand, const int32_t *start_set, int n_starts, const int32_t *set_off,
                           int n_sets, int n_atoms, int32_t *items, int64_t items_cap, int64_t *n_items);
int tsc_csearch_rotate_multi(tsc_ctx *ctx, const double *starts, int n_starts, int n_atoms, const int32_t *torsions,
                             const uint8_t *masks, const int32_t *set_off, int n_sets, const int32_t *start_set, const int32_t *angles,
                             int64_t n_rows, int t_max, const int32_t *cand_start, const int32_t *cand_row, int64_t n_cand, double thresh,
                             int64_t max_clashes, double *out, int32_t *rotated_bonds);
int tsc_csearch_rotate_multi_dev(tsc_ctx *ctx, const double *starts, int n_atoms, const int32_t *torsions, const uint8_t *masks,
                                 const int32_t *set_off, int n_sets, const int32_t *angles, int t_max, const int32_t *cand_start,
                                 const int32_t *cand_row, int64_t n_cand, const int32_t *items, int64_t n_items, double thresh,
                                 int64_t max_clashes, double *out, int32_t *rotated_bonds);
/* Which candidates the reference appends, decided and compacted on the device (tscode/torsion_module.py:505-511; :779 for
 * n_out < 0).  One round of a search hands in, for each start still walking its table, ONE segment g = candidates
 * [seg_off[g], seg_off[g + 1]) of start seg_start[g] in table order, the first of them row seg_a0[g] of that start's table.  A row
 * is kept iff rotated_bonds != 0; only just after a row was kept is `len(new_structures) == n_out or a == max_tries` tested, so a
 * dropped row max_tries does not end the walk; n_out < 0 never stops on the count.  Carried per start from round to round:
 * kept_count i32[n_starts] and done i32[n_starts] (in / out; zero them before the first round; a start that is done takes
 * nothing); rows_consumed i32[n_starts] (out) = rows of the segment the loop walked.  kept_rows f64[capacity, n_atoms, 3] receives
 * the rows taken, in order, the segments back to back (segment g holds kept_count's increase of its start); *n_kept_host their
 * number (the call synchronises for it).  All arrays on the device. */
int tsc_csearch_select_dev(tsc_ctx *ctx, const double *cand, const int32_t *rotated_bonds, int n_atoms, const int32_t *seg_off,
                           const int32_t *seg_start, const int32_t *seg_a0, int n_seg, int n_out, int64_t max_tries, int32_t *kept_count,
                           int32_t *done, int32_t *rows_consumed, double *kept_rows, int64_t capacity, int64_t *n_kept_host);
/* tsc_rotate_dihedral: rotate_dihedral (tscode/utils.py:389-414) for n_structs structures f64[n_structs, n_atoms, 3] that share the
 * torsion (i1, i2, i3, i4) and the mask u8[n_atoms] of the atoms that move: structure s turns them by angles[s] degrees -- any real
 * number, tscode/torsion_module.py:984-1005 searches fractional corrections -- about its own i2 - i3 bond (centre i3).  No clash
 * check, no walk-back.  out f64[n_structs, n_atoms, 3] must not alias coords.  Host arrays. */
int tsc_rotate_dihedral(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const int32_t *torsion, const uint8_t *mask,
                        const double *angles, double *out);
int tsc_torsion_comp_check(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const int32_t *torsion,
                           const uint8_t *mask, double thresh, int64_t max_clashes, int32_t *ok);

/* Greedy per-group filter of the embed loops (tscode/embeds.py:715, :843): inside each group a pose is accepted iff
 * it is not similar (tscode/rmsd_pruning.py:208-224, all atoms, rmsd < thr and maxdev < 2 thr) to any pose accepted
 * before it in that group.  poses f64[n_poses, n_atoms, 3]; group g is poses[group_off[g] : group_off[g+1]]
 * (group_off i32[n_groups + 1], group sizes <= 8192); accepted u8[n_poses]. */
int tsc_greedy_group_filter(tsc_ctx *ctx, const double *poses, const int32_t *group_off, int n_groups, int n_atoms,
                            double rmsd_thr, uint8_t *accepted);
int tsc_greedy_group_filter_dev(tsc_ctx *ctx, const double *poses, const int32_t *group_off_dev, int n_groups, int64_t n_poses,
                                int n_atoms, double rmsd_thr, uint8_t *accepted);

/* The embed loops as one call each.  Both take HOST pointers, keep every intermediate on the device
 * (pose parameters, candidate poses, fingerprints) and return, per candidate in the reference's loop order, the
 * compenetration_check verdict (clash_ok u8[N]) and whether the reference would have appended the pose (kept u8[N]);
 * the kept poses themselves come back compacted in candidate order (poses f64[n_kept, n_atoms_total, 3]; poses may be
 * NULL; poses_capacity = rows the buffer holds, an error if fewer than n_kept).
 *
 * tsc_tfd_greedy_filter: is_new_structure (tscode/embeds.py:47-69) over a whole ordered list of torsion fingerprints
 *   tf f32[n, n_quads]: accepted[s] = 1 iff no fingerprint accepted before s is tfd_similar (tscode/numba_functions.py:242-253,
 *   sum of wrapped differences < thresh) to s's.  The reference's list never evicts (`lru_cache = lru_cache[1:]` rebinds a
 *   local, :66-67) and neither does this.
 *
 * tsc_string_embed: the loop of tscode/embeds.py:91-120.  Two fragments (frags / frag_off / n_atoms / n_conf as in
 *   tsc_transform_batch); n_sites rows (conformer pair, reactive-centre pair) in the reference's order and n_angles angles,
 *   candidate = site * n_angles + angle index (tsc_string_embed_params); compenetration_check(ids = the two fragments,
 *   thresh = clash_thresh, max_clashes) (:118); is_new_structure over the passing poses with the torsion fingerprints of
 *   quads i32[n_quads, 4] (atom indices in the embedded structure) and tfd_thresh (the reference uses 10) (:119).
 *
 * tsc_cyclical_embed: the inner loops of tscode/embeds.py:657-717 and :785-847 for any number of (conformers, pivots,
 *   polygon orientation) groups at once.  One row per (pose, molecule), row = pose * n_mols + m, with the inputs of
 *   tsc_cyclical_embed_params plus conf_idx i32[rows]; group_off i32[n_groups + 1] cuts the poses into the reference's
 *   `angular_poses` groups (consecutive, sizes <= 8192); compenetration_check (:714) and then, inside each group and in
 *   order, `not _rmsd_similarity(pose, kept poses of the group, rmsd_thr)` (:715; the reference passes 1). */
int tsc_tfd_greedy_filter(tsc_ctx *ctx, const float *tf, int64_t n_structs, int n_quads, double thresh, uint8_t *accepted,
                          int64_t *n_kept);
int tsc_string_embed(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf,
                     const double *p1, const double *p2, const double *ref_vec, const double *mol_vec, const int32_t *conf_pair,
                     int64_t n_sites, const double *angles, int n_angles, double clash_thresh, int64_t max_clashes,
                     const int32_t *quads, int n_quads, double tfd_thresh, uint8_t *clash_ok, uint8_t *kept, double *poses,
                     int64_t poses_capacity, int64_t *n_pass, int64_t *n_kept);
int tsc_cyclical_embed(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf,
                       int n_mols, const double *start, const double *end, const double *direction, const double *pivot,
                       const double *meanpoint, const double *r0, const double *r1, const int32_t *n_reactive, const double *angle,
                       const int32_t *conf_idx, int64_t n_poses, const int32_t *group_off, int n_groups, double clash_thresh,
                       int64_t max_clashes, double rmsd_thr, uint8_t *clash_ok, uint8_t *kept, double *poses, int64_t poses_capacity,
                       int64_t *n_pass, int64_t *n_kept);

/* tsc_cyclical_embed_groups: tsc_cyclical_embed (tscode/embeds.py:657-717 / :785-847) from ONE record per (group, molecule) instead
 *   of one per (pose, molecule) -- the form a multiembed (tscode/multiembed.py:26-82: one bimolecular cyclical embed per arrangement
 *   of facing atoms, all over the same two coordinate stacks) needs, where the rows would run into the millions.  start, end,
 *   direction, pivot, meanpoint, r0, r1 f64[n_groups * n_mols * 3] and n_reactive, conf_idx i32[n_groups * n_mols] at index
 *   group * n_mols + m; angles f64[n_angles * n_mols] is the one table of angle sets every group walks (systematic_angles, :665).
 *   Pose g * n_angles + a is record g under angle set a, and the groups are the records: exactly tsc_cyclical_embed on the rows
 *   expanded from them, group_off[g] = g * n_angles.  Outputs as tsc_cyclical_embed with n_poses = n_groups * n_angles.
 *   Checked before the device is touched, the message naming the group: 1 <= n_angles <= 8192, n_groups * n_angles < INT32_MAX,
 *   n_mols 2 or 3, n_reactive 1 or 2, conf_idx in range.  The alignment (align_vec_pair, :691-692) is computed once per
 *   (group, molecule) and not once per pose. */
int tsc_cyclical_embed_groups(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                              const int32_t *n_conf, int n_mols, const double *start, const double *end, const double *direction,
                              const double *pivot, const double *meanpoint, const double *r0, const double *r1,
                              const int32_t *n_reactive, const int32_t *conf_idx, const double *angles, int64_t n_groups, int n_angles,
                              double clash_thresh, int64_t max_clashes, double rmsd_thr, uint8_t *clash_ok, uint8_t *kept, double *poses,
                              int64_t poses_capacity, int64_t *n_pass, int64_t *n_kept);

/* tsc_trimolecular_groups: the records tsc_cyclical_embed_groups takes, for THREE molecules under RIGID, produced on the device.  Replaces
 *   the host loop over (pivot triple, orientation) of tscode/embeds.py:636-655 with _adjust_directions (tscode/embeds.py:312-465) inside it:
 *   per orientation three align_vec_pair, the 7 turns of -30 .. 30 degrees of six facing atoms, 343 candidates of three vec_angle each
 *   and their argmin (the first of the smallest), whose displacement vectors are the `directions` of the group AND the input of the triple's
 *   next orientation.  One wavefront per pivot triple; the orientations of a triple run in order.
 *   Fragments as in tsc_cyclical_embed_groups (frags / frag_off / n_atoms / n_conf, three of them).  Per molecule: reactive i32[3, 2]
 *   (n_reactive[m] = 1 or 2 of them used) and the rows (atom index, cumnum) of its reactive atoms, reactive_cumnums i64[sum n_rows, 2] with
 *   n_rows i32[3], each at most 8.  Per pivot triple t, decided on the host (no comparison of a rounded value is left to the device): conf
 *   i32[T, 3]; pivot, meanpoint f64[T, 3, 3]; cumnums i64[T, 3, 2] (start atom, end atom of the pivot); tri_poly f64[T, 3, 3] the
 *   triangle's vertices the polygon's sides are taken from (side m runs from vertex m to vertex m + 1, backwards where the orientation
 *   says so); tri_cost f64[T, 3, 3] the vertices the candidates are scored against (they differ from tri_poly where a right triangle was
 *   nudged, :287-293); directions f64[T, 3, 3] of _get_directions; mask u8[T], bit v set where orientation v is embedded (:642); base
 *   i64[T] the running count of mask bits in front of t.  The group of (t, v) is written at base[t] + (number of set bits of mask[t] below
 *   v): blocks f64[G, 3, 23] (start, end, direction, pivot, meanpoint, the reactive atoms of conformer conf -- the second a copy of the
 *   first where there is one --, their number, the conformer), group_ids i64[G, 3, 2] (the sorted cumnum pairs of the three contacts,
 *   :895-897) and best i32[G], the chosen candidate's row in cartesian_product(range(7), range(7), range(7)).  An orientation left out
 *   does not touch the directions.  A NaN cost is never chosen (all 343 NaN: candidate 0).
 *   TSC_ERR_INVALID before anything is launched, the message naming the triple: a null pointer, a conformer or atom index out of range,
 *   more than 8 table rows, a base that is not the running count or n_groups that is not its total, and -- for a triple with a
 *   non-empty mask -- a pivot cumnum that no molecule's reactive_cumnums holds.  n_triples = 0 succeeds and writes nothing.
 * tsc_trimolecular_groups_timings: under the context option "pass_timing" >= 1 the call times its kernel with events (and synchronises
 *   for it); *ms = that time for the calling thread's latest call, -1 where none was taken. */
int tsc_trimolecular_groups(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf,
                            const int32_t *reactive, const int32_t *n_reactive, const int64_t *reactive_cumnums, const int32_t *n_rows,
                            const int32_t *conf, const double *pivot, const double *meanpoint, const int64_t *cumnums, const double *tri_poly,
                            const double *tri_cost, const double *directions, const uint8_t *mask, const int64_t *base, int64_t n_triples,
                            int64_t n_groups, double *blocks, int64_t *group_ids, int32_t *best);
int tsc_trimolecular_groups_timings(tsc_ctx *ctx, float *ms);

/* HOST-side helper (no device, no context): the graph step of tscode/numba_functions.py:201-226 (prune_conformers_tfd) and
 * tscode/optimization_methods.py:341-358 (prune_by_moment_of_inertia) for any number of chunks: the matches (rel_i[q], rel_j[q]),
 * q in [chunk_ptr[c], chunk_ptr[c+1]), of chunk c are node indices relative to the chunk (0 <= index < chunk_len[c]), listed in the
 * order the reference adds them to its set (rows ascending); of every connected component of a chunk's match graph only
 * `tuple(subgraph.nodes)[0]` is kept: keep[chunk_off[c] + node] is cleared for the others (keep u8[n_total], set by the caller).
 * Which node that expression names is decided by CPython's set / dict iteration orders inside networkx 3.x; this call re-plays
 * them (tscode_amd/csrc/host_order.hpp).  The Python caller checks the emulation against the real objects before relying on it. */
int tsc_host_graph_step(const int64_t *rel_i, const int64_t *rel_j, const int64_t *chunk_ptr, const int64_t *chunk_off,
                        const int64_t *chunk_len, int64_t n_chunks, int64_t n_total, uint8_t *keep);

/* Per-pass statistics of a prune run (one entry per executed k of the schedule). */
typedef struct {
    int64_t k;               /* number of chunks (tscode/rmsd_pruning.py:186-188) */
    int64_t n_active_before; /* count_nonzero(mask) entering the pass */
    int64_t n_active_after;
    int64_t pairs_evaluated; /* pair evaluations the reference's sequential scan performs in this pass (:70) */
    int64_t pairs_computed;  /* pairs for which the GPU formed H = p^T q and ran the sign test */
    int64_t candidates;      /* pairs that reached the explicit-rotation path */
    int64_t pairs_screened;  /* pairs looked at by the descriptor sieve (0 when the register-tiled kernel ran) */
    int64_t new_keys;        /* cache keys appended (:76, :204) */
    double gpu_ms;           /* HIP-event time of the whole pass on this device (0 unless "pass_timing" is 2) */
    double tile_ms;          /* HIP-event time of the pass's pair kernel alone (0 unless "pass_timing" >= 1; chunk-local passes: 2) */
    int32_t algo;            /* kernel that ran the pass: 1 = register-tiled all-pairs, 2 = descriptor sieve, 3 = chunk-local kernel */
    int32_t nonfinite_input; /* 1: the run met a structure with a NaN or infinite coordinate (the same in every entry of a run; descriptor-sieve
                                runs only).  Such a structure is similar to nothing -- every comparison of :75 with a NaN is false -- and is
                                kept; the reference itself raises LinAlgError there (np.linalg.svd, :19), and so does the Python drop-in */
    int64_t pairs_known;     /* of pairs_screened: pairs inside the rows' ranges that the pass did NOT look at again -- an earlier pass of the run
                                found them dissimilar (switch skip_known, below).  pairs_screened - pairs_known is what the screen multiplied */
} tsc_pass_stats;

#define TSC_MAX_PASSES 18

/* prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on the heavy-atom array:
 *   heavy f64[n, h, 3] = structures[:, atomnos != 1]; rmsd_thr as in the reference (max deviation
 *   threshold is 2*rmsd_thr, :95);
 *   mode 0 = reference-exact, including the pair-cache behaviour of :65-67 / :75-77;
 *   mode 1 = cache-free (the cache test is skipped);
 *   mask u8[n] out (1 = kept); stats (optional) up to TSC_MAX_PASSES entries, n_passes out (optional).
 * For n > 200 000 the reference itself fails (a float k reaches range()); the schedule is used with int(k). */
int tsc_prune_rmsd(tsc_ctx *ctx, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask,
                   tsc_pass_stats *stats, int *n_passes);
/* The same from the arrays the reference's prune_conformers_rmsd receives (rmsd_pruning.py:164-206): structures f64[n, n_atoms, 3]
 * with ALL atoms in host memory and heavy_idx i32[n_heavy] (= flatnonzero(atomnos != 1), increasing): the gather of :178-179 runs on
 * the device. */
int tsc_prune_structures(tsc_ctx *ctx, const double *structures, int64_t n, int n_atoms, const int32_t *heavy_idx, int n_heavy,
                         double rmsd_thr, int mode, uint8_t *mask, tsc_pass_stats *stats, int *n_passes);
int tsc_prune_rmsd_dev(tsc_ctx *ctx, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask,
                       tsc_pass_stats *stats, int *n_passes); /* synchronises (the schedule gate reads counts) */

/* An embed-and-prune run: the cyclical embed of tsc_cyclical_embed_groups (tscode/embeds.py:657-717 / :785-847) whose kept poses go
 * straight into prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) without a trip through host memory.  By definition the result is
 * that of tsc_cyclical_embed_groups over all slabs followed by tsc_prune_structures on the poses it returned: the same flags, the same
 * verdicts and statistics, the same coordinates to the last bit.  The kept poses are never materialised on the host; the run keeps, per
 * kept pose, its heavy atoms (gathered from the very buffer the embed's filter read) and its 100-byte-per-molecule parameter row, prunes
 * the heavy atoms where they are and embeds again only the poses that are asked for -- recomputing a pose from its parameters is cheaper
 * than moving it, as in tsc_pipeline_dev.  Peak device memory: one slab's passing poses plus n_kept_total * (24 n_heavy + 100 n_mols)
 * bytes; the run's buffers grow by doubling.
 *   tsc_embed_prune_create      fragments as in tsc_cyclical_embed_groups (n_mols 2 or 3), uploaded ONCE for all slabs; heavy_idx
 *                               i32[n_heavy] = flatnonzero(atomnos != 1): at least one entry, increasing, below the atom count.
 *   tsc_embed_prune_add_groups  one slab of groups, arguments, checks and messages as tsc_cyclical_embed_groups (rmsd_thr_filter is its
 *                               rmsd_thr; N = n_groups * n_angles).  Only clash_ok u8[N], kept u8[N] and the two counts reach the host;
 *                               the slab's kept poses are appended to the run in candidate order.  May be called any number of times.
 *   tsc_embed_prune_count       kept poses so far, over all slabs.
 *   tsc_embed_prune_run         tsc_prune_rmsd_dev over the kept poses' heavy atoms: mode 0 or 1, survived u8[n_kept_total] (1 = the
 *                               pose outlives the prune), stats / n_passes (optional) as that call returns them.  With no kept pose it
 *                               launches nothing and reports no survivor.  Closes the run for further slabs; may be repeated (another
 *                               threshold), the latest verdicts are the ones that count.
 *   tsc_embed_prune_poses       which = 0: the survivors, which = 1: every kept pose; poses f64[rows, n_total, 3] in candidate order,
 *                               capacity = rows the buffer holds.  Embedded from the kept parameters by the kernel that embedded them
 *                               for the filter, and only these rows are fetched.
 *   tsc_embed_prune_destroy     frees the run ("objects created from a context", above).
 * Refused before the device is touched, with a message: a null pointer, n_heavy < 1, a heavy index out of range or not increasing, a
 * capacity below the row count, a mode other than 0 or 1 (TSC_ERR_INVALID); tsc_embed_prune_add_groups after tsc_embed_prune_run, and
 * tsc_embed_prune_poses with which = 0 before it (TSC_ERR_STATE).  The calls of one run must not overlap; they synchronise. */
typedef struct tsc_embed_prune tsc_embed_prune;
int tsc_embed_prune_create(tsc_ctx *ctx, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf,
                           int n_mols, const int32_t *heavy_idx, int n_heavy, tsc_embed_prune **run);
int tsc_embed_prune_add_groups(tsc_embed_prune *run, const double *start, const double *end, const double *direction,
                               const double *pivot, const double *meanpoint, const double *r0, const double *r1,
                               const int32_t *n_reactive, const int32_t *conf_idx, const double *angles, int64_t n_groups, int n_angles,
                               double clash_thresh, int64_t max_clashes, double rmsd_thr_filter, uint8_t *clash_ok, uint8_t *kept,
                               int64_t *n_pass, int64_t *n_kept);
int tsc_embed_prune_count(tsc_embed_prune *run, int64_t *n_kept_total);
int tsc_embed_prune_run(tsc_embed_prune *run, double rmsd_thr, int mode, uint8_t *survived, tsc_pass_stats *stats, int *n_passes,
                        int64_t *n_survived);
int tsc_embed_prune_poses(tsc_embed_prune *run, int which, double *poses, int64_t capacity);
int tsc_embed_prune_destroy(tsc_embed_prune *run);

/* Per-pass statistics of one segment of tsc_prune_rmsd_batch (one entry per executed k of that segment's schedule). */
typedef struct {
    int64_t k;               /* number of chunks (tscode/rmsd_pruning.py:186-188) */
    int64_t n_active_before; /* count_nonzero(mask) entering the pass (:192) */
    int64_t n_active_after;
    int64_t pairs_evaluated; /* pair evaluations the reference's sequential scan performs in this pass (:70): the columns a row visits up
                                to and including the one it stops at; columns the kernel computed beyond a row's stop are not counted */
    int64_t new_keys;        /* cache keys appended (:76, :204): one per removed row */
} tsc_batch_pass_stats;

#define TSC_PRUNE_BATCH_MAX_N 8192 /* the largest "prune_batch_max_n" */

/* prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206) on MANY ensembles in one launch: one run of :164-206 per segment, each with
 * its own schedule (:186-192), chunks (:136-144), cache (:183, :65-67, :204) and threshold, every one as tsc_prune_rmsd computes it.
 * One workgroup owns one segment for all its passes; the workgroups share nothing.
 *   heavy     f64: the segments' [n[s], h[s], 3] heavy-atom arrays (structures[:, atomnos != 1], :178-179) back to back;
 *   offsets   i64[n_segments + 1]: segment s starts at heavy + offsets[s] (in doubles); offsets[0] = 0 and
 *             offsets[s + 1] - offsets[s] = n[s] * h[s] * 3;
 *   n, h      i32[n_segments]: structures (>= 0, at most the context option "prune_batch_max_n") and heavy atoms (>= 1) per segment;
 *   thr       f64[n_segments]: rmsd_thr per segment (the max deviation threshold is 2 * thr, :95);  mode as in tsc_prune_rmsd;
 *   mask      u8[sum n] out (1 = kept), the segments back to back;
 *   stats     (optional) [n_segments][TSC_MAX_PASSES] out, zero beyond a segment's passes;  n_passes (optional) i32[n_segments] out;
 *   nonfinite (optional) u8[n_segments] out: 1 = the segment holds a structure with a NaN or infinite coordinate.  Such a structure
 *             is similar to nothing and is kept; the reference raises LinAlgError there (np.linalg.svd, :19), and so does the Python layer.
 * "prune_batch_max_n" (tsc_ctx_set_option; 1 .. 8192, default 2048): a longer segment is refused -- a workgroup is one compute unit, a long
 * ensemble belongs to tsc_prune_rmsd, which spreads a pass over the device (the Python layer routes it there).
 * The _dev form takes heavy, mask, stats, n_passes and nonfinite on the device and the four tables in host memory; it synchronises
 * (the tables are sorted into launch order and uploaded from the call's own memory). */
int tsc_prune_rmsd_batch(tsc_ctx *ctx, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr,
                         int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite);
int tsc_prune_rmsd_batch_dev(tsc_ctx *ctx, const double *heavy, const int64_t *offsets_host, const int32_t *n_host, const int32_t *h_host,
                             const double *thr_host, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                             int32_t *n_passes, uint8_t *nonfinite);

#define TSC_PRUNE_TEAM_MAX_N 200000 /* structures per segment that tsc_prune_rmsd_team takes at most: beyond it the reference itself fails */

/* The same runs of prune_conformers_rmsd (tscode/rmsd_pruning.py:164-206), one per segment, for MID-SIZE ensembles: a team of workgroups per
 * segment instead of one.  Schedule (:186-192), chunks (:136-144), cache (:183, :65-67, :204), verdicts and the non-finite rule are those
 * of tsc_prune_rmsd_batch, from the same device functions: masks and statistics are bit for bit the same.  A segment's state lives in
 * device memory; every schedule slot that some segment can take by its n alone costs two launches for the WHOLE batch (a workgroup per
 * segment closes the previous pass, decides the gate of :192 from the segment's own count and builds its cache view; then the rows of
 * all open segments, 16 per work item), so the number of launches depends on the longest segment, never on n_segments, and the host
 * waits once, at the end.
 * Arguments and outputs as tsc_prune_rmsd_batch, except that a segment may hold up to TSC_PRUNE_TEAM_MAX_N structures whatever
 * "prune_batch_max_n" says.  Refused before the device is touched, with the segment's index in the message (TSC_ERR_INVALID): a longer
 * segment, h < 1, n < 0, offsets that do not match n * h * 3, a threshold that is not finite; and a mode other than 0 or 1.  Segments of
 * 0 or 1 structures are legal.  The _dev form takes heavy, mask, stats, n_passes and nonfinite on the device and the four tables in host
 * memory; it synchronises (the tables are uploaded from the call's own memory). */
int tsc_prune_rmsd_team(tsc_ctx *ctx, const double *heavy, const int64_t *offsets, const int32_t *n, const int32_t *h, const double *thr,
                        int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats, int32_t *n_passes, uint8_t *nonfinite);
int tsc_prune_rmsd_team_dev(tsc_ctx *ctx, const double *heavy, const int64_t *offsets_host, const int32_t *n_host, const int32_t *h_host,
                            const double *thr_host, int64_t n_segments, int mode, uint8_t *mask, tsc_batch_pass_stats *stats,
                            int32_t *n_passes, uint8_t *nonfinite);

/* Stepping form of the same run, for one-process-per-GPU sharding of a pass (rows of a pass are
 * independent: tscode/rmsd_pruning.py:92,101-113).  Every rank holds the full `heavy` array and calls
 *   tsc_prune_create; loop { k = tsc_prune_next_pass; if k == 0 break;
 *                            tsc_prune_pass_local(rank, world);      // this rank's row tiles -> best[]
 *                            <all-reduce MIN over tsc_prune_best_ptr, n_active int32 entries>   (RCCL)
 *                            tsc_prune_pass_finish; }                 // identical mask/cache update on every rank
 *   tsc_prune_mask_dev gives the device mask; tsc_prune_destroy frees the state. */
/* A context serves at most 64 live runs at a time (each owns a word of the context's pinned memory; the 65th tsc_prune_create fails with
 * TSC_ERR_STATE).  tsc_prune_create / tsc_prune_destroy take the context's scratch cache: calls of them on ONE context must not overlap
 * (a context is for one thread at a time, see above); runs that exist may then be stepped from different threads.  tsc_prune_destroy and
 * what becomes of a run that outlives its context: "objects created from a context", above. */
int tsc_prune_create(tsc_ctx *ctx, const double *heavy_dev, int64_t n, int h, double rmsd_thr, int mode, tsc_prune **out);
int tsc_prune_next_pass(tsc_prune *p, int64_t *k_out);            /* 0 when the schedule is exhausted; does not wait:
                                                                      the gate of rmsd_pruning.py:192 is evaluated on the
                                                                      device, a pass whose gate is closed does nothing */
int tsc_prune_pass_estimate(tsc_prune *p, int64_t *pairs);        /* upper bound of the pairs of the open pass: lets every
                                                                      rank decide alike whether sharding it pays */
/* Runs every pass that needs no exchange (world == 1: all; world > 1: those with an estimate below min_pairs, computed whole by
 * every rank) and returns with the first pass that does left open (*k = its k) or *k = 0 at the end of the schedule
 * (rmsd_pruning.py:186-204).  One host call instead of three per small pass. */
int tsc_prune_run_replicated(tsc_prune *run, int world, int64_t min_pairs, int64_t *k);
int tsc_prune_pass_local(tsc_prune *p, int rank, int world_size); /* asynchronous -- except on a pass that MAY be culled (option "cull":
                                                                      at least "cull_min_pairs" pairs, fewer than 64 chunks), where the
                                                                      host waits once for the device's culled-or-walked verdict (the
                                                                      run's own word of pinned memory: runs of one context driven from
                                                                      different host threads do not share it); tsc_prune_pass_range
                                                                      likewise.  With world_size == 1 the verdicts are applied
                                                                      in here as well -- by the pair kernel itself, tile by tile
                                                                      (option "fused_apply"; best[] stays readable), or, for a pass
                                                                      whose chunks are short, by the chunk-local kernel (option
                                                                      "local_pass"; best[] is then not produced) -- and
                                                                      tsc_prune_pass_finish only does the host's bookkeeping */
int tsc_prune_pass_rows(tsc_prune *p, int rank, int world_size);  /* after tsc_prune_pass_local: the pair search of ANOTHER rank's row
                                                                     tiles of the same pass, into the same best[] (atomicMin).  Lets
                                                                     one GPU stand in for several ranks (tools/predict_scaling.py times
                                                                     every rank's share this way; repeating a share changes nothing) */
/* RANK-PARTITIONED passes ("early passes": whole chunks to GPUs).  The chunks of a pass are independent
 * (tscode/rmsd_pruning.py:139-157: every chunk reads the same input mask and the same cache), so while a pass has at least
 * min_chunks_per_rank chunks per rank each rank runs the WHOLE pass flow -- rows, stop columns, pair search, verdicts -- on the
 * chunks that start inside its block [n rank / world, n (rank + 1) / world) of the structure axis and on nothing else: no
 * per-row work is replicated, and what crosses the ranks is one bit per structure plus five counters.
 *   tsc_prune_exchange_words(n, mode) -> words of the exchange buffer (int64: n / 64 + 40 removed-row bits, 8 statistics, then --
 *                                mode 0 -- the storage of the run's cache views, which move into this buffer)
 *   tsc_prune_set_partition      right after tsc_prune_create; exch_dev = caller-owned device buffer of that many int64 (e.g. a
 *                                torch tensor that torch.distributed can all-reduce); zeroed here.  The per-pass exchange is over
 *                                its first n / 64 + 48 words
 *   per pass:  tsc_prune_next_pass;  tsc_prune_pass_partitioned -> 1:
 *                  tsc_prune_pass_range;                       // this rank's chunks, asynchronous
 *                  <all-reduce SUM over the exchange buffer>   // the ranks' bits are disjoint: the sum is their union
 *                  tsc_prune_pass_merge;                       // mask, bit copy, scan counts, record, the gate of :192, the next
 *                                                              // pass's rows -- identical on every rank; asynchronous
 *              -> 0: the first such pass after partitioned ones needs the cache keys of every rank (a key (a, b) is only ever
 *                  hit in the chunk that starts at a, which belongs to the same rank in every partitioned pass -- so the keys
 *                  stayed where they were made):  tsc_prune_views_ptr -> words > 0:  <all-reduce SUM over that block> (views_dev,
 *                  or exch_dev + offset_words: the views of the passes still to run), tsc_prune_views_merged;  then
 *                  tsc_prune_pass_local / tsc_prune_pass_finish as above.
 * The per-pass statistics of a partitioned pass (tsc_prune_stats) are the sums over all ranks. */
int tsc_prune_exchange_words(int64_t n, int mode, int64_t *words);
int tsc_prune_set_partition(tsc_prune *p, int rank, int world_size, int min_chunks_per_rank, void *exch_dev_i64, int64_t exch_words);
int tsc_prune_pass_partitioned(tsc_prune *p, int *flag);
int tsc_prune_pass_range(tsc_prune *p);
int tsc_prune_pass_merge(tsc_prune *p);
int tsc_prune_views_ptr(tsc_prune *p, void **views_dev_i64, int64_t *offset_words, int64_t *words);
int tsc_prune_views_merged(tsc_prune *p);
int tsc_prune_best_ptr(tsc_prune *p, void **best_dev, int64_t *n_entries); /* i32[n_entries], valid until finish */
/* Make the run keep best[] in a caller-owned device buffer of n int32 (e.g. a torch tensor that
 * torch.distributed can all-reduce); call right after tsc_prune_create. */
int tsc_prune_use_best_buffer(tsc_prune *p, void *best_dev_i32_n);
int tsc_prune_pass_finish(tsc_prune *p);                          /* asynchronous */

/* ---- the pass loop of a sharded run behind ONE call (the multi-rank variant of the prune) ----
 * tsc_prune_run_sharded walks the whole schedule of `run` as the step-by-step calls above would -- passes below `min_pairs` pairs whole
 * on every rank; passes with at least `min_chunks_per_rank` chunks per rank partitioned by chunks (0: never; needs the exchange buffer
 * exch_dev of tsc_prune_exchange_words words, which then also holds the cache views); the cache views summed once before the first pass
 * of the other kind; the remaining passes dealt by row tiles -- and calls back only for the collectives:
 *     exchange(user, kind, buf_dev, count)   reduce `count` elements at the DEVICE address buf_dev over all ranks, in place:
 *                                            TSC_XCHG_SUM_I64 = all-reduce SUM of int64 (removed-row bits and statistics of a partitioned
 *                                            pass; the cache views), TSC_XCHG_MIN_I32 = all-reduce MIN of int32 (best[] of a pass dealt
 *                                            by row tiles).  Everything the library enqueued before the call is on the context's stream:
 *                                            enqueue the collective on that stream (RCCL: ncclAllReduce(buf, buf, count, ncclInt64 /
 *                                            ncclInt32, ncclSum / ncclMin, comm, stream)) or synchronise around it.  Return 0; anything
 *                                            else aborts the run with TSC_ERR_STATE.
 * One process per GPU owns the communicator; the library opens none.  Every rank makes the same sequence of calls (it depends on n, k
 * and the world size only).  log (optional, log_cap entries): the exchanges made, in order -- k < 0 marks the one exchange of the cache
 * views in front of pass |k|.  With world == 1 the function is tsc_prune_run_replicated to the end (exchange may be NULL).
 * Afterwards: tsc_prune_copy_mask_dev / tsc_prune_stats / tsc_prune_destroy as usual.
 * tscode/rmsd_pruning.py:139-157 (chunks independent), :92,101-113 (rows independent). */
enum { TSC_XCHG_SUM_I64 = 1, TSC_XCHG_MIN_I32 = 2 };
typedef int (*tsc_exchange_fn)(void *user, int kind, void *buf_dev, int64_t count);
typedef struct tsc_exchange_record {
    int64_t k;      /* the pass (negative: the cache views in front of pass -k) */
    int32_t kind;   /* TSC_XCHG_* */
    int64_t count;  /* elements reduced */
} tsc_exchange_record;
int tsc_prune_run_sharded(tsc_prune *run, int rank, int world_size, int min_chunks_per_rank, int64_t min_pairs, void *exch_dev, int64_t exch_words,
                          tsc_exchange_fn exchange, void *user, tsc_exchange_record *log, int log_cap, int *n_log);
/* ---- the exchange inside the library (optional): a one-shot all-reduce over memory the ranks map into each other ----
 * For the small per-pass messages above a collective library's fixed cost (and, from a scripting host, a frame of the host language per
 * collective) is most of what an exchange costs.  A tsc_xchg gives every rank a receive area of FINE-GRAINED device memory that the other
 * ranks of the node map (hipIpcGetMemHandle / hipIpcOpenMemHandle): an exchange is then one kernel that writes this rank's contribution
 * into every peer and raises a flag there, and one that waits for the peers' flags and folds what they delivered into the caller's buffer
 * -- enqueued on the context's stream, no host in between.  The library still opens no communicator: the HOST carries the 64-byte
 * handles from rank to rank, once, over whatever it has (in this repository torch.distributed.all_gather_object).
 *   tsc_xchg_slot_bytes   bytes a slot must hold for runs over up to n structures (the largest message of tsc_prune_run_sharded)
 *   tsc_xchg_create       allocates the area (header + 2 x world slots of slot_bytes) and returns its IPC handle (TSC_XCHG_HANDLE_BYTES bytes)
 *   tsc_xchg_connect      handles = world x TSC_XCHG_HANDLE_BYTES bytes, in rank order (the own entry is ignored): maps the peers.  Call it on
 *                         every rank after all have created; ranks may share a device (other PROCESSES; tests do)
 *   tsc_xchg_allreduce    has the signature of tsc_exchange_fn with user = the tsc_xchg: pass it to tsc_prune_run_sharded as the exchange
 *                         function, or call it directly (buf 8-byte aligned; count elements of int64 / int32 as `kind` says)
 *   tsc_xchg_status       exchanges made so far and how many of them gave up waiting for a peer (tsc_xchg_set_timeout, default 5 s: a
 *                         rank that died must not hang the others' GPUs); after a timeout the reduced buffers are NOT valid -- check after
 *                         the run's synchronisation.  Every rank must make the same sequence of exchanges (tsc_prune_run_sharded does).
 *   tsc_xchg_destroy      unmaps the peers and frees the area ("objects created from a context", above)
 * What these messages are: tscode/rmsd_pruning.py:149-157 (disjoint out_mask[first:last] per chunk), :92,101-113 (rows independent). */
typedef struct tsc_xchg tsc_xchg;
#define TSC_XCHG_HANDLE_BYTES 64
int tsc_xchg_slot_bytes(int64_t n, int mode, int64_t *bytes);
int tsc_xchg_create(tsc_ctx *ctx, int rank, int world_size, int64_t slot_bytes, tsc_xchg **out, void *handle_out);
int tsc_xchg_connect(tsc_xchg *x, const void *handles);
int tsc_xchg_set_timeout(tsc_xchg *x, double seconds);
int tsc_xchg_allreduce(void *xchg, int kind, void *buf_dev, int64_t count);
int tsc_xchg_status(tsc_xchg *x, int64_t *n_exchanges, int *n_timeouts);
int tsc_xchg_destroy(tsc_xchg *x);
int tsc_prune_mask_dev(tsc_prune *p, const uint8_t **mask_dev);
int tsc_prune_copy_mask_dev(tsc_prune *p, uint8_t *dst_dev); /* dst[0..n) <- mask, asynchronous on the stream */
int tsc_prune_stats(tsc_prune *p, tsc_pass_stats *stats, int *n_passes); /* synchronises */
int tsc_prune_destroy(tsc_prune *p);

/* ---- whole pipeline on one device ----------------------------------------------------------------
 * generate -> clash-filter -> similarity-prune, the sequence RunEmbedding.run drives through
 * generate_candidates / compenetration_refining / similarity_refining (tscode/embedder.py:1136-1154,
 * 1230-1266, 1356-1368), with everything resident in HBM:
 *   K1+K2 fused verdicts, ordered compaction of the passing poses (all atoms + heavy atoms), K3 prune.
 * Inputs as tsc_transform_batch_dev plus heavy_idx (indices of atoms with atomnos != 1).
 * Outputs (device, caller-allocated for the worst case n_poses):
 *   clash_mask u8[n_poses]; structures f64[n_pass, n_atoms, 3] (poses that pass the clash check, in order);
 *   keep_mask u8[n_pass] (prune verdict on those); keep_mask_host (optional, host, n_poses bytes) receives a copy of
 *   keep_mask[0 .. n_pass) before the call returns; n_pass_host / n_keep_host scalars on the host.
 * timings_ms (optional, host) float[4] = {embed+clash, compaction, prune, total} from HIP events.
 * HOST COST: the call returns after ONE synchronisation at its end, but in the middle it needs the number of poses that passed the clash
 * check to size the prune (the schedule depends on it).  The scan kernel writes that count into the context's pinned memory and the calling
 * thread SPINS on it (a pause instruction per look: x86; about 40 us per call at 100k poses -- the clash kernel + the scan -- with a fall-back
 * to a copy + synchronise after 5 s): a host core per context is busy for that long in every call.  A caller that keeps several contexts in
 * flight from one thread each pays it per context. */
int tsc_pipeline_dev(tsc_ctx *ctx, const double *frags, const int64_t *frag_off_host, const int32_t *n_atoms_host,
                     const int32_t *n_conf_host, int n_mols, const int32_t *conf_idx, const double *rot, const double *pos,
                     int64_t n_poses, const int32_t *heavy_idx_host, int n_heavy, double clash_thresh, int64_t max_clashes,
                     double rmsd_thr, int mode, uint8_t *clash_mask, double *structures, uint8_t *keep_mask,
                     uint8_t *keep_mask_host, int64_t *n_pass_host, int64_t *n_keep_host, tsc_pass_stats *stats, int *n_passes,
                     float *timings_ms);


/* Symmetry-corrected RMSD pruning (tscode/torsion_module.py:953-1161, prune_conformers_rmsd_rot_corr).
 * The set-up is the caller's (the graph work of :1023-1049, once per call): coords f64[n_structs, n_atoms, 3] centred on their
 * all-atom mean; heavy i32[n_heavy] the heavy atoms; torsions i32[n_tors, 4] the dummy torsions as the reference orients them;
 * angles f64[n_tors, 6] with n_angles i32[n_tors] (1..6) used per row, in the reference's order (0 included); move_mask
 * u8[n_tors, n_atoms] the atoms each torsion turns (_get_rotation_mask); torsion t's local heavy subgraph is
 * sub_idx[sub_ptr[t] .. sub_ptr[t+1]) (sub_ptr i32[n_tors + 1], sub_ptr[0] = 0, every subgraph non-empty).
 * Limits, refused with TSC_ERR_INVALID: n_tors <= 16, n_atoms <= 512, n_structs < 2^31.  Host arrays throughout.
 *   tsc_rot_corr_begin    uploads the set-up and the structures; the run turns ITS copy in place, as the reference turns its array.
 *   tsc_rot_corr_pass     one pass of the schedule (:1080-1152 without the graph step): chunk `step` is [d*step, d*(step+1)), the
 *                         last one [d*(k-1), num_active); rows of a chunk in order, each row's j in order up to and including the
 *                         first similar one (rmsd < max_rmsd), pairs found dissimilar in an earlier pass skipped (the cache).
 *                         first i32[n_structs] = absolute index of row i's first similar j, or -1; pairs_evaluated = the pairs the
 *                         reference would have computed in this pass.  Synchronous.
 *   tsc_rot_corr_end      copies the run's (centred, turned) structures to coords_out f64[n_structs, n_atoms, 3].
 *   tsc_rot_corr_destroy  frees the run ("objects created from a context", above).
 *   tsc_rot_corr_pairs    the value-level form: rotationally_corrected_rmsd(ref = coords[pairs[p, 0]], coord = coords[pairs[p, 1]])
 *                         for every pair on a private copy of the coordinates (nothing is mutated): rmsd f64[n_pairs] and the best
 *                         angle of every torsion, best_angle f64[n_pairs, n_tors]. */
int tsc_rot_corr_begin(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const int32_t *heavy, int n_heavy,
                       const int32_t *torsions, int n_tors, const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                       const int32_t *sub_ptr, const int32_t *sub_idx, tsc_rot_corr **out);
int tsc_rot_corr_pass(tsc_rot_corr *run, int64_t d, int64_t k, int64_t num_active, double max_rmsd, int32_t *first,
                      int64_t *pairs_evaluated);
int tsc_rot_corr_end(tsc_rot_corr *run, double *coords_out);
int tsc_rot_corr_destroy(tsc_rot_corr *run);
int tsc_rot_corr_pairs(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const int32_t *heavy, int n_heavy,
                       const int32_t *torsions, int n_tors, const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                       const int32_t *sub_ptr, const int32_t *sub_idx, const int32_t *pairs, int64_t n_pairs, double *rmsd,
                       double *best_angle);

/* The symmetry-corrected prune of many ensembles per run (tscode/torsion_module.py:1013-1161, one schedule :1076-1152 per segment,
 * walked in lockstep by the caller).  Every segment is an ensemble of its own molecule: segment s has n_structs[s] structures of
 * n_atoms[s] atoms at coords + offsets[s] (offsets i64[n_segments + 1] in doubles, offsets[0] = 0), centred as tsc_rot_corr_begin
 * takes them, and its own set-up in the layout of tsc_rot_corr_begin, the segments' arrays back to back: heavy i32[sum n_heavy],
 * torsions i32[sum n_tors, 4], angles f64[sum n_tors, 6], n_angles i32[sum n_tors], move_mask u8[sum n_tors[s] * n_atoms[s]],
 * sub_ptr i32[sum (n_tors + 1)] (each segment's own, starting at 0), sub_idx i32[sum of the segments' sub_ptr[n_tors]].  The limits
 * of tsc_rot_corr_begin hold per segment and are checked on the host arrays before anything touches the device; tsc_last_error()
 * names the segment.  Host arrays throughout.
 *   tsc_rot_corr_batch_begin    uploads every segment's set-up and structures and zeroes the caches of dissimilar pairs (:1121-1123).
 *   tsc_rot_corr_batch_pass     one schedule slot in ONE launch for the n_open segments open[q] (ascending) whose gate (:1083) is
 *                               open in it: chunk geometry d[q], num_active[q] and threshold max_rmsd[q] their own, k shared.  One
 *                               workgroup per chunk of each open segment walks its rows as tsc_rot_corr_pass does.  first
 *                               i32[sum n_structs]: per row of an open segment what tsc_rot_corr_pass gives the segment alone, as an
 *                               index INSIDE the segment; -1 for every other row.  pairs_evaluated i64[n_open].  Synchronous.
 *   tsc_rot_corr_batch_end      copies the structures as the passes left them to coords_out f64[offsets[n_segments]].
 *   tsc_rot_corr_batch_destroy  frees the run ("objects created from a context", above). */
int tsc_rot_corr_batch_begin(tsc_ctx *ctx, const double *coords, const int64_t *offsets, const int32_t *n_structs,
                             const int32_t *n_atoms, const int32_t *heavy, const int32_t *n_heavy, const int32_t *torsions,
                             const int32_t *n_tors, const double *angles, const int32_t *n_angles, const uint8_t *move_mask,
                             const int32_t *sub_ptr, const int32_t *sub_idx, int64_t n_segments, tsc_rot_corr_batch **out);
int tsc_rot_corr_batch_pass(tsc_rot_corr_batch *run, const int32_t *open, const int64_t *d, int64_t k, const int64_t *num_active,
                            const double *max_rmsd, int64_t n_open, int32_t *first, int64_t *pairs_evaluated);
int tsc_rot_corr_batch_end(tsc_rot_corr_batch *run, double *coords_out);
int tsc_rot_corr_batch_destroy(tsc_rot_corr_batch *run);

/* Ensemble alignment, k-means and the diverse-conformer pick: the end of a conformational search (tscode/torsion_module.py:849-924,
 * most_diverse_conformers; csrc/diverse.hpp).  Host arrays throughout; fp64; every sum in a fixed order, so two calls on the same
 * input return the same bits.  Limits, refused with TSC_ERR_INVALID before any launch: 1 <= k <= 300 (the reference's own gate,
 * :863), k <= N, n_atoms <= 512 (D <= 1536), N < 2^31.
 *   tsc_align_structures  align_structures (tscode/hypermolecule_class.py:38-72): every structure is centred on the mean of its
 *                         indexed atoms (:53-55; indices NULL or n_idx == 0: all atoms, :51) and structures 1 .. N-1 are turned by the
 *                         proper rotation that takes their indexed atoms onto structure 0's (rmsd's kabsch at :63, applied at :70).
 *                         The LinAlgError branch (:65-67) has no counterpart: the solver (Horn's quaternion, csrc/pair_math.hpp) does not
 *                         fail; where the optimum is not unique the result is finite and a proper rotation.  out f64[N, n, 3].
 *   tsc_kmeans_lloyd      what KMeans(n_clusters = k, init = <array>, n_init = 1, algorithm = "lloyd").fit(X) computes (:889-890 with
 *                         the initial centres given): X f64[N, D] and init f64[k, D] are mean-centred, tol_abs = mean(var(X, 0)) * tol;
 *                         per iteration: nearest centre (ties: the lowest), per-cluster means, the j-th empty cluster (ascending)
 *                         takes the row with the j-th largest distance to its own centre (ties: the lower row), which leaves its
 *                         cluster's sum; stop when the labels repeat or the squared shift of the centres <= tol_abs, else after
 *                         max_iter; unless the labels repeated, one more assignment.  labels i32[N], centers f64[k, D] (mean added
 *                         back), *inertia = sum |x_i - centre|^2, *n_iter, *max_empty (optional) = the most clusters empty at once.
 *   tsc_kmeans_seed       k-means++ without local trials, the uniforms u f64[k] in [0, 1) given by the caller (the library has no
 *                         random numbers): rows[0] = floor(u[0] N); then rows[j] = the first row whose running sum (row order) of
 *                         min_d2 = squared distance to the nearest seed so far exceeds u[j] * total.
 *   tsc_diverse_pick      :894-922 on aligned f64[N, n, 3], labels i32[N] in [0, k), centers f64[k, n, 3]: picked[c] = the member of
 *                         cluster c to keep, -1 for an empty cluster.  With energies f64[N]: the lowest energy, the first in row
 *                         order on a tie (:901).  Without: the largest cumdist, the first on a tie (:919-921), where the member at
 *                         position p of its cluster's list sums |centre_c[a] - member[a]| over the atoms and over the centres
 *                         c != p -- the position, as :919 has it (`enumerate(cluster)`), not the member's own cluster.
 *   tsc_diverse_select    :882-922 in one call, nothing but the loop control leaving the device in between: align (all atoms), Lloyd
 *                         from the aligned rows init_rows, pick.  u == NULL: init_rows i32[k] is read.  u f64[k] given: the seeds
 *                         are chosen on the aligned features by the rule of tsc_kmeans_seed and init_rows RECEIVES them.
 *                         aligned_out f64[N, n, 3], labels i32[N], picked i32[k], *n_iter.
 *   tsc_diverse_timings   under the context option "pass_timing" >= 1 the calls above time their stages with events (and synchronise
 *                         for it): ms4 = align, first k_kmeans_assign launch (the kernel alone), first k_kmeans_update launch, device part
 *                         of tsc_diverse_select, of the calling thread's latest call of one of the entries above (each resets all four);
 *                         -1 where that call took none.
 * Non-finite coordinates / X / init / centers, NaN energies and u outside [0, 1) are refused with TSC_ERR_INVALID before any launch. */
int tsc_align_structures(tsc_ctx *ctx, const double *structures, int64_t n_structs, int n_atoms, const int32_t *indices, int n_idx,
                         double *out);
int tsc_kmeans_lloyd(tsc_ctx *ctx, const double *X, int64_t N, int64_t D, const double *init, int k, int max_iter, double tol,
                     int32_t *labels, double *centers, double *inertia, int *n_iter, int *max_empty);
int tsc_kmeans_seed(tsc_ctx *ctx, const double *X, int64_t N, int64_t D, int k, const double *u, int32_t *rows);
int tsc_diverse_pick(tsc_ctx *ctx, const double *aligned, int64_t N, int n_atoms, const int32_t *labels, const double *centers, int k,
                     const double *energies, int32_t *picked);
int tsc_diverse_select(tsc_ctx *ctx, const double *structures, int64_t N, int n_atoms, int32_t *init_rows, const double *u, int k,
                       const double *energies, int max_iter, double tol, double *aligned_out, int32_t *labels, int32_t *picked,
                       int *n_iter);
int tsc_diverse_timings(tsc_ctx *ctx, float *ms4);

/* tsc_diverse_select for many small ensembles per call (csrc/diverse_batch.hpp; tscode/torsion_module.py:882-922 per segment).
 * Segment s has n_structs[s] structures of n_atoms[s] atoms at structures + offsets[s] (offsets i64[n_segments + 1] in doubles,
 * offsets[0] = 0) and k[s] clusters; the limits per segment are tsc_diverse_select's.  flags u8[n_segments]: bit 0 = the segment
 * has energies, at energies + (the sum of n_structs before it) in energies f64[sum n_structs] (may be NULL when no segment has
 * any); bit 1 = its initial centres are k-means++ seeds from u + (the sum of k before it) in u f64[sum k] (may be NULL when no
 * segment is seeded), and its part of init_rows i32[sum k] RECEIVES them; otherwise that part is read.  max_iter and tol hold
 * for every segment.  Outputs, segment after segment: aligned_out f64 like structures, labels i32[sum n_structs], picked i32[sum
 * k] (-1 for an empty cluster), n_iter i32[n_segments].
 * Each segment's results are those of tsc_diverse_select on it alone, bit for bit: the segmented kernels call the same device
 * functions on the segment's own grid, so every sum keeps its fixed order.  Each segment stops by the single call's rule (:889-890
 * as tsc_kmeans_lloyd states it), decided on the device; the host reads one 8-byte record per iteration for the whole batch, and
 * the workgroups of a finished segment return at once.  Seeding takes one pair of launches per seed index for all segments that
 * still need it.  An invalid segment refuses the whole call before any launch; tsc_last_error() names the segment. */
int tsc_diverse_select_batch(tsc_ctx *ctx, const double *structures, const int64_t *offsets, const int32_t *n_structs,
                             const int32_t *n_atoms, const int32_t *k, int64_t n_segments, int32_t *init_rows, const double *u,
                             const double *energies, const uint8_t *flags, int max_iter, double tol, double *aligned_out,
                             int32_t *labels, int32_t *picked, int32_t *n_iter);

/* Bond graphs from distances and their difference to an expected graph, for a whole ensemble per call (csrc/topology.hpp): the
 * topology test the reference applies to every structure that survives the embed and prune steps.
 *   replaces   graphize                 tscode/graph_manipulations.py:33-55 (d_min_bond :28-29)
 *              molecule_check           tscode/utils.py:341-353
 *              scramble_check           tscode/utils.py:355-387
 *              get_double_bonds_indices tscode/utils.py:293-314 (the same scan with another threshold table)
 * Atoms i < j of a structure are BONDED iff both are active and sqrt(dx dx + dy dy + dz dz) < thr[class_i][class_j], in fp64 with the
 * reference's roundings (the kernel compares dx dx + dy dy + dz dz, formed without fused multiply-add, with the smallest double whose
 * square root reaches the threshold: the same verdict).  A threshold of 0 means "never bonded".  The self loops graphize puts on the
 * diagonal are not formed here: only the strict upper triangle is, and every consumer of the reference drops a == b.
 *   coords      f64[n_structs, n_atoms, 3]; n_atoms 1 .. 512.  Non-finite coordinates are not refused: such an atom is bonded to nothing.
 *   atom_class  u8[n_atoms], each < n_classes (1 .. 16): the ensemble shares its elements, so a threshold depends on the class pair only.
 *   thr         f64[n_classes, n_classes], finite and >= 0; read as given (the caller makes it symmetric).
 *   active      u8[n_atoms] or NULL (all): graphize's mask.
 *   ref_bits    u64[n_atoms, W], W = ceil(n_atoms / 64), or NULL (no bonds): the expected bonds, bit (j & 63) of word j >> 6 of row i for
 *               i < j; bits outside the strict upper triangle are refused.  Expected bonds that touch an inactive atom count as broken.
 *   excluded    atoms whose pairs are not counted: i32[n_excl] shared by all structures (excl_per_struct == 0) or
 *               i32[n_structs, n_excl] (excl_per_struct != 0); -1 = unused slot; n_excl 0 .. 16.
 *   care(i, j)  = i < j and neither atom excluded.  formed = #{care & bonded & ~ref}, broken = #{care & ~bonded & ref},
 *   mask[s]     = formed + broken <= max_newbonds.  mask u8[n_structs] is always written; formed i32[n_structs], broken i32[n_structs]
 *               and adj u64[n_structs, n_atoms, W] (the bonds found, laid out as ref_bits, excluded atoms included) where given.
 * tsc_bond_delta takes host arrays.  tsc_bond_delta_dev: coords, excluded (when per structure), mask, formed, broken and adj are device
 * pointers, the small tables host pointers; a per-structure excluded index outside 0 .. n_atoms-1 cannot be refused there and is an unused
 * slot; the call is enqueued on the context's stream and, when ref_bits is given, waits for it.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 512, n_classes outside 1 .. 16, a class
 * >= n_classes, a negative or non-finite threshold, n_excl > 16, an excluded index >= n_atoms or < -1 (host arrays).  n_structs == 0
 * succeeds and writes nothing.
 *   tsc_topology_timings  under the context option "pass_timing" >= 1 the two calls time their kernel with events (and synchronise for
 *                         it): *ms = that time for the calling thread's latest call, -1 where it took none. */
int tsc_bond_delta(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr,
                   int n_classes, const uint8_t *active, const uint64_t *ref_bits, const int32_t *excluded, int n_excl,
                   int excl_per_struct, int64_t max_newbonds, uint8_t *mask, int32_t *formed, int32_t *broken, uint64_t *adj);
int tsc_bond_delta_dev(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr,
                       int n_classes, const uint8_t *active, const uint64_t *ref_bits, const int32_t *excluded, int n_excl,
                       int excl_per_struct, int64_t max_newbonds, uint8_t *mask, int32_t *formed, int32_t *broken, uint64_t *adj);
int tsc_topology_timings(tsc_ctx *ctx, float *ms);

/* Non-covalent interactions of a whole ensemble per call (csrc/nci.hpp), one wavefront per structure.
 *   replaces   get_nci                  tscode/nci.py:28-52, called once per structure from print_nci (tscode/embedder.py:2053-2096)
 *              _get_nci_atomic_pairs    tscode/nci.py:54-89
 *              _get_nci_aromatic_rings  tscode/nci.py:91-139
 *              _get_aromatic_centers    tscode/nci.py:141-181, with is_phenyl (tscode/graph_manipulations.py:152-174) and dihedral
 *                                       (tscode/algebra.py:24-56): the walk over every combination of 6 of a molecule's C/N atoms is
 *                                       replaced by the enumeration of the 6-cliques of the graph "distance not above 3 A"
 * The result equals the reference's, quirks included.  All distances in fp64 with the reference's roundings (dx dx + dy dy + dz dz without
 * fused multiply-add, compared with the squared bound that gives the verdict of sqrt-then-compare); a threshold of 0 means "never".
 *   1 pairs      i1 ascending, i2 ascending over the atoms of every LATER molecule; neither atom constrained; hit iff
 *                dist < thr[class_i1][class_i2], strictly.
 *   2 rings      per molecule in order, every 6-combination of its ring candidates in lexicographic order of atom index: a ring iff no
 *                pair distance is above 3 A and the dihedral of its four LOWEST atoms has 1 - |cos| < 1 - cos(10 deg); atan2(0, 0) = 0 is
 *                flat, a NaN dihedral is not a ring.  Centre = the mean of the six atoms, owner = the molecule.
 *   3 ring-atom  every ring in list order against every atom of the WHOLE system: hit iff dist(centre, atom) < ring_thr[class_atom] and the
 *                owner rule lets the pair through.  owner_rule 0 (the reference as written, nci.py:100-105, where the atom's owner is always
 *                0): the ring's molecule is not molecule 0 -- a ring's own atoms included, rings of molecule 0 never.  owner_rule 1 (what
 *                the comment at :105-106 intends): the atom's molecule is not the ring's.  Constrained atoms are NOT excluded here.
 *   4 ring-ring  rings r < s in list order with different owners: hit iff dist(centre_r, centre_s) < ring_ring_thr.
 *   coords          f64[n_structs, n_atoms, 3]; n_atoms 1 .. 512.  DEVIATION: non-finite coordinates are not refused here (the Python
 *                   layer refuses them); such an atom takes part in no pair and no ring, where the reference's is_phenyl would let a NaN
 *                   distance pass (np.max(...) > 3 is False for NaN).
 *   atom_class      u8[n_atoms], each < n_classes (1 .. 8); thr f64[n_classes, n_classes] and ring_thr f64[n_classes], finite and >= 0.
 *   atom_mol        u8[n_atoms]: the molecule of every atom; non-decreasing from 0 to n_mols - 1 in steps of at most 1 (n_mols 1 .. 8).
 *   ring_candidate  u8[n_atoms]: non-zero for the C / N atoms; at most 64 per molecule.  Molecules with fewer than 6 are not scanned.
 *   constrained     i32[n_con] shared by all structures (con_per_struct == 0) or i32[n_structs, n_con]; -1 = unused slot; n_con 0 .. 16.
 *   counts          i32[n_structs, 4]: pairs, rings, ring-atom hits, ring-ring hits.  Always written, as is
 *   overflow        u8[n_structs]: 1 where a structure has more than 64 rings.  The ring count stays exact; the lists below hold the first
 *                   64 rings in order, and the ring-atom / ring-ring counts cover those.
 *   optional (NULL: not wanted), slots behind the last ring zero:
 *   pair_bits       u64[n_structs, n_atoms, W], W = ceil(n_atoms / 64): bit (i2 & 63) of word i2 >> 6 of row i1, laid out as adj of tsc_bond_delta
 *   ring_atoms      u16[n_structs, 64, 6] ascending atom indices;  ring_owner u8[n_structs, 64];  ring_center f64[n_structs, 64, 3]
 *   ring_atom_bits  u64[n_structs, 64, W]: the atoms hit by ring r;  ring_ring_bits u64[n_structs, 64]: bit s of word r for a hit r < s
 * tsc_nci takes host arrays.  tsc_nci_dev: coords, constrained (when per structure) and every output are device pointers, the small tables
 * host pointers; a per-structure constrained index outside 0 .. n_atoms-1 cannot be refused there and is an unused slot; the call is
 * enqueued on the context's stream and does not wait for it.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 512, n_classes outside 1 .. 8, n_mols
 * outside 1 .. 8, a class >= n_classes, molecule indices that are not contiguous blocks in order, more than 64 candidates in a molecule,
 * a negative or non-finite threshold, n_con > 16, a constrained index >= n_atoms or < -1 (host arrays), an owner rule other than 0 / 1.
 * n_structs == 0 succeeds and writes nothing.
 *   tsc_nci_timings  under the context option "pass_timing" >= 1 the two calls time their kernel with events (and synchronise for it):
 *                    *ms = that time for the calling thread's latest call, -1 where it took none. */
int tsc_nci(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr, int n_classes,
            const uint8_t *atom_mol, int n_mols, const uint8_t *ring_candidate, const double *ring_thr, double ring_ring_thr,
            const int32_t *constrained, int n_con, int con_per_struct, int owner_rule, int32_t *counts, uint8_t *overflow,
            uint64_t *pair_bits, uint16_t *ring_atoms, uint8_t *ring_owner, double *ring_center, uint64_t *ring_atom_bits,
            uint64_t *ring_ring_bits);
int tsc_nci_dev(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr,
                int n_classes, const uint8_t *atom_mol, int n_mols, const uint8_t *ring_candidate, const double *ring_thr,
                double ring_ring_thr, const int32_t *constrained, int n_con, int con_per_struct, int owner_rule, int32_t *counts,
                uint8_t *overflow, uint64_t *pair_bits, uint16_t *ring_atoms, uint8_t *ring_owner, double *ring_center,
                uint64_t *ring_atom_bits, uint64_t *ring_ring_bits);
int tsc_nci_timings(tsc_ctx *ctx, float *ms);

/* Reactive-atom orbitals and pivots of every conformer of one molecule per call (csrc/orbitals.hpp), one lane per conformer: what the embed
 * drivers take as input (tsc_string_embed: centres and orbital vectors; tsc_cyclical_embed: pivots), from coordinates.
 *   replaces   Hypermolecule.compute_orbitals   tscode/hypermolecule_class.py:195-217 (the loop over conformers and reactive atoms, :212-214)
 *              Single / Sp2 / Sp3 / Ether / Ketone / Imine / Sp_or_carbene / Metal .init(update=True)
 *                                               tscode/reactive_atoms_classes.py:34-80, :88-119, :127-207, :253-284, :293-375, :383-416,
 *                                               :425-538, :546-576, with rot_mat_from_pointer, norm, norm_of, vec_angle (tscode/algebra.py)
 *              is_sigmatropic                   tscode/graph_manipulations.py:231-273 -- its test per conformer (:256); the rest comes in as a mode
 *              Embedder._get_pivots             tscode/embedder.py:575-621, with Pivot (tscode/hypermolecule_class.py:388-402)
 *              Embedder._set_pivots             tscode/embedder.py:542-573 (the suprafacial and sigma-star filters)
 * Everything the reference reads from the bond graph (of conformer 0: hypermolecule_class.py:185) comes in a RECIPE per reactive atom, built
 * on the host once (tscode_amd/reactive_atoms.py: orbital_recipes).  tsc_orbital_recipe, field by field:
 *   cls           TSC_ORB_SINGLE .. TSC_ORB_METAL: the class get_atom_type picked (reactive_atoms_classes.py:645-660)
 *   flags         TSC_ORB_F_SIGMASTAR    mol.sp3_sigmastar (is_vicinal, graph_manipulations.py:275-298): the same in every recipe of a call
 *                 TSC_ORB_F_BOND_LENGTH  Single without a parameter: orb_dim is this conformer's |atom - nb[0]| (:77) and the field orb_dim is not read
 *                 TSC_ORB_F_ALLENE / TSC_ORB_F_KETENE   Sp_or_carbene (:448-482): where a conformer is 'sp', pivot1 comes from ex[0], ex[1]
 *                 TSC_ORB_F_KETONE_KETENE / _TWO / _TRILOBE   Ketone: its neighbour has 1 / 2 / 3 other neighbours (:322, :342, :360); one of them is required
 *   atom          the reactive atom
 *   nb[4]         its neighbours in ascending index, as many as the class reads: Single 1 (`other`), Sp2 3, Ether 2, Ketone 1, Imine 2,
 *                 Sp_or_carbene 2, Metal 1, Sp3 0; -1 = unused
 *   ex[4]         Single / Sp3 under sigmastar: {the bonded reactive partner, Single: the first neighbour of the partner that is not `atom` (:60-62);
 *                                 Sp3: the first neighbour of `atom` that is not the partner (:187-189)}
 *                 Sp3 otherwise: {the leaving group (:141-170)}
 *                 Ketone KETENE: {the neighbour's other neighbour, that atom's first other neighbour (:325-329)};  TWO: {a1, a2 (:346-347)};
 *                 TRILOBE: {the three (:363)}
 *                 Sp_or_carbene ALLENE: {the first other neighbour of nb[0], nb[0] (:507-508)};  KETENE: {substituent, ketene atom (:471-479)}
 *                 Metal: {neighbors(graph, nb[0])[0] (:561) -- the metal itself where it has the lowest index there: NaN, as in the reference}
 *   reserved      0
 *   orb_dim       the lobe distance (orb_dim_dict, the DIST keyword, _scale_orbs); for Sp_or_carbene that of 'sp'
 *   orb_dim_bent  Sp_or_carbene: that of 'bent carbene' (the key depends on the conformer, :486)
 *   seed[3]       Sp_or_carbene: stands for np.random.rand(3) of :495, read where a conformer is 'sp' and neither flag is set
 * Per conformer c:
 *   sigmatropic[c]  sigmatropic_mode 0: 0;  1 (two reactive atoms): |atom_0 - atom_1| < 3 A (:256);  2: 1 (an explicit override; the only way to
 *                   the Ketone 'p' lobes of :350-353, which compute_orbitals cannot reach: str() of a Ketone is never in sp2_types)
 *   centers, orb_vecs f64[n_conf, n_reactive, 4, 3]   the class's .center and .orb_vecs, unused lobes zero;  n_lobes u8[n_conf, n_reactive]
 *   kind u8[n_conf, n_reactive]   TSC_ORB_KIND_*: what str(r_atom) names -- 'sp' iff abs(vec_angle - 180) < 5 (:439-446), the Ketone subtype
 *   pivots (one or two reactive atoms; all four arrays or none), in the order of cartesian_product (first lobe index fastest; one reactive atom:
 *   the lobe pairs i < j), after the suprafacial filter (only where a conformer has exactly 4 pivots, embedder.py:552-563) and the sigma-star
 *   filter (lengths within 1e-5 of the shortest, :569-573):
 *   pivot, meanpoint f64[n_conf, 16, 3];  lobe_index i8[n_conf, 16, 2];  n_pivots u8[n_conf];  slots behind the last: 0 and -1
 * Coordinates are used as given (the reference has subtracted the ensemble's centroid, hypermolecule_class.py:179-184).  fp64 throughout; the
 * three decisions per conformer (angle, distance, pivot lengths) are taken on values that may differ from the reference's in the last bits.
 * tsc_orbitals takes host arrays.  tsc_orbitals_dev: coords and every output are device pointers, the recipes a host pointer; the call is
 * enqueued on the context's stream and does not wait for it.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 65536, n_reactive outside 1 .. 8, an unknown class
 * or flag bit, a Ketone without subtype, an atom / neighbour / extra index the class reads outside 0 .. n_atoms-1, a non-finite orb_dim or seed,
 * recipes that disagree on TSC_ORB_F_SIGMASTAR, sigmatropic_mode outside 0 .. 2 or 1 without exactly two reactive atoms, some but not all of the
 * four pivot arrays, pivot arrays with more than two reactive atoms.  n_conf == 0 succeeds and writes nothing.
 *   tsc_orbitals_timings  under the context option "pass_timing" >= 1 the two calls time their kernel with events (and synchronise for it):
 *                         *ms = that time for the calling thread's latest call, -1 where it took none. */
#define TSC_ORB_MAX_REACTIVE 8
#define TSC_ORB_MAX_LOBES 4
#define TSC_ORB_MAX_PIVOTS 16
#define TSC_ORB_MAX_ATOMS 65536
enum { TSC_ORB_SINGLE = 0, TSC_ORB_SP2 = 1, TSC_ORB_SP3 = 2, TSC_ORB_ETHER = 3, TSC_ORB_KETONE = 4, TSC_ORB_IMINE = 5, TSC_ORB_SP_OR_CARBENE = 6,
       TSC_ORB_METAL = 7 };
enum { TSC_ORB_F_SIGMASTAR = 1, TSC_ORB_F_BOND_LENGTH = 2, TSC_ORB_F_ALLENE = 4, TSC_ORB_F_KETENE = 8, TSC_ORB_F_KETONE_KETENE = 16,
       TSC_ORB_F_KETONE_TWO = 32, TSC_ORB_F_KETONE_TRILOBE = 48, TSC_ORB_F_KETONE_MASK = 48, TSC_ORB_F_ALL = 63 };
enum { TSC_ORB_KIND_SINGLE = 0, TSC_ORB_KIND_SP2 = 1, TSC_ORB_KIND_SP3 = 2, TSC_ORB_KIND_ETHER = 3, TSC_ORB_KIND_KETONE_PP = 4,
       TSC_ORB_KIND_KETONE_SP2 = 5, TSC_ORB_KIND_KETONE_P = 6, TSC_ORB_KIND_KETONE_TRILOBE = 7, TSC_ORB_KIND_IMINE = 8, TSC_ORB_KIND_SP = 9,
       TSC_ORB_KIND_BENT_CARBENE = 10, TSC_ORB_KIND_METAL = 11 };
typedef struct tsc_orbital_recipe {
    int32_t cls, flags, atom;
    int32_t nb[4];
    int32_t ex[4];
    int32_t reserved;
    double orb_dim, orb_dim_bent;
    double seed[3];
} tsc_orbital_recipe;
int tsc_orbitals(tsc_ctx *ctx, const double *coords, int64_t n_conf, int n_atoms, const tsc_orbital_recipe *recipes, int n_reactive,
                 int sigmatropic_mode, int suprafacial, double *centers, double *orb_vecs, uint8_t *n_lobes, uint8_t *kind, uint8_t *sigmatropic,
                 double *pivot, double *meanpoint, int8_t *lobe_index, uint8_t *n_pivots);
int tsc_orbitals_dev(tsc_ctx *ctx, const double *coords, int64_t n_conf, int n_atoms, const tsc_orbital_recipe *recipes, int n_reactive,
                     int sigmatropic_mode, int suprafacial, double *centers, double *orb_vecs, uint8_t *n_lobes, uint8_t *kind,
                     uint8_t *sigmatropic, double *pivot, double *meanpoint, int8_t *lobe_index, uint8_t *n_pivots);
int tsc_orbitals_timings(tsc_ctx *ctx, float *ms);

/* Hydrogen bonds and the search graph of a conformational search, for a whole ensemble per call (csrc/torsions.hpp), one wavefront
 * per structure.
 *   replaces   _get_hydrogen_bonds      tscode/torsion_module.py:233-299 (fragments=None, or the connected components of the graph)
 *              the graph set-up and the segmentation verdict of csearch, tscode/torsion_module.py:559-606
 * The search graph starts as bonds U extra.  The NEIGHBOUR LIST of an atom is its bonded atoms in ascending index, then its partners
 * from `extra` in the order of `extra`; an edge that already exists keeps its first position.
 * Hetero pairs (i1 < i2, in index order) QUALIFY iff d_min < sqrt(dx dx + dy dy + dz dz) < d_max, both strictly, in fp64 with the
 * reference's roundings (dx dx + dy dy + dz dz formed without fused multiply-add and compared with the squared bounds that give the
 * verdicts of sqrt-then-compare).  The candidate hydrogens of a pair are the hydrogen neighbours of i1 in list order, then those of i2.
 * With u = (r_i2 - r_i1) / |r_i2 - r_i1|, v1 = r_H - r_i1, v2 = r_H - r_i2: alfa is the angle between v1 and u when v1.u < v2.(-u), else
 * the angle between v2 and -u (degrees, arccos of the clipped dot product of the two normalised vectors).  The FIRST hydrogen with
 * alfa < max_angle ends the pair's search and appends the sorted pair (H, i2) when |v1| < |v2|, else (H, i1).  Output order: by hetero
 * pair, i1 then i2.
 *   mode 0 (keep_hb=True)   every hetero pair is searched.
 *   mode 1 (keep_hb=False)  a search only where bonds U extra has more than one connected component, and then only of the pairs whose two
 *                           hetero atoms lie in different components (:593).
 * The pairs found are then added as edges.  status[s] = 1 (segmented: the reference raises SegmentedGraphError) iff the graph still has
 * more than one component -- which covers mode 1 with a segmented graph and no pair found -- else 0.
 *   coords      f64[n_structs, n_atoms, 3]; n_atoms 1 .. 512.  Non-finite coordinates are not refused: such an atom is in no pair.
 *   hetero      u8[n_atoms]: non-zero for N and O.  hydrogen u8[n_atoms]: non-zero for H.  No atom may carry both.
 *   bonds       u64[n_structs, n_atoms, W], W = ceil(n_atoms / 64): the strict upper triangle as tsc_bond_delta writes adj; bits at or
 *               left of the diagonal and behind the last atom are ignored.
 *   extra       i32[n_structs, n_extra, 2] or NULL with n_extra == 0 (0 .. 64): the constraint pairs; a pair that holds -1, or twice the
 *               same atom, is an unused slot.
 *   hb          i32[n_structs, max_hb, 2]: the pairs, lower index first.  n_hb i32[n_structs]: the TRUE count; where it exceeds max_hb the
 *               first max_hb pairs were written and the caller calls again with more slots.  Nothing is written behind slot max_hb - 1;
 *               the host-array form returns -1 in the slots behind a structure's pairs, the _dev form leaves them as they were.
 *   status      u8[n_structs].  Optional (NULL: not wanted): n_components_before i32[n_structs] (of bonds U extra) and graph
 *               u64[n_structs, n_atoms, W], the strict upper triangle of bonds U extra U hb (all pairs found, also those behind max_hb).
 * tsc_hbonds takes host arrays.  tsc_hbonds_dev: coords, bonds, extra and every output are device pointers, hetero and hydrogen host
 * pointers; an extra index outside -1 .. n_atoms-1 cannot be refused there and makes its pair an unused slot; the call is enqueued on the
 * context's stream.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 512, n_extra outside 0 .. 64,
 * max_hb < 0, a mode other than 0 and 1, an atom flagged both ways, an extra index >= n_atoms or < -1 (host arrays), a non-finite
 * threshold, d_min >= d_max.  n_structs == 0 succeeds and writes nothing.
 *
 * Three reachability answers per (search graph, candidate torsion) (csrc/torsions.hpp), TOR_CHUNK torsions of one graph per wavefront.
 *   replaces   Torsion.in_cycle         tscode/torsion_module.py:54-61   (nx.has_path)
 *              Torsion.sort_torsion     tscode/torsion_module.py:120-132 (one nx.has_path per constrained atom)
 *              _get_rotation_mask       tscode/torsion_module.py:301-325 (nx.shortest_path)
 * Per graph g and torsion (i1, i2, i3, i4) of torsions[set_off[g] .. set_off[g+1]), every search in the graph WITHOUT the edge i2 - i3:
 *   in_cycle  = i4 is reachable from i1.
 *   reversed  = an ODD number of entries of constrained[g] (duplicates counted) are reachable from i2: the reference reverses the tuple
 *               once per reachable entry and always tests from the original i2.
 *   mask      with (a, b, c, _) the tuple after that reversal: the atoms reachable from a; inverted over the n_atoms atoms when more than
 *               n_atoms / 2 (integer division) are; then mask[b] = 0.
 *   graph        u64[n_graphs, n_atoms, W], laid out as above.
 *   torsions     i32[T_total, 4]; set_off i32[n_graphs + 1] ascending from 0 -- a HOST pointer in both forms.
 *   constrained  i32[n_graphs, n_con] or NULL with n_con == 0; -1 = unused slot.
 *   flags        u8[T_total]: bit 0 in_cycle, bit 1 reversed.  masks u8[T_total, n_atoms], zero where in_cycle.
 * tsc_torsion_reach takes host arrays.  tsc_torsion_reach_dev: graph, torsions, constrained, flags and masks are device pointers; a
 * torsion that the host form would refuse gets flags 0x80 and a zero mask there, a constrained entry outside 0 .. n_atoms-1 is an unused
 * slot; the call waits for the stream.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 512, n_graphs < 0, n_con < 0, a set_off
 * that does not start at 0 or decreases, and (host arrays) a torsion index outside 0 .. n_atoms-1, i2 == i3, a constrained entry
 * >= n_atoms or < -1.  n_graphs == 0 or T_total == 0 succeeds and writes nothing.
 *   tsc_torsions_timings  under the context option "pass_timing" >= 1 the calls time their kernel with events (and synchronise for it):
 *                         ms2[0] = the hydrogen-bond kernel, ms2[1] = the reachability kernel of the calling thread's latest calls, -1
 *                         where none was taken. */
int tsc_hbonds(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *hetero, const uint8_t *hydrogen,
               const uint64_t *bonds, const int32_t *extra, int n_extra, double d_min, double d_max, double max_angle, int mode, int max_hb,
               int32_t *hb, int32_t *n_hb, uint8_t *status, int32_t *n_components_before, uint64_t *graph);
int tsc_hbonds_dev(tsc_ctx *ctx, const double *coords, int64_t n_structs, int n_atoms, const uint8_t *hetero, const uint8_t *hydrogen,
                   const uint64_t *bonds, const int32_t *extra, int n_extra, double d_min, double d_max, double max_angle, int mode,
                   int max_hb, int32_t *hb, int32_t *n_hb, uint8_t *status, int32_t *n_components_before, uint64_t *graph);
int tsc_torsion_reach(tsc_ctx *ctx, const uint64_t *graph, int n_graphs, int n_atoms, const int32_t *torsions, const int32_t *set_off,
                      const int32_t *constrained, int n_con, uint8_t *flags, uint8_t *masks);
int tsc_torsion_reach_dev(tsc_ctx *ctx, const uint64_t *graph, int n_graphs, int n_atoms, const int32_t *torsions, const int32_t *set_off,
                          const int32_t *constrained, int n_con, uint8_t *flags, uint8_t *masks);
int tsc_torsions_timings(tsc_ctx *ctx, float *ms2);

/* Which torsions of a structure turn together in a clustered conformational search, for a whole ensemble per call (csrc/torsions.hpp),
 * one wavefront per structure.
 *   replaces   _group_torsions_dbscan   tscode/torsion_module.py:373-397 (scikit-learn's dbscan with min_samples=1, level after level)
 *              the T < 9 branch of clustered_csearch, tscode/torsion_module.py:689-695
 * Per structure s with T = set_off[s+1] - set_off[s] torsions (i1, i2, i3, i4):
 *   T < min_torsions (9 in the reference): one group -- group_of 0 for every torsion, n_groups 1 (0 where T == 0), eps_index -1,
 *   oversize 0.  Otherwise:
 *   centre    of torsion t = (r_i2 + r_i3) / 2 in fp64 (:379).
 *   linked    at a level eps: two torsions whose centres have dx dx + dy dy + dz dz <= eps eps, inclusive, in fp64 without fused
 *             multiply-add (every level is a multiple of 0.5: its square is exact).
 *   clusters  the connected components of that relation; a cluster's label is the rank of its smallest member among the clusters'
 *             smallest members (dbscan with min_samples=1: every point is a core point, clusters are numbered as they are met).
 *   levels    10.0, 9.5, ..., 2.0 (np.arange(10, 1.5, -0.5), seventeen), in that order: the first whose largest cluster has at most
 *             max_size members (5 in the reference, 3 with ff_opt) is kept and eps_index is its position.  No level qualifies (the
 *             reference's loop has no else): the clusters of the last level stand, eps_index = 16, oversize = 1.
 *   order     the groups are the clusters by size ascending, ties by label (sorted(output, key=len), :394, a stable sort);
 *             group_of[t] is the position of t's cluster in that order.  Inside a group the torsions keep ascending index.
 *   coords      f64[n_structs, n_atoms, 3]; n_atoms 1 .. 512.  A torsion with a non-finite centre is linked to nothing.
 *   torsions    i32[T_total, 4]; set_off i32[n_structs + 1] ascending from 0 -- a HOST pointer in both forms; at most 512 torsions per
 *               structure.
 *   group_of    i32[T_total].  n_groups, eps_index i32[n_structs].  oversize u8[n_structs].
 * tsc_torsion_groups takes host arrays.  tsc_torsion_groups_dev: coords, torsions and the four outputs are device pointers; a torsion
 * with i2 or i3 outside 0 .. n_atoms-1, which the host form refuses, has no centre there and is linked to nothing; the call waits for
 * the stream.
 * Refused with TSC_ERR_INVALID before any launch: null required pointers, n_atoms outside 1 .. 512, n_structs < 0, max_size < 1, a
 * set_off that does not start at 0 or decreases, more than 512 torsions in a structure, and (host arrays) a torsion index outside
 * 0 .. n_atoms-1.  n_structs == 0 or T_total == 0 succeeds and writes nothing.
 *   tsc_torsion_groups_timings  under the context option "pass_timing" >= 1: *ms = the kernel of the calling thread's latest call, -1
 *                               where none was taken. */
int tsc_torsion_groups(tsc_ctx *ctx, const double *coords, int n_structs, int n_atoms, const int32_t *torsions, const int32_t *set_off,
                       int max_size, int min_torsions, int32_t *group_of, int32_t *n_groups, int32_t *eps_index, uint8_t *oversize);
int tsc_torsion_groups_dev(tsc_ctx *ctx, const double *coords, int n_structs, int n_atoms, const int32_t *torsions, const int32_t *set_off,
                           int max_size, int min_torsions, int32_t *group_of, int32_t *n_groups, int32_t *eps_index, uint8_t *oversize);
int tsc_torsion_groups_timings(tsc_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* TSCODE_HIP_H */
