// prune.hip -- K3: prune_conformers_rmsd -- the run, its passes, the sharded protocol
// gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "call.hpp"
#include "prune_host.hpp"
#include "cull_layout.hpp"
#include "mm_kernels.hpp"
#include "rmsd.hpp"
#include "descriptor_kernels.hpp"
#include "describe.hpp"
#include "descriptor_basis.hpp"

// --------------------------------------------------------------------------------------------------
// K3: pairs

namespace tsc {
inline __global__ __launch_bounds__(256) void k_rmsd_pairs(const double *__restrict__ heavy, int h, const int32_t *__restrict__ pairs,
                                                     int64_t n_pairs, double *__restrict__ rmsd, double *__restrict__ maxdev) {
    for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n_pairs; k += int64_t(gridDim.x) * blockDim.x) {
        double r, m;
        rmsd_and_max_pair(heavy + int64_t(pairs[2 * k]) * h * 3, heavy + int64_t(pairs[2 * k + 1]) * h * 3, h, r, m);
        rmsd[k] = r;
        maxdev[k] = m;
    }
}
}  // namespace tsc

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_pairs_dev(tsc_ctx *c, const double *heavy, int64_t n_structs, int h, const int32_t *pairs, int64_t n_pairs,
                                  double *rmsd, double *maxdev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && heavy && pairs && rmsd && maxdev, "tsc_rmsd_pairs_dev: null argument");
    TSC_REQUIRE(n_structs >= 0 && h > 0 && n_pairs >= 0, "bad sizes");
    if (n_pairs == 0) return 0;
    DeviceGuard guard(c->device);
    hipLaunchKernelGGL(k_rmsd_pairs, dim3(grid_for(n_pairs, 256)), dim3(256), 0, c->stream, heavy, h, pairs, n_pairs, rmsd, maxdev);
    TSC_HIP(hipGetLastError());
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_pairs(tsc_ctx *c, const double *heavy, int64_t n_structs, int h, const int32_t *pairs, int64_t n_pairs,
                              double *rmsd, double *maxdev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && heavy && pairs && rmsd && maxdev, "tsc_rmsd_pairs: null argument");
    TSC_REQUIRE(n_structs >= 0 && h > 0 && n_pairs >= 0, "bad sizes");
    for (int64_t k = 0; k < 2 * n_pairs; ++k)
        TSC_REQUIRE(pairs[k] >= 0 && pairs[k] < n_structs, "pairs[%lld] = %d out of range", (long long)k, pairs[k]);
    if (n_pairs == 0) return 0;
    HostCall call(c);
    double *d_heavy, *d_r, *d_m;
    int32_t *d_pairs;
    TSC_TRY(call.in(heavy, size_t(n_structs) * h * 3, &d_heavy));
    TSC_TRY(call.in(pairs, size_t(n_pairs) * 2, &d_pairs));
    TSC_TRY(call.out(rmsd, size_t(n_pairs), &d_r));
    TSC_TRY(call.out(maxdev, size_t(n_pairs), &d_m));
    TSC_TRY(tsc_rmsd_pairs_dev(c, d_heavy, n_structs, h, d_pairs, n_pairs, d_r, d_m));
    return call.finish();
    TSC_API_GUARD_END
}

// The two test entry points of the matrix-core screen share everything but the dump kernel: the run's largest |component| from the host's
// descriptors, their records through k_mm_records, then S f32[2, 64, n] (k_mm_screen_dump) or keep u8[64, n] (k_mm_screen_keeps).
static int screen_mm_dump(tsc_ctx *c, const char *who, const float *D, int64_t n, double limit, float *S, uint8_t *keep, int32_t *limit_bits, float *out_scale) {
    TSC_REQUIRE(c && D && (S || keep) && limit_bits && out_scale, "%s: null argument", who);
    TSC_REQUIRE(n >= 1 && n <= (1 << 20), "n = %lld not supported", (long long)n);
    float dmax = 0.0f;
    for (int64_t e = 0; e < n * DW; ++e) dmax = std::fabs(D[e]) > dmax || std::isnan(D[e]) ? (std::isnan(D[e]) ? NAN : std::fabs(D[e])) : dmax;
    unsigned bits;   // (uploaded from here: declared in front of the call, which waits for the stream before it goes)
    memcpy(&bits, &dmax, sizeof(bits));
    if (std::isnan(dmax)) bits = NONFINITE_BITS;
    HostCall call(c);
    float *d_D, *d_S;
    uint8_t *d_keep;
    unsigned *d_bits;
    int32_t *d_lim;
    _Float16 *d_rec;
    TSC_TRY(call.in(D, size_t(n) * DW, &d_D));
    TSC_TRY(call.in(&bits, 1, &d_bits));
    TSC_TRY(call.scratch().get(size_t(n) * MM_REC_HALVES, &d_rec));
    TSC_TRY(call.out(S, size_t(NFAM) * MM_ROWS * n, &d_S));
    TSC_TRY(call.out(keep, size_t(MM_ROWS) * n, &d_keep));
    TSC_TRY(call.out(limit_bits, 1, &d_lim));
    hipLaunchKernelGGL(k_mm_records, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const float *)d_D, n, (const unsigned *)d_bits, d_rec);
    const dim3 grid(unsigned(ceil_div<int64_t>(n, MM_STEP)));
    if (S) hipLaunchKernelGGL(k_mm_screen_dump, grid, dim3(64), 0, c->stream, (const _Float16 *)d_rec, int(n), (const unsigned *)d_bits, limit, d_S, d_lim);
    else hipLaunchKernelGGL(k_mm_screen_keeps, grid, dim3(64), 0, c->stream, (const _Float16 *)d_rec, int(n), (const unsigned *)d_bits, limit, d_keep, d_lim);
    TSC_HIP(hipGetLastError());
    TSC_TRY(call.finish());
    *out_scale = mm_scale(bits);
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_screen_mm_values(tsc_ctx *c, const float *D, int64_t n, double limit, float *S, int32_t *limit_bits,
                                                                           float *out_scale) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(S, "tsc_screen_mm_values: null argument");
    return screen_mm_dump(c, "tsc_screen_mm_values", D, n, limit, S, nullptr, limit_bits, out_scale);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_screen_mm_keeps(tsc_ctx *c, const float *D, int64_t n, double limit, uint8_t *keep, int32_t *limit_bits,
                                                                          float *out_scale) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(keep, "tsc_screen_mm_keeps: null argument");
    return screen_mm_dump(c, "tsc_screen_mm_keeps", D, n, limit, nullptr, keep, limit_bits, out_scale);
    TSC_API_GUARD_END
}

// What tsc_prune_destroy and tsc_ctx_destroy undo beside the run's blocks.  In one critical section with the unlisting: the run's word of
// pinned memory and its hold on the descriptors it borrowed (tsc_prune_create).
void tsc_prune::unlisted() {
    if (borrows_xd && ctx->xd_borrowers > 0) --ctx->xd_borrowers;
    if (flag_slot >= 0) ctx->flag_slots_used &= ~(1ull << flag_slot);
}
tsc_prune::~tsc_prune() {
    for (auto &slot : ev)
        for (hipEvent_t e : slot)
            if (e) ctx->event_pool.push_back(e);
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_destroy(tsc_prune *p) {
    TSC_API_GUARD_BEGIN
    return destroy_owned(p);   // (without a wait for the stream: owned.hpp, destroy_waits)
    TSC_API_GUARD_END
}


// d_moments (optional): moment_doubles(h) doubles already zeroed on `st` by the caller; otherwise taken from `s` and cleared here
int build_basis(tsc_ctx *c, hipStream_t st, Scratch &s, const double *heavy, int h, int n_samples, int64_t stride, double *d_Q,
                       unsigned *zero_word, double *d_moments, double *spread_host) {
    const int nf[NFAM] = {n_features(h, 0), n_features(h, 1)};
    const size_t q_doubles = size_t(KD) * (nf[0] + nf[1]);
    double *d_M[NFAM], *d_zero;
    // the moment matrices of both families in one block (one memset)
    const size_t m0 = size_t(MOM_BLOCKS) * (nf[0] + 1) * (nf[0] + 1), m1 = size_t(MOM_BLOCKS) * (nf[1] + 1) * (nf[1] + 1);
    if (d_moments) {
        d_zero = d_moments;
    } else {
        TSC_TRY(s.get(m0 + m1 + 1, &d_zero));
        // (the arrival counters of the deterministic form -- its partial matrices are written whole --, or the matrices the fast form adds into)
        if (c->opt.deterministic_basis) TSC_HIP(hipMemsetAsync(d_zero + m0 + m1, 0, sizeof(double), st));
        else TSC_HIP(hipMemsetAsync(d_zero, 0, (m0 + m1 + 1) * sizeof(double), st));
    }
    d_M[0] = d_zero, d_M[1] = d_zero + m0;
    {
        const size_t lds = size_t(32) * (std::max(nf[0], nf[1]) + 1) * sizeof(double);
        if (lds > 64 * 1024)
            TSC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_feature_moments), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        if (c->opt.deterministic_basis)
            hipLaunchKernelGGL(k_feature_moments, dim3(MOM_BLOCKS, NFAM), dim3(256), lds, st, heavy, h, nf[0], nf[1], stride, n_samples, d_M[0], d_M[1],
                               reinterpret_cast<unsigned *>(d_zero + m0 + m1));
        else
            hipLaunchKernelGGL(k_feature_moments, dim3(ceil_div(n_samples, 32), NFAM), dim3(256), lds, st, heavy, h, nf[0], nf[1], stride, n_samples, d_M[0],
                               d_M[1], (unsigned *)nullptr);
    }
    hipLaunchKernelGGL(k_descriptor_basis, dim3(NFAM), dim3(64), 0, st, (const double *)d_M[0], (const double *)d_M[1], nf[0], nf[1], n_samples, d_Q,
                       d_Q + q_doubles, zero_word, spread_host);
    TSC_HIP(hipGetLastError());
    return 0;
}


// rows are valid: the choice only moves how many pairs the screen drops); otherwise it is estimated from the structures.
// Everything is enqueued; nothing waits for the host.
static int build_descriptors(tsc_prune *p, const double *basis) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    const int h = p->h;
    const int nf[NFAM] = {n_features(h, 0), n_features(h, 1)};
    const size_t q_doubles = size_t(KD) * (nf[0] + nf[1]);
    Scratch s(c);
    const double *d_Q = basis;
    if (!basis) {
        const int n_samples = int(std::min<int64_t>(p->n, DESC_SAMPLE));
        const int64_t stride = std::max<int64_t>(1, p->n / n_samples);
        double *q;
        TSC_TRY(s.get(basis_doubles(h), &q));
        if (p->n < c->opt.pca_min_n) {  // small ensemble: the identity basis, one tiny launch (descriptor_kernels.hpp)
            hipLaunchKernelGGL(k_identity_basis, dim3(1), dim3(256), 0, st, nf[0], nf[1], q, q + q_doubles);
            TSC_HIP(hipGetLastError());
        } else {
            TSC_TRY(build_basis(c, st, s, p->heavy, h, n_samples, stride, q));
        }
        d_Q = q;
    }
    // structures per block of k_descriptors: as many as fit 48 KB of LDS next to the basis (a power of two, 4..64: the
    // 256 / S lanes that share a structure must be one wavefront at most)
    const size_t pitch = size_t(h * 3) | 1;
    int S = 64;
    while (S > 4 && (q_doubles + size_t(S) * pitch) * sizeof(double) > 48 * 1024) S >>= 1;
    const size_t lds_desc = (q_doubles + size_t(S) * pitch) * sizeof(double);
    TSC_REQUIRE(lds_desc <= 150 * 1024, "%d heavy atoms per structure exceed what the descriptor kernel can stage in LDS", h);
    if (lds_desc > 64 * 1024)
        TSC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_descriptors), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_desc)));
    hipLaunchKernelGGL(k_descriptors, dim3(ceil_div<int64_t>(p->n, S)), dim3(256), lds_desc, st, p->heavy, p->n, h, nf[0], nf[1], d_Q,
                       (const double *)(d_Q + q_doubles), p->Dall, p->Gall, p->dmax_bits, S);
    TSC_HIP(hipGetLastError());
    return 0;  // the scratch blocks go back to the stream-ordered cache: later users run after these kernels
}

// ---- tsc_prune_create in steps; every error behind the first is undone by tsc_prune_destroy, at the one caller (prune_create_impl) ----

// 1. the argument checks and the registration: the run with its word of pinned memory (the culled-or-walked verdict of a candidate pass)
// and its entry in the context's list
static int prune_register(tsc_ctx *c, const double *heavy_dev, int64_t n, int h, double rmsd_thr, int mode, tsc_prune **out, tsc_prune **run) {
    TSC_REQUIRE(c && heavy_dev && out, "tsc_prune_create: null argument");
    TSC_REQUIRE(n > 0 && n < INT32_MAX - 4096, "n = %lld not supported", (long long)n);
    TSC_REQUIRE(h > 0, "no heavy atoms: the reference divides by zero here (rmsd_pruning.py:35)");
    TSC_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (reference-exact) or 1 (cache-free)");
    TSC_REQUIRE(rmsd_thr > 0, "rmsd_thr must be positive");
    TSC_REQUIRE(c->opt.prune_algo != ALGO_TILE || h <= MAX_HP, "prune_algo=1 (register-tiled kernel) supports at most %d heavy atoms, got %d", MAX_HP, h);
    *out = nullptr;
    tsc_prune *p = new (std::nothrow) tsc_prune(c);
    if (!p) return fail(TSC_ERR_NOMEM, "out of host memory");
    p->heavy = heavy_dev;
    p->n = n;
    p->npad = (n + 63) / 64 * 64 + 320;  // the last column tile of a segment reads up to 255 columns past the active count
    p->h = h;
    p->hp = (h + 3) / 4 * 4;
    p->thr = rmsd_thr;
    p->mode = mode;
    p->algo = (c->opt.prune_algo == ALGO_TILE) ? ALGO_TILE : ALGO_SIEVE;
    p->det_desc = c->opt.deterministic_basis != 0;
    p->cur.start(n);   // (the first pass of the schedule is opened by k_init_run itself)
    std::lock_guard<std::mutex> lock(c->owned.mutex);
    static_assert(PINNED_FLAG_SLOTS == 64, "one bit per flag word");
    const int slot = ~c->flag_slots_used ? __builtin_ctzll(~c->flag_slots_used) : -1;
    if (slot < 0) {
        delete p;
        return fail(TSC_ERR_STATE, "tsc_prune_create: %d prune runs are alive on this context, the most it serves at a time (destroy some, or use a "
                                   "context per thread)", PINNED_FLAG_SLOTS);
    }
    c->flag_slots_used |= 1ull << slot;
    p->flag_slot = slot;
    c->owned.adopt_locked(p);
    *run = p;
    return 0;
}

// 2. the pair kernel of the run, where neither the caller nor the options name it and no basis comes from a pipeline around the run: estimate
// the basis now and ask whether the screen can separate anything (one synchronisation, some 20 us, on a run of at least 30 000 structures).
// *basis: the estimate, where the sieve's descriptors are to be built from it
static int choose_kernel(tsc_prune *p, Scratch &s_basis, const double **basis, const ExternalDescriptors *ext, int force_algo) {
    tsc_ctx *c = p->ctx;
    if (force_algo >= 0) p->algo = force_algo;
    if (force_algo >= 0 || !(c->opt.prune_algo == ALGO_AUTO && p->mode == 1 && p->h <= MAX_HP && p->n >= AUTO_TILE_MIN_N && !*basis && !(ext && ext->D))) return 0;
    const int n_samples = int(std::min<int64_t>(p->n, DESC_SAMPLE));
    double *q = nullptr;
    TSC_TRY(s_basis.get(basis_doubles(p->h), &q));
    TSC_TRY(build_basis(c, c->stream, s_basis, p->heavy, p->h, n_samples, std::max<int64_t>(1, p->n / n_samples), q));
    double *host = reinterpret_cast<double *>(static_cast<char *>(c->pinned) + PINNED_SPREAD_OFFSET);
    hipError_t e = hipMemcpyAsync(host, q + basis_spread_offset(p->h), NFAM * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(TSC_ERR_HIP, "descriptor spread read-back failed: %s", hipGetErrorString(e));
    if (screen_is_useless(host, p->h, p->thr)) p->algo = ALGO_TILE, p->auto_tile = true;
    else *basis = q;  // (the sieve's descriptors are built from it further down)
    return 0;
}

// 3. the run's blocks: what every run has ...
static int alloc_always(tsc_prune *p, uint8_t *mask_buffer) {
    const size_t n = size_t(p->n);
    p->bit_words = bit_words_of(p->n), p->dsum_words = dsum_words_of(p->bit_words);
    p->n_blocks = int(scan_bsum_count(p->n));
    if (mask_buffer) p->mask = mask_buffer;  // the caller's verdict buffer serves as the working mask (8-byte aligned, n bytes)
    else TSC_TRY(p->get(n, &p->mask));
    TSC_TRY(p->get(n, &p->act));
    TSC_TRY(p->get(n, &p->cend));
    TSC_TRY(p->get(n, &p->best));
    TSC_TRY(p->get(size_t(p->n_blocks) + 1, &p->bsum));
    TSC_TRY(p->get(size_t(p->n_blocks) + 1, &p->boff));
    TSC_TRY(p->get(2 * (n / 16 + 8), &p->tile_cmax));  // (per tile: largest stop column, smallest first column)
    TSC_TRY(p->get(n / 16 + 8, &p->tile_done));
    TSC_TRY(p->get(n, &p->known));
    TSC_TRY(p->get(n, &p->cbeg));
    TSC_TRY(p->get(2 * p->bit_words, &p->bits));
    int v = 0;
    for (int slot = 0; slot < TSC_MAX_PASSES; ++slot) p->view_of_slot[slot] = (pass_can_run(p->n, slot) && p->mode == 0) ? v++ : -1;
    p->n_views = n_views_of(p->n, p->mode);
    TSC_TRY(p->get(std::max<size_t>(1, size_t(p->n_views) * view_stride(p->bit_words)), &p->views));
    TSC_TRY(p->get(TSC_MAX_PASSES, &p->view_pass));
    TSC_TRY(p->get(TSC_MAX_PASSES, &p->counters_all));
    TSC_TRY(p->get(TSC_MAX_PASSES, &p->state_all));
    p->counters = p->counters_all, p->state = p->state_all;  // (pass_launch moves them to the slot of the pass in flight)
    TSC_TRY(p->get(TSC_MAX_PASSES, &p->records));
    return 0;
}

// ... what the sieve kernels read (external descriptors: already enqueued on this stream, the caller owns the buffers) ...
static int alloc_sieve(tsc_prune *p, const ExternalDescriptors *ext) {
    tsc_ctx *c = p->ctx;
    const int64_t n = p->n;
    if (ext && ext->D) {
        p->Dall = ext->D, p->Gall = ext->G, p->dmax_bits = ext->dmax_bits;
    } else {
        TSC_TRY(p->get(size_t(n) * DW, &p->Dall));
        TSC_TRY(p->get(size_t(n), &p->Gall));
        TSC_TRY(p->get(4, &p->dmax_bits));
    }
    TSC_TRY(p->get(size_t(n) * DW, &p->Dc));
    // (mm.hpp; decided per run: the 64-row kernels for large runs, the 16-row form of the walked kernel -- "sieve_mm16" -- below that)
    p->mm64 = c->opt.sieve_mm == 2 || (c->opt.sieve_mm == 1 && n >= c->opt.mm_min_n);
    if (p->mm64 || c->opt.sieve_mm16 != 0) TSC_TRY(p->get(size_t(n) * MM_REC_HALVES, &p->Dh));
    // the records by structure index of the chunk-local pass's matrix-core screen ("sieve_mm16"): only where a pass of the schedule can have
    // chunks short enough for that kernel (a rank's share of a partitioned pass may leave the longer last chunk to another rank)
    bool local_possible = false;
    for (int slot = 0; slot < TSC_MAX_PASSES; ++slot)
        local_possible = local_possible || (pass_can_run(n, slot) && n / int64_t(KS[slot]) <= std::min(LP_MAX_ROWS, c->opt.local_max_chunk));
    if (c->opt.sieve_mm16 != 0 && c->opt.local_pass != 0 && local_possible) TSC_TRY(p->get(size_t(n) * MM_REC_HALVES, &p->Drec));
    // the float32 copy stage 1 reads (pair_stages.hpp, pair_stage1): from the embedding kernel where there was one, else converted here
    // (it pays where the gathers come from HBM: 41 MB of heavy atoms at C3 sit in the 256 MB infinity cache and the conversions cost the
    // VALU-bound kernel 2 %; at C4's 348 MB a step goes from 12.1 to 10.6 ms.  "stage1_f32": 0 never, 1 from 128 MB on, 2 always)
    if (!want_heavy32(c->opt, double(n) * p->h * 24.0)) return 0;
    if (ext && ext->heavy32) {  // written by the kernel that embedded the structures
        p->heavy32 = ext->heavy32;
        return 0;
    }
    TSC_TRY(p->get(size_t(n) * heavy32_pitch(p->h), &p->heavy32));
    hipLaunchKernelGGL(k_heavy32, dim3(unsigned(std::min<int64_t>(ceil_div<int64_t>(n * heavy32_pitch(p->h), 256), 65536))), dim3(256), 0, c->stream, p->heavy, n,
                       p->h, p->heavy32);
    return 0;
}

// ... and the compacted layouts of the register-tiled kernel
static int alloc_tile(tsc_prune *p) {
    const size_t hp3 = size_t(p->hp) * 3;
    TSC_TRY(p->get(size_t(p->npad) * hp3, &p->Xr));
    TSC_TRY(p->get(size_t(p->npad) * hp3, &p->Xc));
    TSC_TRY(p->get(size_t(p->npad), &p->G));
    return 0;
}

// 4. what k_init_run is handed.  rec_here: it also writes the records by structure (two structures per thread then, not eight)
static InitArgs init_args(const tsc_prune *p, bool own_desc, bool rec_here) {
    const int first_slot = p->cur.opened;  // the pass tsc_prune_next_pass will hand out first: opened by k_init_run itself
    InitArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.n = p->n, ia.mask = p->mask, ia.bits = p->bits, ia.bit_words = int(p->bit_words);
    ia.views = p->views, ia.view_words = int64_t(p->n_views) * int64_t(view_stride(p->bit_words)), ia.view_pass = p->view_pass, ia.n_views = p->n_views;
    for (int slot = 0; slot < TSC_MAX_PASSES; ++slot)
        if (p->view_of_slot[slot] >= 0) ia.sched[p->view_of_slot[slot]] = view_pass(int(p->n), int(KS[slot]));
    ia.st = p->state_all, ia.rec = p->records, ia.n_rec = TSC_MAX_PASSES, ia.cnt = p->counters_all;  // (every slot's)
    ia.bsum = p->bsum, ia.boff = p->boff, ia.n_blocks = p->n_blocks, ia.block_items = SCAN_TILE;
    ia.dmax_bits = own_desc ? p->dmax_bits : nullptr;
    // the arrival counters and the per-tile ones lie in two blocks: the tickets are zeroed here, tile_done by its own loop below
    ia.zero_words = reinterpret_cast<unsigned *>(p->tickets), ia.n_zero_words = int64_t(sizeof(*p->tickets) / sizeof(unsigned));
    ia.act = p->act, ia.first_slot = first_slot, ia.first_k = first_slot >= 0 ? (long long)KS[first_slot] : 0ll, ia.first_algo = p->algo;
    ia.tile_done = p->tile_done, ia.n_tile_done = p->n / 16 + 8;
    ia.known = p->known;
    if (rec_here) ia.Dall = p->Dall, ia.rec_dmax_bits = p->dmax_bits, ia.mm_rec = p->Drec;
    return ia;
}

// 5. the launches: the state of every slot, then the descriptors and records of a run that builds its own
static int first_launches(tsc_prune *p, const double *basis, bool own_desc) {
    hipStream_t st = p->ctx->stream;
    const int64_t n = p->n;
    // External descriptors (and their maximum) were enqueued on this stream in front of the run: final here, k_init_run writes the records by
    // structure as it walks n.  A run that builds its own descriptors does so BEHIND this launch, which zeroes the maximum they raise: its
    // records come from k_mm_records behind build_descriptors, below.
    const bool rec_here = p->Drec && !own_desc;
    hipLaunchKernelGGL(k_init_run, dim3(grid_for(n / (rec_here ? 2 : 8) + 1, 256, 512)), dim3(256), 0, st, init_args(p, own_desc, rec_here));
    hipError_t e = hipGetLastError();
    // padded columns of the compacted layouts are read by the last column tile of a segment but never used; the
    // register-tiled kernel's buffers are zeroed once so that those reads see finite numbers
    if (e == hipSuccess && p->Xc) e = hipMemsetAsync(p->Xc, 0, size_t(p->npad) * p->hp * 3 * sizeof(double), st);
    if (e == hipSuccess && p->Xr) e = hipMemsetAsync(p->Xr, 0, size_t(p->npad) * p->hp * 3 * sizeof(double), st);
    if (e == hipSuccess && p->G) e = hipMemsetAsync(p->G, 0, size_t(p->npad) * sizeof(double), st);
    if (e != hipSuccess) return fail(TSC_ERR_HIP, "prune state setup failed: %s", hipGetErrorString(e));
    if (p->Dall && own_desc) TSC_TRY(build_descriptors(p, basis));
    if (p->Drec && own_desc) {
        hipLaunchKernelGGL(k_mm_records, dim3(grid_for(n, 256, 1024)), dim3(256), 0, st, (const float *)p->Dall, n, (const unsigned *)p->dmax_bits, p->Drec);
        if (hipGetLastError() != hipSuccess) return fail(TSC_ERR_HIP, "the records of the chunk-local pass could not be written");
    }
    return 0;
}

static int prune_setup(tsc_prune *p, uint8_t *mask_buffer, const double *basis, const ExternalDescriptors *ext, int force_algo) {
    Scratch s_basis(p->ctx);
    TSC_TRY(choose_kernel(p, s_basis, &basis, ext, force_algo));
    TSC_TRY(alloc_always(p, mask_buffer));
    if (p->algo == ALGO_SIEVE) TSC_TRY(alloc_sieve(p, ext));
    TSC_TRY(p->get(1, &p->tickets));
    if (p->algo == ALGO_TILE) TSC_TRY(alloc_tile(p));
    return first_launches(p, basis, !(ext && ext->D));
}

static int prune_create_impl(tsc_ctx *c, const double *heavy_dev, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask_buffer, tsc_prune **out,
                             const double *basis = nullptr, const ExternalDescriptors *ext = nullptr, int force_algo = -1) {
    tsc_prune *p = nullptr;
    TSC_TRY(prune_register(c, heavy_dev, n, h, rmsd_thr, mode, out, &p));
    DeviceGuard guard(c->device);
    const int rc = prune_setup(p, mask_buffer, basis, ext, force_algo);
    if (rc) {
        tsc_prune_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_create(tsc_ctx *c, const double *heavy_dev, int64_t n, int h, double rmsd_thr, int mode, tsc_prune **out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c != nullptr, "tsc_prune_create: null argument");
    // descriptors that tsc_embed_masked_dev wrote with this very array are used once, by the run created next ...
    if (c->xd_valid && c->xd_h == h && c->xd_heavy == heavy_dev && n <= c->xd_cap && c->opt.prune_algo != ALGO_TILE) {
        ExternalDescriptors ext;
        ext.D = c->xd_D, ext.G = c->xd_G, ext.dmax_bits = c->xd_dmax;
        ext.heavy32 = c->xd_h32_valid ? c->xd_heavy32 : nullptr;
        c->xd_valid = false;
        TSC_TRY(prune_create_impl(c, heavy_dev, n, h, rmsd_thr, mode, nullptr, out, nullptr, &ext));
        std::lock_guard<std::mutex> lock(c->owned.mutex);
        (*out)->borrows_xd = true;   // (tsc_embed_masked_dev will not release or regrow the buffers under this run)
        ++c->xd_borrowers;
        return 0;
    }
    c->xd_valid = false;
    // ... and so is a basis that tsc_embed_clash_compact_dev / tsc_basis_from_poses_dev estimated on the side stream
    const double *basis = pending_basis(c, h);
    if (basis) {
        DeviceGuard guard(c->device);
        TSC_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    c->eb_valid = false;
    return prune_create_impl(c, heavy_dev, n, h, rmsd_thr, mode, nullptr, out, basis);
    TSC_API_GUARD_END
}

// the call order of the stepping API (pass_cursor.hpp: refusal): 0, or TSC_ERR_STATE with the message of the entry point
static int allowed(const tsc_prune *p, StepCall call) {
    const char *why = p->cur.refusal(call);
    return why ? fail(TSC_ERR_STATE, "%s", why) : 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_next_pass(tsc_prune *p, int64_t *k_out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && k_out, "null argument");
    TSC_TRY(allowed(p, StepCall::NextPass));
    const int slot = p->cur.next_slot();
    p->cur.begin(slot);
    *k_out = slot >= 0 ? p->cur.k : 0;
    return 0;
    TSC_API_GUARD_END
}

// Rough size of the open pass in pairs (n structures, every row against half of an average chunk); it depends only
// on n and k, so every rank of a sharded run computes the same number.
extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_estimate(tsc_prune *p, int64_t *pairs) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && pairs, "null argument");
    TSC_TRY(allowed(p, StepCall::Estimate));
    *pairs = p->n * (p->n / p->cur.k) / 2;
    return 0;
    TSC_API_GUARD_END
}

// ---- what the launches of a pass share ----

// the pair kernel's own start / stop events ride on its dispatch packet (no extra packets in the stream; a hipEventRecord before and
// after it costs about 4 us each on MI355X).  level: the "pass_timing" from which this kernel is timed
struct PairEvents {
    hipEvent_t e0, e1;
};
static PairEvents pair_events(const tsc_prune *p, int level) {
    const bool on = p->ctx->opt.pass_timing >= level;
    return PairEvents{on ? p->ev[p->cur.slot][1] : nullptr, on ? p->ev[p->cur.slot][2] : nullptr};
}

// the thresholds of the open run, the same in every argument block that has them (pass_plan.hpp: thresholds)
template <typename Args>
static void put_thresholds(const tsc_prune *p, Args &a) {
    const Thresholds t = thresholds(p->h, p->thr);
    a.thr = t.thr, a.maxdev_thr = t.maxdev_thr;  // :95
    a.half_h_thr2 = t.half_h_thr2;
}
template <typename Args>
static void put_screen_thresholds(const tsc_prune *p, Args &a) {
    const Thresholds t = thresholds(p->h, p->thr);
    put_thresholds(p, a);
    a.two_thr2 = t.two_thr2, a.desc_limit = t.desc_limit;
    a.dmax_bits = p->dmax_bits;
}
// rows: the bound the grid was sized for -- tiles of the last block beyond it must leave before they read a stale tile_cmax[] entry and
// arrive at the pass's counter as a tile that does not exist.  tile_cmax: null in a culled pass, whose tiles lie in another order
static SieveArgs sieve_args(const tsc_prune *p, int rows, int rank, int world, int seg_cols, const int32_t *tile_cmax) {
    SieveArgs a;
    memset(&a, 0, sizeof(a));
    a.n = rows, a.h = p->h;
    a.tile_begin = rank, a.tile_stride = world, a.seg_cols = seg_cols;
    put_screen_thresholds(p, a);
    a.heavy32 = p->heavy32;
    a.tile_cmax = tile_cmax, a.cbeg = p->cbeg;   // (both written by this pass's k_open_rows)
    a.drain_min = p->ctx->opt.drain_min;
    return a;
}

#ifdef TSC_DBG_STAMPS
// room for 8 time stamps of each of `waves` wavefronts (tools/stamps.py), cleared on the stream
static int stamp_buffer(tsc_ctx *c, int64_t waves, unsigned long long **dbg) {
    const size_t bytes = size_t(waves) * 8 * sizeof(unsigned long long);
    if (c->dbg_bytes < bytes) {
        if (c->dbg_buf) (void)hipFree(c->dbg_buf);
        TSC_HIP(hipMalloc(&c->dbg_buf, bytes));
        c->dbg_bytes = bytes;
    }
    TSC_HIP(hipMemsetAsync(c->dbg_buf, 0, bytes, c->stream));
    c->dbg_waves = waves;
    *dbg = static_cast<unsigned long long *>(c->dbg_buf);
    return 0;
}
#endif

// ---- the walked pass: the pair search of one rank's row tiles of the open pass, in index order (step 3 of a pass; steps 1-2 have run) ----
// fused: the pair kernel applies the rows of its own tiles; rows_ub, rows_now: pass_plan.hpp, plan_walked
static int walked_pass(tsc_prune *p, int rank, int world, bool fused, int64_t rows_ub, int64_t rows_now = -1) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    const PairForm form = pair_form(c->opt, p->algo, p->Dh != nullptr, p->mm64);
    const WalkedPlan w = plan_walked(c->opt, p->n, p->cur.k, rank, world, rows_ub, rows_now, form);
    const PairEvents ev = pair_events(p, 1);
    if (p->algo == ALGO_TILE) {
        TileArgs a;
        a.ld = p->npad, a.h = p->h;
        a.tile_begin = rank, a.tile_stride = world, a.seg_cols = w.seg_cols;
        put_thresholds(p, a);
        TSC_TRY(launch_rmsd_tile(p->hp, st, w.grid, ev.e0, ev.e1, (const double *)p->Xr, (const double *)p->Xc, (const double *)p->G, (const int32_t *)p->cend,
                                 p->best, p->counters, (const PruneState *)p->state, a));
        TSC_HIP(hipGetLastError());
        return 0;
    }
    SieveArgs a = sieve_args(p, w.rows, rank, world, w.seg_cols, p->tile_cmax);
#ifdef TSC_DBG_STAMPS
    if (c->opt.dbg_stamp_k == p->cur.k) TSC_TRY(stamp_buffer(c, int64_t(w.grid.x) * w.grid.y * 4, &a.dbg));
#endif
    FusedApply fa;
    memset(&fa, 0, sizeof(fa));
    if (fused) {
        fa.ap = apply_args(p);
        // a rank-partitioned pass is closed by the pair kernel's last tile (its statistics go to the exchange buffer); any other is left
        // open -- no arrivals, no closing wavefront -- and closed behind the kernel boundary by the first kernel of the next pass
        fa.tile_done = p->tile_done, fa.tickets = p->cur.range ? &p->tickets->pass : nullptr, fa.n_tiles = unsigned(w.n_tiles);
        fa.sc = step_ctx(p, p->cur.range);
        fa.next = next_step_args(p);
    }
    const bool trim = c->opt.sieve_cpl == 2 && c->opt.sieve_trim;
    if (form.mm16) {
        TSC_TRY(launch_rmsd_sieve_mm16(fused, a.heavy32 != nullptr, w.mm16_waves, st, w.grid, ev.e0, ev.e1, p->heavy, (const int32_t *)p->act,
                                       (const double *)p->Gall, (const _Float16 *)p->Dh, (const int32_t *)p->cend, p->best, p->counters,
                                       (const PruneState *)p->state, a, fa));
        return 0;
    }
    if (form.mm) {
        TSC_TRY(launch_rmsd_sieve_mm(fused, a.heavy32 != nullptr, st, w.grid, ev.e0, ev.e1, p->heavy, (const int32_t *)p->act, (const double *)p->Gall,
                                     (const float *)p->Dc, (const _Float16 *)p->Dh, (const int32_t *)p->cend, p->best, p->counters, (const PruneState *)p->state, a,
                                     fa));
        return 0;
    }
    // (stage 1 on the float32 copy exists for the default shape of the kernel only)
    TSC_TRY((fused ? launch_rmsd_sieve_fused : launch_rmsd_sieve_plain)(
        c->opt.sieve_cpl, trim, trim && a.heavy32 != nullptr, st, w.grid, ev.e0, ev.e1, p->heavy, (const int32_t *)p->act, (const double *)p->Gall, (const float *)p->Dc,
        (const int32_t *)p->cend, p->best, p->counters, (const PruneState *)p->state, a, fa));
    TSC_HIP(hipGetLastError());
    return 0;
}

// ---- the chunk-local pass: the whole pass in one launch, a workgroup (or a few) per chunk (local_pass.hpp) ----
static int local_pass(tsc_prune *p, const PassGeom &g, const PassRows &r, bool range) {
    const LocalPlan l = plan_local(p->n, p->cur.k, r);
    LocalPassArgs a;
    a.h = p->h, a.use_cache = (p->mode == 0);
    a.nb_regular = l.nb_regular, a.nb_last = l.nb_last;
    a.c_lo = int(r.c_lo), a.n_reg = l.n_reg;
    a.exch = range ? p->exch : nullptr;
    // (the records exist where "sieve_mm16" was on when the run was created; the option is looked at again: a run may be stepped under another value)
    a.rec = p->ctx->opt.sieve_mm16 != 0 ? p->Drec : nullptr;
    a.dbg = nullptr;
#ifdef TSC_DBG_STAMPS
    if (p->ctx->opt.dbg_stamp_k == p->cur.k) TSC_TRY(stamp_buffer(p->ctx, int64_t(l.blocks) * 4, &a.dbg));
#endif
    put_screen_thresholds(p, a);
    const StepArgs sa = next_step_args(p, true);
    // (its own events only at pass_timing 2: level 1 is what a timed region carries for the PAIR kernel's durations, and a pair of
    // events costs a small pass about 6 us)
    const PairEvents ev = pair_events(p, 2);
    // (range: the last block leaves the statistics in the exchange buffer; otherwise the pass is left open, as in walked_pass)
    TSC_TRY(launch_pass_chunks(a.rec != nullptr, p->ctx->stream, unsigned(l.blocks), ev.e0, ev.e1, g, a, p->state, p->mask, p->bits, int(p->bit_words), view_of_open_pass(p), p->heavy,
                               (const double *)p->Gall, (const float *)p->Dall, later_views(p), p->counters, p->bsum, SCAN_TILE, step_ctx(p, range), sa,
                               range ? &p->tickets->local : nullptr, derive_args(p)));
    return 0;
}

// ---- what the culled and the walked pass have in front of them ----
// 1. per row: which structure it is, its stop column, best[] = none, its descriptor by position (k_open_rows, rmsd.hpp); the coordinates by
// position for the register-tiled kernel
static int open_rows(tsc_prune *p, const PassGeom &g, const PassShape &s, bool range, int world) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    const OpenPlan o = plan_open_rows(s.rows_ub);
    OpenArgs oa;
    // (fused: tiles without columns arrive at the pass's counter here -- only where the pair kernel's last tile closes the pass, walked_pass)
    oa.use_cache = (p->mode == 0), oa.fused = (s.fused && range) ? 1 : 0, oa.lds_cap = std::min(c->opt.open_lds_blocks, OPEN_LDS_BLOCKS);
    oa.view = view_of_open_pass(p), oa.bits = p->bits, oa.bit_words = int(p->bit_words);
    oa.boff = p->boff, oa.n_blocks = p->n_blocks, oa.block_items = SCAN_TILE;
    oa.n_tiles = o.n_tiles, oa.tickets = &p->tickets->pass;
    oa.dv = derive_args(p), oa.bsum = p->bsum, oa.boff_out = p->boff;
    oa.rank_of = s.culled ? p->rank_of : nullptr;
    oa.Dh = p->Dh, oa.dmax_bits = p->dmax_bits;
    // known[]: read and raised where every row of the pass is opened and applied on this device (a rank's share of a partitioned pass, and a
    // pass dealt to several ranks, leave it alone: too small is always safe).  The rows' first columns are HONOURED -- a tile with nothing
    // left is declared dead here, the known pairs are counted -- where the kernel behind this launch is the 16-row matrix-core kernel
    // applying its own tiles: a candidate for culling may end in another kernel, and k_apply_pass counts every row itself
    const bool track = c->opt.skip_known != 0 && !range && world == 1;
    const bool skip = track && s.fused && !s.culled && pair_form(c->opt, p->algo, p->Dh != nullptr, p->mm64).mm16;
    oa.known = track ? p->known : nullptr, oa.cbeg = p->cbeg, oa.skip = skip ? 1 : 0;
    oa.dbg = nullptr;
#ifdef TSC_DBG_STAMPS
    if (c->opt.dbg_stamp_k == -p->cur.k) TSC_TRY(stamp_buffer(c, int64_t(o.stamp_blocks) * 4, &oa.dbg));  // (a negative k selects k_open_rows of pass k)
#endif
    const StepArgs sa = s.fused ? next_step_args(p) : StepArgs{-1, -1, 0ll, 0, -1};
    static_assert(SCAN_TILE == 64 * SCAN_BLOCK_WORDS && DW == DESC_WORDS, "k_open_rows");
    hipLaunchKernelGGL(k_open_rows, dim3(o.blocks), dim3(256), 0, st, g, oa, step_ctx(p, range), sa, p->act, p->cend, p->best, p->tile_cmax, (const float *)p->Dall,
                       s.need_dc ? p->Dc : nullptr);
    if (p->algo == ALGO_TILE) {
        const int hp3 = p->hp * 3;
        size_t lds = size_t(64) * (hp3 + 1) * sizeof(double);
        hipLaunchKernelGGL(k_compact_coords, dim3(ceil_div(s.rows_ub, 64)), dim3(256), lds, st, p->heavy, p->h, hp3, p->act, (const PruneState *)p->state, p->Xr,
                           p->Xc, p->npad, p->G);
    }
    return 0;
}

// ---- the culled pass: the structures laid out along a Morton curve, tile pairs skipped by bounding box (cull.hpp); the verdicts are
// applied by k_apply_pass behind the pair kernel (tsc_prune_pass_finish), on one rank or several ----

// its buffers, when the first candidate comes up (in front of k_open_rows, which fills rank_of)
static int cull_buffers(tsc_prune *p) {
    if (p->morton_order) return 0;
    const size_t n = size_t(p->n);
    TSC_TRY(p->get(n, &p->morton_order));
    TSC_TRY(p->get(n, &p->rank_of));
    TSC_TRY(p->get(n + 256, &p->crank));
    TSC_TRY(p->get(size_t(CULL_MAX_CHUNKS) + 1, &p->cbase));
    TSC_TRY(p->get(size_t(CULL_MAX_CHUNKS) + 1, &p->cfill));
    TSC_TRY(p->get((n / CULL_LAYOUT_ITEMS + 2) * CULL_MAX_CHUNKS, &p->blk_cnt));
    TSC_TRY(p->get((n + 256) * DW, &p->Ds));
    if (p->Dh && p->mm64) TSC_TRY(p->get((n + 256) * MM_REC_HALVES, &p->Dhs));
    if (p->Dh && p->mm64) TSC_TRY(p->get(n + 256, &p->cstruct));
    TSC_TRY(p->get((n / CULL_COLS + 2) * CULL_BOX, &p->cbox));
    TSC_TRY(p->get((n / CULL_COLS + 2) * 8 * CULL_BOX, &p->rbox));
    return 0;
}

// once per run: the structures in coarse Morton order of their descriptors -- a stable two-digit radix sort by cell, so that
// every rank of a sharded run comes to the same order (cull.hpp)
static int morton_sort(tsc_prune *p) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    const int64_t n = p->n;
    Scratch s(c);
    int32_t *tmp, *blk, *tot;
    const int n_rb = int(ceil_div<int64_t>(n, 2048));
    TSC_TRY(s.get(size_t(n), &tmp));
    TSC_TRY(s.get(size_t(n_rb) * RADIX_BUCKETS, &blk));
    TSC_TRY(s.get(size_t(RADIX_BUCKETS), &tot));
    static_assert(CULL_MORTON_BITS * CULL_MORTON_DIMS <= 16, "two 8-bit digits");
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *in = pass == 0 ? nullptr : tmp;
        int32_t *out = pass == 0 ? tmp : p->morton_order;
        hipLaunchKernelGGL(k_radix_count, dim3(unsigned(n_rb)), dim3(256), 0, st, (const float *)p->Dall, in, n, (const unsigned *)p->dmax_bits, 8 * pass, blk);
        hipLaunchKernelGGL(k_radix_scan, dim3(RADIX_BUCKETS), dim3(64), 0, st, n_rb, blk, tot);
        hipLaunchKernelGGL(k_radix_base, dim3(1), dim3(256), 0, st, tot);
        hipLaunchKernelGGL(k_radix_scatter, dim3(unsigned(n_rb)), dim3(256), 0, st, (const float *)p->Dall, in, n, (const unsigned *)p->dmax_bits, 8 * pass,
                           (const int32_t *)blk, (const int32_t *)tot, out);
    }
    TSC_HIP(hipGetLastError());
    p->morton_sorted = true;
    return 0;
}

// culled, or walked in index order?  The rows' ranges decide (k_cull_decide); the host waits for the verdict -- a pass this
// large takes a millisecond or more, the round trip some 20 us.  *rows_now: the pass's rows, which the host learns with it
static int cull_verdict(tsc_prune *p, const PassGeom &g, bool *run_culled, int64_t *rows_now) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    volatile int *flag = reinterpret_cast<volatile int *>(static_cast<char *>(c->pinned) + PINNED_FLAG_OFFSET + 64 * size_t(p->flag_slot));
    *flag = 0;
    hipLaunchKernelGGL(k_chunk_bases, dim3(unsigned(g.k + 1)), dim3(64), 0, st, g, (const PruneState *)p->state, (const int32_t *)p->boff,
                       (const unsigned long long *)p->bits, int(p->bit_words), p->n_blocks, p->cbase, p->cfill);
    hipLaunchKernelGGL(k_cull_decide, dim3(1), dim3(64), 0, st, p->state, (const PassCounters *)p->counters, (const int32_t *)p->cbase, g.k, c->opt.cull == 2 ? 1 : 0,
                       const_cast<int *>(flag));
    TSC_HIP(hipStreamSynchronize(st));
    *run_culled = *flag != 0;
    *rows_now = flag[1];
    return 0;
}

// A candidate pass: *ran = false where the device's verdict is "walked" (nothing but the verdict's two kernels has been enqueued then)
static int culled_pass(tsc_prune *p, int rank, int world, bool range, const PassGeom &g, const PassShape &s, const PassRows &r, bool *ran, int64_t *rows_now) {
    tsc_ctx *c = p->ctx;
    hipStream_t st = c->stream;
    const int64_t n = p->n, k = p->cur.k;
    TSC_TRY(cull_verdict(p, g, ran, rows_now));
    if (!*ran) return 0;
    if (!p->morton_sorted) TSC_TRY(morton_sort(p));
    // (the culled pass with the screen on the matrix cores: groups of 64 rows of the layout, dealt to the ranks in runs of tile_block / 4)
    const bool cull_mm = p->Dhs && p->mm64;
    const int n_lb = int(ceil_div<int64_t>(n, CULL_LAYOUT_ITEMS));
    const LayoutRange lr{int(r.s_lo), int(r.s_hi)};
    hipLaunchKernelGGL(k_layout_count, dim3(unsigned(n_lb)), dim3(256), 0, st, g, lr, (const PruneState *)p->state, (const int32_t *)p->morton_order,
                       (const unsigned long long *)p->bits, int(p->bit_words), p->blk_cnt);
    hipLaunchKernelGGL(k_layout_scan, dim3(unsigned(k)), dim3(64), 0, st, (const PruneState *)p->state, n_lb, (const int32_t *)p->cbase, p->blk_cnt);
    hipLaunchKernelGGL(k_layout_scatter, dim3(unsigned(n_lb)), dim3(256), 0, st, g, lr, (const PruneState *)p->state, (const int32_t *)p->morton_order,
                       (const unsigned long long *)p->bits, int(p->bit_words), (const int32_t *)p->rank_of, (const float *)p->Dc, (const int32_t *)p->blk_cnt, p->Ds,
                       p->crank, (const _Float16 *)(cull_mm ? p->Dh : nullptr), cull_mm ? p->Dhs : nullptr, cull_mm ? p->cstruct : nullptr);
    hipLaunchKernelGGL(k_tile_boxes, dim3(unsigned(ceil_div<int64_t>(n, CULL_COLS))), dim3(128), 0, st, (const PruneState *)p->state, (const float *)p->Ds, p->cbox,
                       p->rbox);
    const CulledPlan q = plan_culled(c->opt, s.rows_ub, s.longest_of_rank, rank, world, cull_mm);
    SieveArgs a = sieve_args(p, s.rows_ub, rank, world, CULL_SEG_COLS, nullptr);
    const CullArgs ca{p->Ds, p->crank, p->cbase, p->cbox, p->rbox, int(k), q.tile_block, c->opt.cull_xcd};
    const PairEvents ev = pair_events(p, 1);
    if (cull_mm) {
#ifdef TSC_DBG_STAMPS
        if (c->opt.dbg_stamp_k == k) TSC_TRY(stamp_buffer(c, q.grid_mm * 4, &a.dbg));  // (8 of every 32 words used: one wavefront per workgroup)
#endif
        const CullMmArgs cm{p->Dhs, p->cstruct};
        TSC_TRY(launch_rmsd_sieve_sorted_mm(a.heavy32 != nullptr, st, dim3(unsigned(std::max<int64_t>(1, q.grid_mm))), ev.e0, ev.e1, p->heavy, (const int32_t *)p->act,
                                            (const double *)p->Gall, (const int32_t *)p->cend, p->best, p->counters, (const PruneState *)p->state, a, ca, cm,
                                            q.n_groups, q.n_seg_mm));
    } else {
        TSC_TRY(launch_rmsd_sieve_sorted(a.heavy32 != nullptr, st, dim3(q.sgrid), ev.e0, ev.e1, p->heavy, (const int32_t *)p->act, (const double *)p->Gall,
                                         (const int32_t *)p->cend, p->best, p->counters, (const PruneState *)p->state, a, ca, q.my_tiles, q.n_seg));
    }
    if (range) {
        // a partitioned pass is closed by tsc_prune_pass_merge after the exchange: this rank's verdicts go into the exchange buffer
        // now (k_apply_pass in its noting form), its last block leaves the statistics there
        const int blocks = int(std::min<int64_t>(ceil_div<int64_t>(s.rows_ub, 256), 512));
        hipLaunchKernelGGL(k_apply_pass, dim3(blocks), dim3(256), 0, st, apply_args(p), step_ctx(p, true), next_step_args(p));
        TSC_HIP(hipGetLastError());
    }
    return 0;
}

// a one-block launch closes the pass that was left open and opens the slot behind it (pass_cursor.hpp: Opener::Step)
static void launch_pass_step(const tsc_prune *p, const Handover &h) {
    hipLaunchKernelGGL(k_pass_step, dim3(1), dim3(64), 0, p->ctx->stream, step_ctx_of(p, h.prev, h.next), step_args_of(p, h));
}

// The launches of a pass on this device: what every pass has (events, opening the slot on the device where the pass before it has not),
// then one of the three shapes (pass_plan.hpp: pass_shape).  range = false: the rows dealt to (rank, world) by tiles, of
// all chunks (tsc_prune_pass_local).  range = true: every row of the chunks that belong to this rank (tsc_prune_pass_range); rank / world
// are then 0 / 1 for the kernels -- they see an ensemble made of this rank's rows.
static int pass_launch(tsc_prune *p, int rank, int world, bool range) {
    tsc_ctx *c = p->ctx;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    const int64_t n = p->n, k = p->cur.k;
    const int slot = p->cur.slot;
    const PassRows r = range ? partition_bounds(n, k, p->part_rank, p->part_world) : whole_pass(n, k);
    const PassShape s = pass_shape(c->opt, n, k, p->algo, p->Dh != nullptr, p->mm64, p->det_desc, world, range, r);
    const PassGeom g{int(n), int(k), int(n / k)};
    for (int i = 0; i < 4; ++i)
        if (!p->ev[slot][i]) TSC_TRY(get_event(c, &p->ev[slot][i]));
    if (c->opt.pass_timing >= 2) TSC_HIP(hipEventRecord(p->ev[slot][0], st));
    p->state = p->state_all + slot, p->counters = p->counters_all + slot;
    // 0. open this pass: gate (:192), record, state block of its slot -- already done by the kernel that closed the pass before it (its
    //    last block; k_init_run for the first pass of a run), or the pass before it was left open: then the first kernel of this pass
    //    closes it and opens this one in its first round trip (pass_derive; derive_args reads the cursor) -- k_pass_chunks, or k_open_rows
    //    where the prefix of the scan blocks fits its LDS array; a one-block launch where neither is the first kernel
    const Handover h = p->cur.open_slot(range, !range && (s.local || p->n_blocks <= std::min(c->opt.open_lds_blocks, OPEN_LDS_BLOCKS)));
    if (h.how == Opener::Nothing)
        return fail(TSC_ERR_STATE, "prune pass k = %lld: no pass in front of it was left open and nothing has opened its slot", (long long)k);
    if (h.how == Opener::Step) launch_pass_step(p, h);
    if (range && !p->cur.rows_ready())  // no k_pass_merge in front of this pass (the first of a run): which rows are this rank's
        hipLaunchKernelGGL(k_range_open, dim3(1), dim3(64), 0, st, p->state, (const int32_t *)p->boff, (const unsigned long long *)p->bits, int(p->bit_words),
                           p->n_blocks, int(r.s_lo), int(r.s_hi));
    if (s.local) {
        TSC_TRY(local_pass(p, g, r, range));
        p->cur.launched(PassKind::Local);
        return 0;
    }
    if (world > 1 && p->auto_tile && !p->det_desc)
        return fail(TSC_ERR_STATE, "tsc_prune_pass_local: this run chose the all-pairs kernel from its own basis estimate; ranks of a sharded run could "
                                   "choose differently -- create the runs under deterministic_basis = 1, or force prune_algo 1 or 2 on every rank");
    if (s.culled) TSC_TRY(cull_buffers(p));
    TSC_TRY(open_rows(p, g, s, range, world));
    // (in a culled pass rows collect verdicts as columns of other tiles too: it is applied behind the pair kernel, by k_apply_pass)
    bool ran_culled = false;
    int64_t rows_now = -1;   // (the pass's rows, where the host has waited for the device anyway)
    if (s.culled) TSC_TRY(culled_pass(p, rank, world, range, g, s, r, &ran_culled, &rows_now));
    const bool fused = s.fused && !ran_culled;
    if (!ran_culled) TSC_TRY(walked_pass(p, rank, world, fused, s.rows_ub, rows_now));
    p->cur.launched(fused ? PassKind::Fused : PassKind::Behind);
    return 0;
}

// The open pass ends on the host (tsc_prune_pass_finish, tsc_prune_pass_merge).  closed: the last kernel enqueued for it has closed it on the
// device and opened the pass that follows; otherwise it is left open
static int end_pass(tsc_prune *p, bool closed) {
    if (closed) p->cur.closed_on_device();
    if (p->ctx->opt.pass_timing >= 2) TSC_HIP(hipEventRecord(p->ev[p->cur.slot][3], p->ctx->stream));
    p->cur.end_pass();
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_local(tsc_prune *p, int rank, int world) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank %d / world %d", rank, world);
    TSC_TRY(allowed(p, StepCall::PassLocal));
    if (p->cur.split && p->mode == 0)
        return fail(TSC_ERR_STATE, "tsc_prune_pass_local: rank-partitioned passes have run; sum the cache views over the ranks first "
                                   "(tsc_prune_views_ptr, tsc_prune_views_merged)");
    return pass_launch(p, rank, world, false);
    TSC_API_GUARD_END
}

// ---- rank-partitioned passes (rmsd.hpp, k_pass_merge) ----
// (the words of the exchange buffer: pass_cursor.hpp, exchange_words_of)
extern "C" __attribute__((visibility("default"))) int tsc_prune_exchange_words(int64_t n, int mode, int64_t *words) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(words && n > 0, "bad argument");
    *words = exchange_words_of(n, mode);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_set_partition(tsc_prune *p, int rank, int world, int min_chunks_per_rank, void *exch_dev,
                                                                              int64_t exch_words) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && exch_dev, "null argument");
    TSC_REQUIRE(world >= 1 && rank >= 0 && rank < world && min_chunks_per_rank >= 1, "bad rank %d / world %d / min_chunks_per_rank %d", rank, world,
                min_chunks_per_rank);
    const int64_t need = exchange_words_of(p->n, p->mode);
    TSC_REQUIRE(exch_words >= need, "exchange buffer of %lld words, %lld needed (tsc_prune_exchange_words)", (long long)exch_words, (long long)need);
    TSC_TRY(allowed(p, StepCall::SetPartition));
    DeviceGuard guard(p->ctx->device);
    p->part_rank = rank, p->part_world = world, p->part_min_chunks = min_chunks_per_rank;
    p->exch = static_cast<unsigned long long *>(exch_dev);
    TSC_HIP(hipMemsetAsync(p->exch, 0, size_t(need) * sizeof(unsigned long long), p->ctx->stream));
    if (p->mode == 0) p->views = p->exch + p->bit_words + EXCH_STAT_WORDS;  // the cache views live in the caller's buffer from here on (still empty)
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_partitioned(tsc_prune *p, int *flag) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && flag, "null argument");
    TSC_TRY(allowed(p, StepCall::Partitioned));
    *flag = pass_is_partitioned(p, p->cur.k) ? 1 : 0;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_range(tsc_prune *p) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_TRY(allowed(p, StepCall::PassRange));
    if (!pass_is_partitioned(p, p->cur.k)) return fail(TSC_ERR_STATE, "tsc_prune_pass_range: the open pass (k = %lld) is not rank-partitioned", (long long)p->cur.k);
    TSC_TRY(pass_launch(p, 0, 1, true));
    p->cur.split_views();
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_merge(tsc_prune *p) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_TRY(allowed(p, StepCall::PassMerge));
    tsc_ctx *c = p->ctx;
    DeviceGuard guard(c->device);
    const int nxt = p->cur.next_slot();
    MergeArgs ma;
    ma.n = int(p->n), ma.bit_words = int(p->bit_words), ma.n_blocks = p->n_blocks, ma.bits = p->bits, ma.exch = p->exch, ma.mask = p->mask;
    ma.next_s_lo = ma.next_s_hi = -1;
    if (nxt >= 0 && pass_is_partitioned(p, int64_t(KS[nxt]))) {
        const PassRows next = partition_bounds(p->n, int64_t(KS[nxt]), p->part_rank, p->part_world);
        ma.next_s_lo = int(next.s_lo), ma.next_s_hi = int(next.s_hi);
        p->cur.range_ready(nxt);
    }
    hipLaunchKernelGGL(k_pass_merge, dim3(1), dim3(1024), 0, c->stream, ma, step_ctx(p), next_step_args(p, p->cur.kind == PassKind::Local));
    TSC_HIP(hipGetLastError());
    return end_pass(p, true);
    TSC_API_GUARD_END
}

// The cache views of the passes that have not run yet (the open one included), as one block of 64-bit words: after partitioned
// passes they hold the keys of this rank's removed rows only.  *words = 0: nothing to exchange (cache-free mode, or no partitioned
// pass has run).  Otherwise: sum the block over the ranks (the ranks' bits are disjoint), then tsc_prune_views_merged.
extern "C" __attribute__((visibility("default"))) int tsc_prune_views_ptr(tsc_prune *p, void **views_dev, int64_t *offset_words, int64_t *words) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && views_dev && offset_words && words, "null argument");
    TSC_TRY(allowed(p, StepCall::ViewsPtr));
    *views_dev = nullptr, *offset_words = 0, *words = 0;
    if (!p->cur.split || p->mode != 0) return 0;
    *views_dev = view_of_open_pass(p);
    *offset_words = int64_t(view_of_open_pass(p) - p->exch);
    *words = int64_t(p->n_views - p->view_of_slot[p->cur.slot]) * int64_t(view_stride(p->bit_words));
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_views_merged(tsc_prune *p) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_TRY(allowed(p, StepCall::ViewsMerged));
    if (p->cur.split && p->mode == 0) {
        DeviceGuard guard(p->ctx->device);
        const int count = p->n_views - p->view_of_slot[p->cur.slot];
        hipLaunchKernelGGL(k_views_summaries, dim3(unsigned(std::min<int64_t>(ceil_div<int64_t>(int64_t(count) * p->dsum_words * 64, 256), 2048))), dim3(256), 0, p->ctx->stream,
                           view_of_open_pass(p), (long long)view_stride(p->bit_words), int(p->bit_words), int(p->dsum_words), count);
        TSC_HIP(hipGetLastError());
    }
    p->cur.merged_views();
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_rows(tsc_prune *p, int rank, int world) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank %d / world %d", rank, world);
    TSC_TRY(allowed(p, StepCall::PassRows));
    DeviceGuard guard(p->ctx->device);
    return walked_pass(p, rank, world, false, p->n);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_best_ptr(tsc_prune *p, void **best_dev, int64_t *n_entries) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && best_dev && n_entries, "null argument");
    TSC_TRY(allowed(p, StepCall::BestPtr));
    *best_dev = p->best;
    *n_entries = p->n;  // entries beyond the (device-side) active count are not touched by the pass
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_use_best_buffer(tsc_prune *p, void *best_dev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && best_dev, "null argument");
    TSC_TRY(allowed(p, StepCall::UseBestBuffer));
    p->best = static_cast<int32_t *>(best_dev);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_pass_finish(tsc_prune *p) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_TRY(allowed(p, StepCall::PassFinish));
    DeviceGuard guard(p->ctx->device);
    const bool behind = p->cur.kind == PassKind::Behind;  // (a chunk-local pass, and the pair kernel of a fused one, have applied the verdicts already)
    if (behind) {
        const int blocks = int(std::min<int64_t>(ceil_div<int64_t>(p->n, 256), 512));
        hipLaunchKernelGGL(k_apply_pass, dim3(blocks), dim3(256), 0, p->ctx->stream, apply_args(p), step_ctx(p), next_step_args(p));
        TSC_HIP(hipGetLastError());
    }
    return end_pass(p, behind);
    TSC_API_GUARD_END
}

// Runs every pass that needs no exchange between ranks (all of them for world == 1; for world > 1 those whose estimate is
// below min_pairs: every rank computes them whole and reaches the same verdicts) and returns with the first pass that does
// open (*k_out = its k; the caller runs tsc_prune_pass_local(rank, world), merges best[], tsc_prune_pass_finish) or with
// *k_out = 0 when the schedule is exhausted.  One host call instead of three per small pass.
extern "C" __attribute__((visibility("default"))) int tsc_prune_run_replicated(tsc_prune *p, int world, int64_t min_pairs, int64_t *k_out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && k_out && world >= 1, "null argument");
    for (;;) {
        int64_t k = 0;
        TSC_TRY(tsc_prune_next_pass(p, &k));
        *k_out = k;
        if (k == 0) return 0;
        // (a partitioned pass, or the first pass after partitioned ones -- the cache views must be summed over the ranks first --
        // goes back to the caller as well)
        if (world > 1 && (pass_is_partitioned(p, k) || (p->cur.split && p->mode == 0) || p->n * (p->n / k) / 2 >= min_pairs)) return 0;
        TSC_TRY(tsc_prune_pass_local(p, 0, 1));
        TSC_TRY(tsc_prune_pass_finish(p));
    }
    TSC_API_GUARD_END
}

// The whole pass loop of a SHARDED run behind one call (the multi-rank variant of the prune; 8e: the protocol).  The library
// walks the schedule exactly as tscode_amd/pipeline.py::sharded_step does -- passes below `min_pairs` whole on every rank, passes with at
// least `min_chunks_per_rank` chunks per rank partitioned by chunks (removed-row bits summed), the cache views summed once before the
// first pass of the other kind, the remaining large passes dealt by row tiles (best[] min-merged) -- and hands the host nothing but the
// collectives: `exchange(user, kind, buf, count)` must reduce the `count` elements at device address `buf` over the ranks IN PLACE, in
// stream order with the context's stream (enqueue it there, or synchronise on both sides), and return 0.  One process per GPU owns the
// communicator (RCCL through torch.distributed, or ncclAllReduce on the context's stream from a C host); the library opens none.
extern "C" __attribute__((visibility("default"))) int tsc_prune_run_sharded(tsc_prune *p, int rank, int world, int min_chunks_per_rank, int64_t min_pairs,
                                                                            void *exch_dev, int64_t exch_words, tsc_exchange_fn exchange, void *user,
                                                                            tsc_exchange_record *log, int log_cap, int *n_log) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank %d / world %d", rank, world);
    TSC_REQUIRE(world == 1 || exchange != nullptr, "tsc_prune_run_sharded: %d ranks and no exchange function", world);
    TSC_REQUIRE(min_chunks_per_rank >= 0 && log_cap >= 0 && (log || log_cap == 0), "bad argument");
    int logged = 0;
    if (n_log) *n_log = 0;
    auto xchg = [&](int kind, void *buf, int64_t count, int64_t k) -> int {
        if (log && logged < log_cap) log[logged] = tsc_exchange_record{k, kind, count};
        ++logged;
        if (n_log) *n_log = std::min(logged, log_cap);
        if (world == 1 && !exchange) return 0;
        const int rc = exchange(user, kind, buf, count);
        if (rc != 0) return fail(TSC_ERR_STATE, "tsc_prune_run_sharded: the exchange function returned %d (pass k = %lld, kind %d, %lld elements)", rc,
                                 (long long)k, kind, (long long)count);
        return 0;
    };
    const bool can_partition = world > 1 && min_chunks_per_rank > 0 && exch_dev != nullptr && p->algo == ALGO_SIEVE;
    if (can_partition) TSC_TRY(tsc_prune_set_partition(p, rank, world, min_chunks_per_rank, exch_dev, exch_words));
    for (;;) {
        int64_t k = 0;
        TSC_TRY(tsc_prune_run_replicated(p, world, min_pairs, &k));  // (every pass that needs no exchange; returns with the first that does, open)
        if (k == 0) break;
        if (pass_is_partitioned(p, k)) {
            // the whole pass on this rank's chunks; what the ranks tell each other is which rows they removed (+ the statistics)
            TSC_TRY(tsc_prune_pass_range(p));
            TSC_TRY(xchg(TSC_XCHG_SUM_I64, p->exch, int64_t(p->bit_words) + EXCH_STAT_WORDS, k));
            TSC_TRY(tsc_prune_pass_merge(p));
            continue;
        }
        if (p->cur.split && p->mode == 0) {
            // first pass after the partitioned ones: every rank needs every rank's cache keys from here on
            void *views = nullptr;
            int64_t off = 0, words = 0;
            TSC_TRY(tsc_prune_views_ptr(p, &views, &off, &words));
            if (words > 0) TSC_TRY(xchg(TSC_XCHG_SUM_I64, views, words, -k));
            TSC_TRY(tsc_prune_views_merged(p));
        }
        if (world > 1 && p->n * (p->n / k) / 2 >= min_pairs) {
            TSC_TRY(tsc_prune_pass_local(p, rank, world));  // this rank's row tiles only ...
            TSC_TRY(xchg(TSC_XCHG_MIN_I32, p->best, p->n, k));  // ... merged
        } else {
            TSC_TRY(tsc_prune_pass_local(p, 0, 1));  // (a small pass that only came back for the views' exchange)
        }
        TSC_TRY(tsc_prune_pass_finish(p));
    }
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_mask_dev(tsc_prune *p, const uint8_t **mask_dev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && mask_dev, "null argument");
    *mask_dev = p->mask;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_copy_mask_dev(tsc_prune *p, uint8_t *dst) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p && dst, "null argument");
    DeviceGuard guard(p->ctx->device);
    TSC_HIP(hipMemcpyAsync(dst, p->mask, size_t(p->n), hipMemcpyDeviceToDevice, p->ctx->stream));
    return 0;
    TSC_API_GUARD_END
}

// Close the last pass on the device, read the records back (the one synchronisation of a run) and build the
// per-pass statistics of the passes whose gate was open.
extern "C" __attribute__((visibility("default"))) int tsc_prune_stats(tsc_prune *p, tsc_pass_stats *stats, int *n_passes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(p != nullptr, "null argument");
    TSC_TRY(allowed(p, StepCall::Stats));
    tsc_ctx *c = p->ctx;
    DeviceGuard guard(c->device);
    if (!p->cur.exported) {
        hipStream_t st = c->stream;
        const Handover h = p->cur.close_for_export();  // the last pass was left open: close it, and open the one that follows where the run goes on
        if (h.how == Opener::Step) launch_pass_step(p, h);
        static_assert(sizeof(PassRecord) * TSC_MAX_PASSES <= 4096 && sizeof(PassRecord) % 8 == 0, "records fit the pinned staging buffer");
        {
            const int rec_words = int(sizeof(PassRecord) * TSC_MAX_PASSES / 8);
            const int64_t mask_words = p->export_mask_host ? p->n / 8 : 0;
            hipLaunchKernelGGL(k_export_run, dim3(grid_for(std::max<int64_t>(mask_words, rec_words), 256, 64)), dim3(256), 0, st,
                               reinterpret_cast<const unsigned long long *>(p->records), rec_words, static_cast<unsigned long long *>(c->pinned),
                               reinterpret_cast<const unsigned long long *>(p->mask), mask_words, (const uint8_t *)p->mask, p->n,
                               reinterpret_cast<unsigned long long *>(p->export_mask_host), (const unsigned *)p->dmax_bits);
            TSC_HIP(hipGetLastError());
            p->export_mask_host = nullptr;
        }
        TSC_HIP(hipStreamSynchronize(st));
        const PassRecord *rec = static_cast<const PassRecord *>(c->pinned);
        const bool nonfinite = unsigned(static_cast<const unsigned long long *>(c->pinned)[sizeof(PassRecord) * TSC_MAX_PASSES / 8]) >= 0x7f800000u;
        p->n_passes = 0;
        for (int slot = 0; slot < TSC_MAX_PASSES; ++slot) {
            if (!p->cur.ran[slot] || !rec[slot].on) continue;
            tsc_pass_stats &s = p->stats[p->n_passes++];
            memset(&s, 0, sizeof(s));
            s.k = rec[slot].k, s.n_active_before = rec[slot].n_before, s.n_active_after = rec[slot].n_after;
            s.pairs_evaluated = rec[slot].evaluated, s.pairs_computed = rec[slot].formed, s.candidates = rec[slot].exact;
            s.pairs_screened = rec[slot].screened, s.new_keys = rec[slot].removed, s.algo = rec[slot].algo;
            s.pairs_known = rec[slot].known;
            s.nonfinite_input = nonfinite ? 1 : 0;
            float ms = 0;
            if (c->opt.pass_timing >= 2 && hipEventElapsedTime(&ms, p->ev[slot][0], p->ev[slot][3]) == hipSuccess) s.gpu_ms = ms;
            if (c->opt.pass_timing >= (rec[slot].algo == ALGO_LOCAL ? 2 : 1) && hipEventElapsedTime(&ms, p->ev[slot][1], p->ev[slot][2]) == hipSuccess) s.tile_ms = ms;
        }
        p->cur.exported = true;
    }
    if (stats) memcpy(stats, p->stats, sizeof(tsc_pass_stats) * size_t(p->n_passes));
    if (n_passes) *n_passes = p->n_passes;
    return 0;
    TSC_API_GUARD_END
}

// One whole run on device data; mask_host (optional) also receives the verdicts, copied before the run's single
// synchronisation (the statistics read-back).
int prune_run(tsc_ctx *c, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask, uint8_t *mask_host,
                     tsc_pass_stats *stats, int *n_passes, const double *basis, const ExternalDescriptors *ext, int force_algo) {
    tsc_prune *p = nullptr;
    const bool in_place = (reinterpret_cast<uintptr_t>(mask) & 7u) == 0;  // run on the caller's buffer: no copy at the end
    TSC_TRY(prune_create_impl(c, heavy, n, h, rmsd_thr, mode, in_place ? mask : nullptr, &p, basis, ext, force_algo));
    int rc = 0;
    for (;;) {
        int64_t k = 0;
        if ((rc = tsc_prune_next_pass(p, &k)) != 0 || k == 0) break;
        if ((rc = tsc_prune_pass_local(p, 0, 1)) != 0) break;
        if ((rc = tsc_prune_pass_finish(p)) != 0) break;
    }
    if (!rc) {
        DeviceGuard guard(c->device);
        hipError_t e = in_place ? hipSuccess : hipMemcpyAsync(mask, p->mask, size_t(n), hipMemcpyDeviceToDevice, c->stream);
        // the verdicts go to the host with the statistics (one launch, k_export_run) when the buffer is pinned host memory the
        // device can write; any other pointer takes a copy command
        p->export_mask_host = nullptr;
        if (e == hipSuccess && mask_host) {
            hipPointerAttribute_t at;
            const bool mapped = (reinterpret_cast<uintptr_t>(mask_host) & 7u) == 0 && (reinterpret_cast<uintptr_t>(p->mask) & 7u) == 0 &&
                                hipPointerGetAttributes(&at, mask_host) == hipSuccess && at.type == hipMemoryTypeHost;
            // the address the DEVICE sees: for hipHostRegister'ed or non-mapped pinned memory it need not be the host address,
            // and may not exist at all
            uint8_t *dev_view = mapped ? static_cast<uint8_t *>(at.devicePointer) : nullptr;
            if (dev_view && (reinterpret_cast<uintptr_t>(dev_view) & 7u) == 0) {
                p->export_mask_host = dev_view;
            } else {
                (void)hipGetLastError();
                e = hipMemcpyAsync(mask_host, p->mask, size_t(n), hipMemcpyDeviceToHost, c->stream);
            }
        }
        if (e != hipSuccess) rc = fail(TSC_ERR_HIP, "mask copy failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = tsc_prune_stats(p, stats, n_passes);
    tsc_prune_destroy(p);
    return rc;
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_dev(tsc_ctx *c, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask,
                                  tsc_pass_stats *stats, int *n_passes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && heavy && mask, "tsc_prune_rmsd_dev: null argument");
    if (n == 0) {
        if (n_passes) *n_passes = 0;
        return 0;
    }
    return prune_run(c, heavy, n, h, rmsd_thr, mode, mask, nullptr, stats, n_passes);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd(tsc_ctx *c, const double *heavy, int64_t n, int h, double rmsd_thr, int mode, uint8_t *mask,
                              tsc_pass_stats *stats, int *n_passes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && heavy && mask, "tsc_prune_rmsd: null argument");
    TSC_REQUIRE(n >= 0 && h > 0, "bad sizes");
    if (n == 0) {
        if (n_passes) *n_passes = 0;
        return 0;
    }
    HostCall call(c);
    double *d_heavy;
    uint8_t *d_mask;
    TSC_TRY(call.in(heavy, size_t(n) * h * 3, &d_heavy));
    TSC_TRY(call.out(mask, size_t(n), &d_mask));
    TSC_TRY(tsc_prune_rmsd_dev(c, d_heavy, n, h, rmsd_thr, mode, d_mask, stats, n_passes));
    return call.finish();
    TSC_API_GUARD_END
}

// prune_conformers_rmsd as the reference calls it (rmsd_pruning.py:164-206): ALL atoms of every structure in host memory plus
// the indices of the heavy ones.  The heavy-atom gather `structures[:, atomnos != 1]` (:178-179) runs on the device: on the
// host it is a strided 40 MB copy that costs ten times the prune at 57k structures.
extern "C" __attribute__((visibility("default"))) int tsc_prune_structures(tsc_ctx *c, const double *structures, int64_t n, int n_atoms, const int32_t *heavy_idx,
                                                                           int n_heavy, double rmsd_thr, int mode, uint8_t *mask, tsc_pass_stats *stats,
                                                                           int *n_passes) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && heavy_idx && mask, "tsc_prune_structures: null argument");
    TSC_REQUIRE(n >= 0 && n_atoms > 0 && n_heavy > 0 && n_heavy <= n_atoms, "bad sizes");
    if (n == 0) {
        if (n_passes) *n_passes = 0;
        return 0;
    }
    HostCall call(c);
    double *d_all, *d_heavy;
    uint8_t *d_mask;
    TSC_TRY(call.in(structures, size_t(n) * n_atoms * 3, &d_all));
    TSC_TRY(call.scratch().get(size_t(n) * n_heavy * 3, &d_heavy));
    TSC_TRY(call.out(mask, size_t(n), &d_mask));
    TSC_TRY(tsc_gather_heavy_dev(c, d_all, nullptr, n, n_atoms, heavy_idx, n_heavy, d_heavy, nullptr));
    TSC_TRY(tsc_prune_rmsd_dev(c, d_heavy, n, n_heavy, rmsd_thr, mode, d_mask, stats, n_passes));
    return call.finish();
    TSC_API_GUARD_END
}

