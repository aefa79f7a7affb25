// leader.hip -- the energy-ordered RMSD prune (leader.hpp): keep a row iff no row kept before it in the order is similar to it; every
// cluster collapses to its first member.  gfx950 only; there is no CPU implementation behind these entry points.
#include "call.hpp"
#include "cross.hpp"
#include "gather_rows.hpp"
#include "host.hpp"
#include "leader.hpp"

namespace {

// the CX_FIRST rectangle of cross.hpp for hp = cross_padded_atoms(h) (0: the general path)
int launch_first(int hp, hipStream_t st, dim3 grid, const CrossArgs &a) {
    const dim3 block(64 * CX_WAVES);
    switch (hp) {
        case 0: hipLaunchKernelGGL((k_cross_general<CX_FIRST>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_cross_tile<4, CX_FIRST>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_cross_tile<8, CX_FIRST>), grid, block, 0, st, a); break;
        case 12: hipLaunchKernelGGL((k_cross_tile<12, CX_FIRST>), grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL((k_cross_tile<16, CX_FIRST>), grid, block, 0, st, a); break;
        case 20: hipLaunchKernelGGL((k_cross_tile<20, CX_FIRST>), grid, block, 0, st, a); break;
        case 24: hipLaunchKernelGGL((k_cross_tile<24, CX_FIRST>), grid, block, 0, st, a); break;
        case 28: hipLaunchKernelGGL((k_cross_tile<28, CX_FIRST>), grid, block, 0, st, a); break;
        case 32: hipLaunchKernelGGL((k_cross_tile<32, CX_FIRST>), grid, block, 0, st, a); break;
        default: return fail(TSC_ERR_INVALID, "unsupported padded atom count %d", hp);
    }
    TSC_HIP(hipGetLastError());
    return 0;
}

struct LeaderCall {
    const char *who;
    const double *structures;
    int64_t n;
    const double *library;   // null: none
    int64_t nl;
    int n_atoms;
    const int32_t *idx;      // device
    int n_idx;
    int center;
    const int32_t *order;    // device, or null: the rows as they lie
    double thr;
};

int check_sizes(const LeaderCall &k) {
    TSC_REQUIRE(k.n >= 0 && k.n <= INT_MAX && k.nl >= 0 && k.nl <= INT_MAX && k.n + k.nl <= INT_MAX,
                "%s: %lld structures, %lld library structures (0 .. 2^31 - 1 each and together)", k.who, (long long)k.n, (long long)k.nl);
    TSC_REQUIRE(k.library || k.nl == 0, "%s: no library: n_library must be 0", k.who);
    TSC_REQUIRE(k.n_atoms >= 1, "%s: %d atoms", k.who, k.n_atoms);
    TSC_REQUIRE(k.idx ? (k.n_idx >= 1 && k.n_idx <= k.n_atoms) : k.n_idx == 0, "%s: %d compared atoms of %d (an index list has 1 .. n_atoms entries, none has 0)", k.who,
                k.n_idx, k.n_atoms);
    TSC_REQUIRE(std::isfinite(k.thr), "%s: thr is not finite", k.who);
    return 0;
}

int pack(tsc_ctx *c, const double *src, int64_t n, const LeaderCall &k, int h, double *Xr, double *Xc, int64_t ld, double *G) {
    CrossPackArgs a;
    a.src = src, a.n = n, a.n_atoms = k.n_atoms, a.idx = k.idx, a.h = h, a.pitch = cross_pitch(h), a.center = k.center;
    a.Xr = Xr, a.Xc = Xc, a.ld = ld, a.G = G;
    const size_t lds = Xc ? size_t(64) * (a.pitch + 1) * sizeof(double) : 0;
    hipLaunchKernelGGL(k_cross_pack, dim3(grid_for(ceil_div<int64_t>(n, 64), 1, 1 << 20)), dim3(256), lds, c->stream, a);
    TSC_HIP(hipGetLastError());
    return 0;
}

// Everything on the device but *n_kept.  Waits for the stream once per block (the kept count sizes the next block's library walk), so the
// outputs are complete when it returns.
int leader_run(tsc_ctx *c, Scratch &s, const LeaderCall &k, uint8_t *mask, int32_t *rep, int32_t *lib_rep, int64_t *n_kept) {
    const int h = k.idx ? k.n_idx : k.n_atoms;
    const int hp = cross_padded_atoms(h);
    const int pitch = cross_pitch(h);
    // 1. the ensemble in order, row-major, with its norms
    double *Er, *Eg;
    TSC_TRY(s.get(size_t(k.n) * pitch, &Er));
    TSC_TRY(s.get(size_t(cross_ld(k.n)), &Eg));
    if (k.order) {
        double *ordered;
        TSC_TRY(s.get(size_t(k.n) * k.n_atoms * 3, &ordered));
        TSC_TRY(launch_gather_rows(c->stream, k.structures, k.order, k.n, k.n_atoms * 3, nullptr, k.n_atoms * 3, ordered));
        TSC_TRY(pack(c, ordered, k.n, k, h, Er, nullptr, cross_ld(k.n), Eg));
        s.give_back(ordered);   // (the cache is stream-ordered)
    } else {
        TSC_TRY(pack(c, k.structures, k.n, k, h, Er, nullptr, cross_ld(k.n), Eg));
    }
    // 2. the pack everything kept goes to: the caller's library in front
    const int64_t capacity = leader_capacity(k.nl, k.n), ld = leader_ld(k.nl, k.n);
    double *Lr, *Lc = nullptr, *Lg;
    TSC_TRY(s.get(size_t(capacity) * pitch, &Lr));
    TSC_TRY(s.get(size_t(ld), &Lg));
    TSC_HIP(hipMemsetAsync(Lg, 0, size_t(ld) * sizeof(double), c->stream));
    if (hp) {
        TSC_TRY(s.get(size_t(ld) * pitch, &Lc));
        TSC_HIP(hipMemsetAsync(Lc, 0, size_t(ld) * pitch * sizeof(double), c->stream));
    }
    if (k.nl) TSC_TRY(pack(c, k.library, k.nl, k, h, Lr, Lc, ld, Lg));
    // 3. the blocks
    int32_t *first, *kept_src, *acc_pos, *count;
    unsigned long long *bits;
    TSC_TRY(s.get(size_t(k.n), &first));
    TSC_TRY(s.get(size_t(k.n), &kept_src));
    TSC_TRY(s.get(size_t(LEADER_BLOCK), &acc_pos));
    TSC_TRY(s.get(size_t(1), &count));
    TSC_TRY(s.get(size_t(LEADER_BLOCK) * LEADER_WORDS, &bits));
    TSC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), INT_MAX, size_t(k.n), c->stream));
    const int64_t n_blocks = leader_blocks(k.n);
    int32_t kept = 0;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t b0 = b * LEADER_BLOCK;
        const int nb = leader_block_rows(k.n, b);
        const int64_t nl = k.nl + kept;
        if (nl > 0) {   // (a) the block against the pack so far
            const CrossPlan p = cross_plan(nb, nl);
            CrossArgs a;
            a.Qr = Er + b0 * pitch, a.Qg = Eg + b0, a.nq = nb, a.n_tiles = p.n_tiles;
            a.Lr = Lr, a.Lc = Lc, a.Lg = Lg, a.ld = ld, a.nl = nl;
            a.h = h, a.pitch = pitch, a.seg_cols = p.seg_cols;
            a.thr = k.thr, a.maxdev_thr = 2.0 * k.thr, a.half_h_thr2 = 0.5 * double(h) * k.thr * k.thr;   // rmsd_pruning.py:75, :95
            a.rmsd = a.maxdev = nullptr, a.idx = first + b0;
            TSC_TRY(launch_first(hp, c->stream, dim3(p.grid_x, unsigned(p.n_seg)), a));
        }
        {   // (b) the open rows against the open rows before them
            LeaderBitsArgs a;
            a.Xr = Er + b0 * pitch, a.first = first + b0, a.nb = nb, a.h = h, a.pitch = pitch;
            a.thr = k.thr, a.maxdev_thr = 2.0 * k.thr, a.half_h_thr2 = 0.5 * double(h) * k.thr * k.thr;
            a.bits = bits;
            const LeaderBitsGrid g = leader_bits_grid(nb);
            hipLaunchKernelGGL(k_leader_bits, dim3(g.x, g.y), dim3(64 * LD_WAVES), 0, c->stream, a);
            TSC_HIP(hipGetLastError());
        }
        {   // (c) the order replayed on the bits
            LeaderReplayArgs a;
            a.bits = bits, a.first = first + b0, a.order = k.order, a.n = k.n, a.b0 = b0, a.nb = nb, a.n_library = int(k.nl), a.kept_before = kept;
            a.kept_src = kept_src, a.acc_pos = acc_pos, a.count = count, a.mask = mask, a.rep = rep, a.lib_rep = lib_rep;
            hipLaunchKernelGGL(k_leader_replay, dim3(1), dim3(64), 0, c->stream, a);
            TSC_HIP(hipGetLastError());
        }
        if (b + 1 < n_blocks) {   // (d) the accepted rows join the pack
            LeaderAppendArgs a;
            a.Er = Er + b0 * pitch, a.Eg = Eg + b0, a.acc_pos = acc_pos, a.count = count, a.kept_before = kept, a.nl = nl, a.capacity = capacity;
            a.pitch = pitch, a.Lr = Lr, a.Lc = Lc, a.Lg = Lg, a.ld = ld;
            hipLaunchKernelGGL(k_leader_append, dim3(nb), dim3(128), 0, c->stream, a);
            TSC_HIP(hipGetLastError());
        }
        TSC_TRY(read_i32(c, count, &kept));   // the one wait of a block
        TSC_REQUIRE(kept >= 0 && kept <= b0 + nb, "%s: the device reports %d rows kept of %lld", k.who, kept, (long long)(b0 + nb));
    }
    *n_kept = kept;
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_leader_block(void) {
    TSC_API_GUARD_BEGIN
    return LEADER_BLOCK;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_ordered_dev(tsc_ctx *c, const double *structures, int64_t n, const double *library, int64_t n_library,
                                                                                 int n_atoms, const int32_t *idx, int n_idx, int center, const int32_t *order,
                                                                                 double thr, uint8_t *mask, int32_t *rep, int32_t *lib_rep, int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && mask && rep && lib_rep && n_kept, "tsc_prune_rmsd_ordered_dev: null argument");
    const LeaderCall k{"tsc_prune_rmsd_ordered_dev", structures, n, library, n_library, n_atoms, idx, n_idx, center, order, thr};
    TSC_TRY(check_sizes(k));
    *n_kept = 0;
    if (n == 0) return 0;
    DeviceGuard guard(c->device);
    Scratch s(c);
    return leader_run(c, s, k, mask, rep, lib_rep, n_kept);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_prune_rmsd_ordered(tsc_ctx *c, const double *structures, int64_t n, const double *library, int64_t n_library,
                                                                             int n_atoms, const int32_t *idx, int n_idx, int center, const int32_t *order, double thr,
                                                                             uint8_t *mask, int32_t *rep, int32_t *lib_rep, int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && mask && rep && lib_rep && n_kept, "tsc_prune_rmsd_ordered: null argument");
    LeaderCall k{"tsc_prune_rmsd_ordered", structures, n, library, n_library, n_atoms, idx, n_idx, center, order, thr};
    TSC_TRY(check_sizes(k));
    for (int e = 0; idx && e < n_idx; ++e) TSC_REQUIRE(idx[e] >= 0 && idx[e] < n_atoms, "tsc_prune_rmsd_ordered: compared atom %d with %d atoms", idx[e], n_atoms);
    if (order) {   // a permutation of 0 .. n - 1
        std::vector<bool> seen(size_t(n), false);
        for (int64_t i = 0; i < n; ++i) {
            TSC_REQUIRE(order[i] >= 0 && order[i] < n && !seen[size_t(order[i])], "tsc_prune_rmsd_ordered: order[%lld] = %d: not a permutation of 0 .. %lld",
                        (long long)i, order[i], (long long)n - 1);
            seen[size_t(order[i])] = true;
        }
    }
    *n_kept = 0;
    if (n == 0) return 0;
    HostCall call(c);
    TSC_TRY(call.in(structures, size_t(n) * n_atoms * 3, &k.structures));
    if (n_library) TSC_TRY(call.in(library, size_t(n_library) * n_atoms * 3, &k.library));
    else k.library = nullptr;
    if (idx) TSC_TRY(call.in(idx, size_t(n_idx), &k.idx));
    if (order) TSC_TRY(call.in(order, size_t(n), &k.order));
    uint8_t *d_mask;
    int32_t *d_rep, *d_lib;
    TSC_TRY(call.out(mask, size_t(n), &d_mask));
    TSC_TRY(call.out(rep, size_t(n), &d_rep));
    TSC_TRY(call.out(lib_rep, size_t(n), &d_lib));
    TSC_TRY(leader_run(c, call.scratch(), k, d_mask, d_rep, d_lib, n_kept));
    return call.finish();
    TSC_API_GUARD_END
}
