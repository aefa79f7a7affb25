// cross.hip -- cross-set RMSD (cross.hpp): queries against a library as a matrix of values, as the first similar library member of every
// query, as the nearest library member of every query.  gfx950 only; there is no CPU implementation behind these entry points.
#include "call.hpp"
#include "cross.hpp"
#include "cross_reduce.hpp"
#include "host.hpp"

namespace {

template <int EPI>
void launch_general(hipStream_t st, dim3 grid, const CrossArgs &a) {
    hipLaunchKernelGGL((k_cross_general<EPI>), grid, dim3(64 * CX_WAVES), 0, st, a);
}
template <int HP>
void launch_tile_hp(int epi, hipStream_t st, dim3 grid, const CrossArgs &a) {
    switch (epi) {
        case CX_VALUES: hipLaunchKernelGGL((k_cross_tile<HP, CX_VALUES>), grid, dim3(64 * CX_WAVES), 0, st, a); break;
        case CX_FIRST: hipLaunchKernelGGL((k_cross_tile<HP, CX_FIRST>), grid, dim3(64 * CX_WAVES), 0, st, a); break;
        default: hipLaunchKernelGGL((k_cross_tile<HP, CX_NEAREST>), grid, dim3(64 * CX_WAVES), 0, st, a); break;
    }
}
// hp: cross_padded_atoms(h) -- 4 .. 32 in steps of 4, or 0 for the general path
int launch_cross(int hp, int epi, hipStream_t st, dim3 grid, const CrossArgs &a) {
    switch (hp) {
        case 0:
            if (epi == CX_VALUES) launch_general<CX_VALUES>(st, grid, a);
            else if (epi == CX_FIRST) launch_general<CX_FIRST>(st, grid, a);
            else launch_general<CX_NEAREST>(st, grid, a);
            break;
        case 4: launch_tile_hp<4>(epi, st, grid, a); break;
        case 8: launch_tile_hp<8>(epi, st, grid, a); break;
        case 12: launch_tile_hp<12>(epi, st, grid, a); break;
        case 16: launch_tile_hp<16>(epi, st, grid, a); break;
        case 20: launch_tile_hp<20>(epi, st, grid, a); break;
        case 24: launch_tile_hp<24>(epi, st, grid, a); break;
        case 28: launch_tile_hp<28>(epi, st, grid, a); break;
        case 32: launch_tile_hp<32>(epi, st, grid, a); break;
        default: return fail(TSC_ERR_INVALID, "unsupported padded atom count %d", hp);
    }
    TSC_HIP(hipGetLastError());
    return 0;
}

// One side of a call, packed on the device
struct Packed {
    double *Xr = nullptr, *Xc = nullptr, *G = nullptr;
    int64_t n = 0, ld = 0;
};

// rows / columns: which of the two layouts the side is read in (a library on the register path is read by rows only where survivors of the
// screen take the explicit rotation)
int pack_side(tsc_ctx *c, Scratch &s, const double *src, int64_t n, int n_atoms, const int32_t *idx, int h, int center, bool rows, bool columns, Packed *out) {
    const int pitch = cross_pitch(h);
    out->n = n, out->ld = cross_ld(n);
    if (rows) TSC_TRY(s.get(size_t(n) * pitch, &out->Xr));
    TSC_TRY(s.get(size_t(out->ld), &out->G));
    if (columns) TSC_TRY(s.get(size_t(out->ld) * pitch, &out->Xc));
    CrossPackArgs a;
    a.src = src, a.n = n, a.n_atoms = n_atoms, a.idx = idx, a.h = h, a.pitch = pitch, a.center = center;
    a.Xr = out->Xr, a.Xc = out->Xc, a.ld = out->ld, a.G = out->G;
    const size_t lds = columns ? size_t(64) * (pitch + 1) * sizeof(double) : 0;
    hipLaunchKernelGGL(k_cross_pack, dim3(grid_for(ceil_div<int64_t>(n, 64), 1, 1 << 20)), dim3(256), lds, c->stream, a);
    TSC_HIP(hipGetLastError());
    return 0;
}

struct CrossCall {
    const char *who;
    const double *queries;
    int64_t nq;
    const double *library;   // null: the queries themselves
    int64_t nl;
    int n_atoms;
    const int32_t *idx;      // device
    int n_idx;
    int center;
};

int check_sizes(const CrossCall &k) {
    TSC_REQUIRE(k.nq >= 0 && k.nq <= INT_MAX && k.nl >= 0 && k.nl <= INT_MAX, "%s: %lld queries, %lld library structures (0 .. 2^31 - 1 each)", k.who,
                (long long)k.nq, (long long)k.nl);
    TSC_REQUIRE(k.n_atoms >= 1, "%s: %d atoms", k.who, k.n_atoms);
    TSC_REQUIRE(k.idx ? (k.n_idx >= 1 && k.n_idx <= k.n_atoms) : k.n_idx == 0, "%s: %d compared atoms of %d (an index list has 1 .. n_atoms entries, none has 0)", k.who,
                k.n_idx, k.n_atoms);
    TSC_REQUIRE(k.library || k.nl == k.nq, "%s: no library: n_library must equal n_queries", k.who);
    return 0;
}

// Packs both sides and runs one epilogue on device data.  thr: CX_FIRST only.  out_r / out_m / out_i: the epilogue's outputs (device).
int cross_run(tsc_ctx *c, const CrossCall &k, int epi, double thr, double *out_r, double *out_m, int32_t *out_i) {
    Scratch s(c);
    const int h = k.idx ? k.n_idx : k.n_atoms;
    const int hp = cross_padded_atoms(h);
    Packed Q, L;
    TSC_TRY(pack_side(c, s, k.queries, k.nq, k.n_atoms, k.idx, h, k.center, true, hp != 0 && !k.library, &Q));
    if (k.library) TSC_TRY(pack_side(c, s, k.library, k.nl, k.n_atoms, k.idx, h, k.center, hp == 0 || epi == CX_FIRST, hp != 0, &L));
    else L = Q;
    const CrossPlan p = cross_plan(k.nq, k.nl);
    CrossArgs a;
    a.Lr = L.Xr, a.Lc = L.Xc, a.Lg = L.G, a.ld = L.ld, a.nl = k.nl;
    a.h = h, a.pitch = cross_pitch(h), a.seg_cols = p.seg_cols;
    a.thr = thr, a.maxdev_thr = 2.0 * thr, a.half_h_thr2 = 0.5 * double(h) * thr * thr;   // rmsd_pruning.py:75, :95
    if (epi == CX_FIRST) TSC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_i), INT_MAX, size_t(k.nq), c->stream));
    // the nearest epilogue walks the rows in blocks whose partial arrays stay within CX_PARTIAL_BYTES (one block for all but huge calls)
    const int64_t rows_per = epi == CX_NEAREST ? cross_nearest_rows(k.nq, p.n_seg) : k.nq;
    double *part_r = nullptr, *part_m = nullptr;
    int32_t *part_i = nullptr;
    if (epi == CX_NEAREST) {
        TSC_TRY(s.get(size_t(rows_per) * p.n_seg, &part_r));
        TSC_TRY(s.get(size_t(rows_per) * p.n_seg, &part_m));
        TSC_TRY(s.get(size_t(rows_per) * p.n_seg, &part_i));
    }
    for (int64_t lo = 0; lo < k.nq; lo += rows_per) {
        const int64_t rows = std::min(rows_per, k.nq - lo);
        a.Qr = Q.Xr + lo * a.pitch, a.Qg = Q.G + lo, a.nq = rows, a.n_tiles = ceil_div<int64_t>(rows, CX_ROWS);
        const unsigned gx = unsigned(std::min<int64_t>(ceil_div<int64_t>(a.n_tiles, CX_WAVES), CX_MAX_GROUPS_X));
        if (epi == CX_NEAREST) a.rmsd = part_r, a.maxdev = part_m, a.idx = part_i;
        else a.rmsd = out_r, a.maxdev = out_m, a.idx = out_i;
        TSC_TRY(launch_cross(hp, epi, c->stream, dim3(gx, unsigned(p.n_seg)), a));
        if (epi == CX_NEAREST) {
            hipLaunchKernelGGL(k_cross_nearest_reduce, dim3(grid_for(rows, 256)), dim3(256), 0, c->stream, part_r, part_m, part_i, p.n_seg, (long long)rows, out_i + lo,
                               out_r + lo, out_m + lo);
            TSC_HIP(hipGetLastError());
        }
    }
    return 0;
}

// the compared-atom list of a host-array call: checked here, before anything is uploaded
int check_idx_host(const CrossCall &k) {
    for (int e = 0; k.idx && e < k.n_idx; ++e)
        TSC_REQUIRE(k.idx[e] >= 0 && k.idx[e] < k.n_atoms, "%s: compared atom %d with %d atoms", k.who, k.idx[e], k.n_atoms);
    return 0;
}

// uploads of a host-array call: the two coordinate arrays and the index list, `k` rewritten to the device copies
int upload_sides(HostCall &call, CrossCall *k) {
    const double *dq = nullptr, *dl = nullptr;
    const int32_t *di = nullptr;
    TSC_TRY(call.in(k->queries, size_t(k->nq) * k->n_atoms * 3, &dq));
    if (k->library) TSC_TRY(call.in(k->library, size_t(k->nl) * k->n_atoms * 3, &dl));
    if (k->idx) TSC_TRY(call.in(k->idx, size_t(k->n_idx), &di));
    k->queries = dq, k->library = k->library ? dl : nullptr, k->idx = k->idx ? di : nullptr;
    return 0;
}

}  // namespace

// --------------------------------------------------------------------------------------------------
// values

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_rows(int64_t n_library, int64_t max_bytes, int64_t *rows) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(rows && n_library >= 0 && n_library <= INT_MAX && max_bytes >= 0, "tsc_rmsd_cross_rows: bad argument");
    *rows = cross_value_rows(INT_MAX, n_library, max_bytes);
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_dev(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library, int64_t n_library,
                                                                         int n_atoms, const int32_t *idx, int n_idx, int center, double *rmsd, double *maxdev,
                                                                         int64_t capacity) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && rmsd && maxdev, "tsc_rmsd_cross_dev: null argument");
    const CrossCall k{"tsc_rmsd_cross_dev", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    TSC_REQUIRE(capacity >= 0 && n_queries * n_library <= capacity, "tsc_rmsd_cross_dev: %lld x %lld values, room for %lld", (long long)n_queries,
                (long long)n_library, (long long)capacity);
    if (n_queries == 0 || n_library == 0) return 0;
    DeviceGuard guard(c->device);
    return cross_run(c, k, CX_VALUES, 0.0, rmsd, maxdev, nullptr);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library, int64_t n_library,
                                                                     int n_atoms, const int32_t *idx, int n_idx, int center, double *rmsd, double *maxdev,
                                                                     int64_t capacity) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && rmsd && maxdev, "tsc_rmsd_cross: null argument");
    CrossCall k{"tsc_rmsd_cross", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    TSC_TRY(check_idx_host(k));
    TSC_REQUIRE(capacity >= 0 && n_queries * n_library <= capacity, "tsc_rmsd_cross: %lld x %lld values, room for %lld", (long long)n_queries, (long long)n_library,
                (long long)capacity);
    if (n_queries == 0 || n_library == 0) return 0;
    HostCall call(c);
    double *d_r, *d_m;
    TSC_TRY(upload_sides(call, &k));
    TSC_TRY(call.out(rmsd, size_t(n_queries) * n_library, &d_r));
    TSC_TRY(call.out(maxdev, size_t(n_queries) * n_library, &d_m));
    TSC_TRY(cross_run(c, k, CX_VALUES, 0.0, d_r, d_m, nullptr));
    return call.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// first match

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_first_dev(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library,
                                                                               int64_t n_library, int n_atoms, const int32_t *idx, int n_idx, int center, double thr,
                                                                               int32_t *first) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && first, "tsc_rmsd_cross_first_dev: null argument");
    const CrossCall k{"tsc_rmsd_cross_first_dev", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    TSC_REQUIRE(std::isfinite(thr), "tsc_rmsd_cross_first_dev: thr is not finite");
    if (n_queries == 0) return 0;
    DeviceGuard guard(c->device);
    if (n_library == 0) {
        TSC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), INT_MAX, size_t(n_queries), c->stream));
        return 0;
    }
    return cross_run(c, k, CX_FIRST, thr, nullptr, nullptr, first);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_first(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library, int64_t n_library,
                                                                           int n_atoms, const int32_t *idx, int n_idx, int center, double thr, int32_t *first) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && first, "tsc_rmsd_cross_first: null argument");
    CrossCall k{"tsc_rmsd_cross_first", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    TSC_TRY(check_idx_host(k));
    TSC_REQUIRE(std::isfinite(thr), "tsc_rmsd_cross_first: thr is not finite");
    if (n_queries == 0) return 0;
    if (n_library == 0) {
        for (int64_t q = 0; q < n_queries; ++q) first[q] = INT_MAX;
        return 0;
    }
    HostCall call(c);
    int32_t *d_f;
    TSC_TRY(upload_sides(call, &k));
    TSC_TRY(call.out(first, size_t(n_queries), &d_f));
    TSC_TRY(cross_run(c, k, CX_FIRST, thr, nullptr, nullptr, d_f));
    return call.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// nearest

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_nearest_dev(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library,
                                                                                 int64_t n_library, int n_atoms, const int32_t *idx, int n_idx, int center,
                                                                                 int32_t *index, double *rmsd, double *maxdev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && index && rmsd && maxdev, "tsc_rmsd_cross_nearest_dev: null argument");
    const CrossCall k{"tsc_rmsd_cross_nearest_dev", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    if (n_queries == 0) return 0;
    TSC_REQUIRE(n_library >= 1, "tsc_rmsd_cross_nearest_dev: an empty library has no nearest member");
    DeviceGuard guard(c->device);
    return cross_run(c, k, CX_NEAREST, 0.0, rmsd, maxdev, index);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rmsd_cross_nearest(tsc_ctx *c, const double *queries, int64_t n_queries, const double *library,
                                                                             int64_t n_library, int n_atoms, const int32_t *idx, int n_idx, int center, int32_t *index,
                                                                             double *rmsd, double *maxdev) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && queries && index && rmsd && maxdev, "tsc_rmsd_cross_nearest: null argument");
    CrossCall k{"tsc_rmsd_cross_nearest", queries, n_queries, library, n_library, n_atoms, idx, n_idx, center};
    TSC_TRY(check_sizes(k));
    TSC_TRY(check_idx_host(k));
    if (n_queries == 0) return 0;
    TSC_REQUIRE(n_library >= 1, "tsc_rmsd_cross_nearest: an empty library has no nearest member");
    HostCall call(c);
    int32_t *d_i;
    double *d_r, *d_m;
    TSC_TRY(upload_sides(call, &k));
    TSC_TRY(call.out(index, size_t(n_queries), &d_i));
    TSC_TRY(call.out(rmsd, size_t(n_queries), &d_r));
    TSC_TRY(call.out(maxdev, size_t(n_queries), &d_m));
    TSC_TRY(cross_run(c, k, CX_NEAREST, 0.0, d_r, d_m, d_i));
    return call.finish();
    TSC_API_GUARD_END
}
