// diverse.hip -- launches and C ABI of ensemble alignment, k-means and the diverse-conformer pick (diverse.hpp;
// tscode/hypermolecule_class.py:38-72, tscode/torsion_module.py:849-924).  gfx950 only.  There is deliberately no CPU implementation
// behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "diverse_kernels.hpp"

#include <algorithm>
#include <climits>

namespace {

using namespace tsc;

// stage times of the calling thread's latest call (every entry resets them), taken only under the context option "pass_timing" >= 1 (tools/diverse_profile.py):
// align, the first k_kmeans_assign launch, the first k_kmeans_update launch, the whole device part of the call
thread_local float g_times[4] = {-1.f, -1.f, -1.f, -1.f};

void reset_times() {
    for (float &t : g_times) t = -1.f;
}

int align_dev(tsc_ctx *c, HostCall &h, const double *d_in, int64_t N, int n, const int32_t *idx_host, int n_idx, double *d_out) {
    int32_t *d_idx = nullptr;
    if (idx_host && n_idx > 0) {
        for (int q = 0; q < n_idx; ++q) TSC_REQUIRE(idx_host[q] >= 0 && idx_host[q] < n, "align_structures: index %d out of range", idx_host[q]);
        TSC_TRY(h.in(idx_host, size_t(n_idx), &d_idx));
    } else {
        n_idx = n;   // hypermolecule_class.py:51
    }
    hipLaunchKernelGGL(k_align_structures, dim3(unsigned(ceil_div<int64_t>(N, 4))), dim3(256), 0, c->stream, d_in, N, n, d_idx, n_idx, d_out);
    TSC_HIP(hipGetLastError());
    return 0;
}

// column sums (squares != 0: of the squares) of X[N, D] times `scale`, into d_out[D]
int col_stats(tsc_ctx *c, Scratch &s, const double *X, int64_t N, int D, int squares, double scale, double *d_out) {
    const int chunks = int(std::max<int64_t>(1, std::min<int64_t>(64, N / 256)));
    double *part;
    TSC_TRY(s.get(size_t(chunks) * D, &part));
    hipLaunchKernelGGL(k_col_partial, dim3(ceil_div(D, 64), chunks), dim3(256), 0, c->stream, X, N, D, squares, part);
    TSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_col_finish, dim3(ceil_div(D, 256)), dim3(256), 0, c->stream, part, chunks, D, scale, d_out);
    TSC_HIP(hipGetLastError());
    return 0;
}

// X -= X.mean(0) in place; d_mean[D] the mean; *tol_abs = mean(var(X, axis = 0)) * tol  (scikit-learn's _tolerance)
int centre_features(tsc_ctx *c, Scratch &s, double *X, int64_t N, int D, double *d_mean, double tol, double *tol_abs) {
    TSC_TRY(col_stats(c, s, X, N, D, 0, 1.0 / double(N), d_mean));
    hipLaunchKernelGGL(k_shift_cols, dim3(grid_for(N * D, 256)), dim3(256), 0, c->stream, X, N, D, d_mean, -1.0);
    TSC_HIP(hipGetLastError());
    double *var, *mv;
    TSC_TRY(s.get(size_t(D), &var));
    TSC_TRY(s.get(1, &mv));
    TSC_TRY(col_stats(c, s, X, N, D, 1, 1.0 / double(N), var));
    hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(1024), 0, c->stream, var, int64_t(D), 1.0 / double(D), mv);
    TSC_HIP(hipGetLastError());
    double h = 0.0;
    TSC_HIP(hipMemcpyAsync(&h, mv, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    *tol_abs = h * tol;
    return 0;
}

struct Lloyd {   // device state of one clustering; every block belongs to the caller's Scratch
    double *X = nullptr, *C = nullptr, *xn = nullptr, *cn = nullptr, *own_d2 = nullptr, *shift_part = nullptr;
    int32_t *labels = nullptr, *counts = nullptr, *offs = nullptr, *members = nullptr;
    int *changed = nullptr;
    KmControl *ctl = nullptr;
    int64_t N = 0;
    int D = 0, k = 0, slices = 0;
};

int lloyd_alloc(tsc_ctx *c, Scratch &s, Lloyd &L, double *X, int64_t N, int D, int k) {
    L.X = X, L.N = N, L.D = D, L.k = k, L.slices = ceil_div(D, 64);
    TSC_TRY(s.get(size_t(k) * D, &L.C));
    TSC_TRY(s.get(size_t(N), &L.xn));
    TSC_TRY(s.get(size_t(k), &L.cn));
    TSC_TRY(s.get(size_t(N), &L.own_d2));
    TSC_TRY(s.get(size_t(k) * L.slices, &L.shift_part));
    TSC_TRY(s.get(size_t(N), &L.labels));
    TSC_TRY(s.get(size_t(k), &L.counts));
    TSC_TRY(s.get(size_t(k) + 1, &L.offs));
    TSC_TRY(s.get(size_t(N), &L.members));
    TSC_TRY(s.get(1, &L.changed));
    TSC_TRY(s.get(1, &L.ctl));
    return 0;
}

int assign(tsc_ctx *c, Lloyd &L, StageTimer *tm = nullptr) {
    const int tiles = ceil_div(L.k, 16), blocks = ceil_div(tiles, 8), nt = ceil_div(tiles, blocks);
    hipLaunchKernelGGL(k_row_norms, dim3(ceil_div(L.k, 4)), dim3(256), 0, c->stream, L.C, int64_t(L.k), L.D, L.cn);
    TSC_HIP(hipMemsetAsync(L.changed, 0, sizeof(int), c->stream));
    if (tm) tm->begin();   // (the k_kmeans_assign launch alone)
    with_width(nt, [&](auto w) {
        hipLaunchKernelGGL(k_kmeans_assign<decltype(w)::value>, dim3(unsigned(ceil_div<int64_t>(L.N, KA_ROWS))), dim3(256), 0, c->stream, L.X, L.N, L.D,
                           L.C, L.k, L.xn, L.cn, L.labels, L.own_d2, L.changed);
    });
    if (tm) tm->end(&g_times[1]);
    TSC_HIP(hipGetLastError());
    return 0;
}

int bucket(tsc_ctx *c, Lloyd &L) {
    hipLaunchKernelGGL(k_label_count, dim3(L.k), dim3(256), 0, c->stream, L.labels, L.N, L.counts);
    hipLaunchKernelGGL(k_label_bucket, dim3(L.k), dim3(256), 0, c->stream, L.labels, L.N, L.counts, L.k, L.offs, L.members);
    TSC_HIP(hipGetLastError());
    return 0;
}

// The Lloyd loop of scikit-learn's KMeans(init = <array>, n_init = 1, algorithm = "lloyd") on centred X and centred C (what
// torsion_module.py:889-890 runs); the loop control is on the host, with one 16-byte read-back per iteration.  On return the labels
// are consistent with the final centres and counts / offs / members describe them.
int lloyd_run(tsc_ctx *c, Lloyd &L, int max_iter, double tol_abs, int *n_iter, int *max_empty, StageTimer *tm) {
    hipLaunchKernelGGL(k_row_norms, dim3(unsigned(ceil_div<int64_t>(L.N, 4))), dim3(256), 0, c->stream, L.X, L.N, L.D, L.xn);
    TSC_HIP(hipMemsetAsync(L.labels, 0xff, size_t(L.N) * sizeof(int32_t), c->stream));
    bool strict = false;
    int it = 0, worst = 0;
    for (; it < max_iter; ++it) {
        const bool timed = tm && it == 0;
        TSC_TRY(assign(c, L, timed ? tm : nullptr));
        TSC_TRY(bucket(c, L));
        hipLaunchKernelGGL(k_own_d2, dim3(unsigned(ceil_div<int64_t>(L.N, 4))), dim3(256), 0, c->stream, L.X, L.N, L.D, L.C, L.labels, L.counts, L.k, 1,
                           L.own_d2);
        hipLaunchKernelGGL(k_kmeans_relocate, dim3(1), dim3(256), 0, c->stream, L.own_d2, L.N, L.labels, L.counts, L.k, L.ctl);
        if (timed) tm->begin();
        hipLaunchKernelGGL(k_kmeans_update, dim3(L.k, L.slices), dim3(256), 0, c->stream, L.X, L.D, L.members, L.offs, L.counts, L.ctl, L.C,
                           L.shift_part);
        if (timed) tm->end(&g_times[2]);
        hipLaunchKernelGGL(k_kmeans_control, dim3(1), dim3(64), 0, c->stream, L.shift_part, L.k * L.slices, L.changed, L.ctl);
        TSC_HIP(hipGetLastError());
        struct {
            int changed, n_empty;
            double shift;
        } h;
        static_assert(sizeof(h) == 16 && offsetof(KmControl, shift) == 8, "the head of KmControl");
        TSC_HIP(hipMemcpyAsync(&h, L.ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        TSC_HIP(hipStreamSynchronize(c->stream));
        worst = std::max(worst, h.n_empty);
        if (h.changed == 0) {   // labels == labels of the iteration before: strict convergence
            strict = true;
            ++it;
            break;
        }
        if (h.shift <= tol_abs) {
            ++it;
            break;
        }
    }
    if (!strict) {
        TSC_TRY(assign(c, L));
        TSC_TRY(bucket(c, L));
    }
    *n_iter = std::min(it, max_iter);
    if (max_empty) *max_empty = worst;
    return 0;
}

// k-means++ without local trials on X[N, D]: d_rows[k] on the device (tsc_kmeans_seed in the header); u_host checked by the caller
int seed_dev(tsc_ctx *c, HostCall &h, const double *X, int64_t N, int D, int k, const double *u_host, int32_t *d_rows) {
    double *d_u, *min_d2;
    TSC_TRY(h.in(u_host, size_t(k), &d_u));
    TSC_TRY(h.scratch().get(size_t(N), &min_d2));
    const int32_t first = int32_t(std::min<int64_t>(N - 1, int64_t(u_host[0] * double(N))));
    TSC_HIP(hipMemcpyAsync(d_rows, &first, sizeof(first), hipMemcpyHostToDevice, c->stream));
    for (int j = 1; j < k; ++j) {
        hipLaunchKernelGGL(k_kmeans_seed_update, dim3(unsigned(ceil_div<int64_t>(N, 4))), dim3(256), 0, c->stream, X, N, D, d_rows, j - 1, min_d2);
        hipLaunchKernelGGL(k_kmeans_seed_pick, dim3(1), dim3(1024), 0, c->stream, min_d2, N, d_u, j, d_rows);
    }
    TSC_HIP(hipGetLastError());
    TSC_HIP(hipStreamSynchronize(c->stream));   // (`first` is a stack variable)
    return 0;
}

int pick_dev(tsc_ctx *c, const Lloyd &L, const double *X, const double *C, const double *d_energies, int32_t *d_picked) {
    hipLaunchKernelGGL(k_diverse_pick, dim3(L.k), dim3(256), 0, c->stream, X, L.D / 3, L.members, L.offs, L.counts, C, L.k, d_energies, d_picked);
    TSC_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_diverse_timings(tsc_ctx *c, float *ms4) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms4, "tsc_diverse_timings: null argument");
    for (int q = 0; q < 4; ++q) ms4[q] = g_times[q];
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_align_structures(tsc_ctx *c, const double *structures, int64_t n_structs, int n_atoms,
                                                                           const int32_t *indices, int n_idx, double *out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && out, "tsc_align_structures: null argument");
    TSC_REQUIRE(n_idx >= 0 && (n_idx == 0 || indices), "tsc_align_structures: %d indices without an index array", n_idx);
    TSC_TRY(check_shape("tsc_align_structures", n_structs, n_atoms));
    TSC_REQUIRE(n_idx <= n_atoms, "tsc_align_structures: %d indices for %d atoms", n_idx, n_atoms);
    TSC_TRY(check_finite("tsc_align_structures", "structures", structures, size_t(n_structs) * n_atoms * 3));
    reset_times();
    HostCall h(c);
    const size_t count = size_t(n_structs) * n_atoms * 3;
    double *d_in, *d_out;
    TSC_TRY(h.in(structures, count, &d_in));
    TSC_TRY(h.out(out, count, &d_out));
    StageTimer tm(c);
    tm.begin();
    TSC_TRY(align_dev(c, h, d_in, n_structs, n_atoms, indices, n_idx, d_out));
    tm.end(&g_times[0]);
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_kmeans_lloyd(tsc_ctx *c, const double *X, int64_t N, int64_t D, const double *init, int k,
                                                                       int max_iter, double tol, int32_t *labels, double *centers, double *inertia,
                                                                       int *n_iter, int *max_empty) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && X && init && labels && centers && inertia && n_iter, "tsc_kmeans_lloyd: null argument");
    TSC_TRY(check_k("tsc_kmeans_lloyd", N, D, k));
    TSC_REQUIRE(max_iter >= 1 && std::isfinite(tol) && tol >= 0.0, "tsc_kmeans_lloyd: max_iter = %d, tol = %g", max_iter, tol);
    TSC_TRY(check_finite("tsc_kmeans_lloyd", "X", X, size_t(N) * D));
    TSC_TRY(check_finite("tsc_kmeans_lloyd", "init", init, size_t(k) * D));
    reset_times();
    HostCall h(c);
    Scratch &s = h.scratch();
    double *d_X, *d_mean, *d_in;
    TSC_TRY(h.in(X, size_t(N) * D, &d_X));
    TSC_TRY(s.get(size_t(D), &d_mean));
    double tol_abs = 0.0;
    TSC_TRY(centre_features(c, s, d_X, N, int(D), d_mean, tol, &tol_abs));
    Lloyd L;
    TSC_TRY(lloyd_alloc(c, s, L, d_X, N, int(D), k));
    TSC_HIP(hipMemcpyAsync(L.C, init, size_t(k) * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_shift_cols, dim3(grid_for(int64_t(k) * D, 256)), dim3(256), 0, c->stream, L.C, int64_t(k), int(D), d_mean, -1.0);
    StageTimer tm(c);
    TSC_TRY(lloyd_run(c, L, max_iter, tol_abs, n_iter, max_empty, tm.on ? &tm : nullptr));
    // inertia by direct differences, summed in row order
    TSC_TRY(s.get(1, &d_in));
    hipLaunchKernelGGL(k_own_d2, dim3(unsigned(ceil_div<int64_t>(N, 4))), dim3(256), 0, c->stream, L.X, N, int(D), L.C, L.labels, L.counts, k, 0, L.own_d2);
    hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(1024), 0, c->stream, L.own_d2, N, 1.0, d_in);
    hipLaunchKernelGGL(k_shift_cols, dim3(grid_for(int64_t(k) * D, 256)), dim3(256), 0, c->stream, L.C, int64_t(k), int(D), d_mean, 1.0);
    TSC_HIP(hipGetLastError());
    TSC_TRY(h.fetch(labels, L.labels, size_t(N)));
    TSC_TRY(h.fetch(centers, L.C, size_t(k) * D));
    TSC_TRY(h.fetch(inertia, d_in, 1));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_kmeans_seed(tsc_ctx *c, const double *X, int64_t N, int64_t D, int k, const double *u,
                                                                      int32_t *rows) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && X && u && rows, "tsc_kmeans_seed: null argument");
    TSC_TRY(check_k("tsc_kmeans_seed", N, D, k));
    TSC_TRY(check_uniforms("tsc_kmeans_seed", u, k));
    TSC_TRY(check_finite("tsc_kmeans_seed", "X", X, size_t(N) * D));
    reset_times();
    HostCall h(c);
    double *d_X;
    int32_t *d_rows;
    TSC_TRY(h.in(X, size_t(N) * D, &d_X));
    TSC_TRY(h.out(rows, size_t(k), &d_rows));
    TSC_TRY(seed_dev(c, h, d_X, N, int(D), k, u, d_rows));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_diverse_pick(tsc_ctx *c, const double *aligned, int64_t N, int n_atoms, const int32_t *labels,
                                                                       const double *centers, int k, const double *energies, int32_t *picked) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && aligned && labels && centers && picked, "tsc_diverse_pick: null argument");
    TSC_TRY(check_shape("tsc_diverse_pick", N, n_atoms));
    TSC_REQUIRE(k >= 1 && k <= DV_MAX_K, "tsc_diverse_pick: %d clusters (1 .. %d)", k, DV_MAX_K);
    for (int64_t i = 0; i < N; ++i) TSC_REQUIRE(labels[i] >= 0 && labels[i] < k, "tsc_diverse_pick: label %d of row %lld out of range", labels[i], (long long)i);
    TSC_TRY(check_finite("tsc_diverse_pick", "aligned", aligned, size_t(N) * n_atoms * 3));
    TSC_TRY(check_finite("tsc_diverse_pick", "centers", centers, size_t(k) * n_atoms * 3));
    if (energies)
        for (int64_t i = 0; i < N; ++i) TSC_REQUIRE(!std::isnan(energies[i]), "tsc_diverse_pick: energies[%lld] is NaN", (long long)i);
    reset_times();
    HostCall h(c);
    Scratch &s = h.scratch();
    const int D = 3 * n_atoms;
    double *d_X, *d_C, *d_e = nullptr;
    int32_t *d_picked;
    TSC_TRY(h.in(aligned, size_t(N) * D, &d_X));
    TSC_TRY(h.in(centers, size_t(k) * D, &d_C));
    if (energies) TSC_TRY(h.in(energies, size_t(N), &d_e));
    Lloyd L;
    L.N = N, L.D = D, L.k = k;
    TSC_TRY(h.in(labels, size_t(N), &L.labels));
    TSC_TRY(s.get(size_t(k), &L.counts));
    TSC_TRY(s.get(size_t(k) + 1, &L.offs));
    TSC_TRY(s.get(size_t(N), &L.members));
    TSC_TRY(h.out(picked, size_t(k), &d_picked));
    TSC_TRY(bucket(c, L));
    TSC_TRY(pick_dev(c, L, d_X, d_C, d_e, d_picked));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_diverse_select(tsc_ctx *c, const double *structures, int64_t N, int n_atoms,
                                                                         int32_t *init_rows, const double *u, int k, const double *energies,
                                                                         int max_iter, double tol, double *aligned_out, int32_t *labels,
                                                                         int32_t *picked, int *n_iter) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && aligned_out && labels && picked && n_iter && init_rows, "tsc_diverse_select: null argument");
    TSC_TRY(check_shape("tsc_diverse_select", N, n_atoms));
    const int D = 3 * n_atoms;
    TSC_TRY(check_k("tsc_diverse_select", N, D, k));
    TSC_REQUIRE(max_iter >= 1 && std::isfinite(tol) && tol >= 0.0, "tsc_diverse_select: max_iter = %d, tol = %g", max_iter, tol);
    if (u)
        TSC_TRY(check_uniforms("tsc_diverse_select", u, k));
    else
        for (int j = 0; j < k; ++j) TSC_REQUIRE(init_rows[j] >= 0 && init_rows[j] < N, "tsc_diverse_select: init row %d out of range", init_rows[j]);
    TSC_TRY(check_finite("tsc_diverse_select", "structures", structures, size_t(N) * D));
    if (energies)
        for (int64_t i = 0; i < N; ++i) TSC_REQUIRE(!std::isnan(energies[i]), "tsc_diverse_select: energies[%lld] is NaN", (long long)i);
    reset_times();
    HostCall h(c);
    Scratch &s = h.scratch();
    const size_t count = size_t(N) * D;
    double *d_in, *d_al, *d_X, *d_mean, *d_e = nullptr;
    int32_t *d_rows, *d_picked;
    TSC_TRY(h.in(structures, count, &d_in));
    TSC_TRY(s.get(count, &d_al));
    TSC_TRY(s.get(count, &d_X));
    TSC_TRY(s.get(size_t(D), &d_mean));
    TSC_TRY(s.get(size_t(k), &d_rows));
    TSC_TRY(h.out(picked, size_t(k), &d_picked));
    if (energies) TSC_TRY(h.in(energies, size_t(N), &d_e));
    StageTimer whole(c), tm(c);
    whole.begin();
    tm.begin();
    TSC_TRY(align_dev(c, h, d_in, N, n_atoms, nullptr, 0, d_al));
    tm.end(&g_times[0]);
    TSC_TRY(h.fetch(aligned_out, d_al, count));
    TSC_HIP(hipMemcpyAsync(d_X, d_al, count * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (u) {   // seeds chosen here, on the aligned features, and handed back
        TSC_TRY(seed_dev(c, h, d_al, N, D, k, u, d_rows));
        TSC_TRY(h.fetch(init_rows, d_rows, size_t(k)));
    } else {
        TSC_HIP(hipMemcpyAsync(d_rows, init_rows, size_t(k) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    double tol_abs = 0.0;
    TSC_TRY(centre_features(c, s, d_X, N, D, d_mean, tol, &tol_abs));
    Lloyd L;
    TSC_TRY(lloyd_alloc(c, s, L, d_X, N, D, k));
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(int64_t(k) * D, 256)), dim3(256), 0, c->stream, d_X, D, d_rows, k, L.C);
    TSC_TRY(lloyd_run(c, L, max_iter, tol_abs, n_iter, nullptr, tm.on ? &tm : nullptr));
    // the pick sees differences centre - member only: the centred features and centres serve as they are
    TSC_TRY(pick_dev(c, L, d_X, L.C, d_e, d_picked));
    whole.end(&g_times[3]);
    TSC_TRY(h.fetch(labels, L.labels, size_t(N)));
    return h.finish();
    TSC_API_GUARD_END
}
