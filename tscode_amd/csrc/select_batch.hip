// select_batch.hip -- launches and C ABI of what takes many small ensembles per call: the torsion fingerprints and the pair search of
// prune_conformers_tfd (tfd.hpp; tscode/numba_functions.py:142-231, one run of :160-226 per segment), and alignment, k-means and the
// diverse-conformer pick (diverse_batch.hpp; tscode/torsion_module.py:882-922 per segment).  gfx950 only.  There is deliberately no CPU
// implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "diverse_batch.hpp"
#include "tfd_batch.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

using namespace tsc;

// _get_tf_mat (tscode/numba_functions.py:233-240) of n_segments ensembles at once.  Host arrays in, the fingerprints stay on the device:
// tf f32[tf_count = sum N T], segment after segment, for the schedule slots of tsc_tfd_batch_pass_dev.
extern "C" __attribute__((visibility("default"))) int tsc_tfd_batch_fingerprints_dev(tsc_ctx *c, const double *coords, const int64_t *offsets,
                                                                                     const int32_t *n_structs, const int32_t *n_atoms,
                                                                                     const int32_t *quads, const int32_t *n_quads,
                                                                                     int64_t n_segments, float *tf, int64_t tf_count) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_tfd_batch_fingerprints_dev";
    TSC_REQUIRE(c, "%s: null argument", who);
    TSC_REQUIRE(n_segments >= 0 && n_segments < INT_MAX, "%s: %lld segments", who, (long long)n_segments);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(offsets && n_structs && n_atoms && n_quads, "%s: null argument", who);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    std::vector<TfdSegment> segs{};
    segs.resize(size_t(n_segments));   // (in front of the HostCall: it outlives the call's wait for the stream)
    int64_t quad0 = 0, elem0 = 0;
    for (int64_t s = 0; s < n_segments; ++s) {
        TSC_REQUIRE(n_structs[s] >= 0 && n_atoms[s] > 0 && n_quads[s] >= 0, "%s: segment %lld: bad sizes (%d structures, %d atoms, %d quadruplets)", who,
                    (long long)s, n_structs[s], n_atoms[s], n_quads[s]);
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == int64_t(n_structs[s]) * n_atoms[s] * 3, "%s: offsets[%lld] .. offsets[%lld] span %lld doubles, segment is %d x %d x 3",
                    who, (long long)s, (long long)s + 1, (long long)(offsets[s + 1] - offsets[s]), n_structs[s], n_atoms[s]);
        TSC_REQUIRE(n_quads[s] == 0 || quads, "%s: null argument", who);
        for (int64_t q = 4 * quad0; q < 4 * (quad0 + n_quads[s]); ++q)
            TSC_REQUIRE(quads[q] >= 0 && quads[q] < n_atoms[s], "%s: segment %lld: quadruplet atom index %d out of range", who, (long long)s, quads[q]);
        TfdSegment &g = segs[size_t(s)];
        g.coord0 = offsets[s], g.quad0 = quad0, g.elem0 = elem0, g.N = n_structs[s], g.n = n_atoms[s], g.T = n_quads[s], g.pad = 0;
        quad0 += n_quads[s], elem0 += int64_t(n_structs[s]) * n_quads[s];
    }
    TSC_REQUIRE(tf_count == elem0, "%s: room for %lld fingerprint elements, the segments have %lld", who, (long long)tf_count, (long long)elem0);
    if (elem0 == 0) return 0;
    TSC_REQUIRE(coords && tf, "%s: null argument", who);
    HostCall h(c);
    const double *d_coords;
    const int32_t *d_quads;
    const TfdSegment *d_segs;
    TSC_TRY(h.in(segs.data(), segs.size(), &d_segs));
    TSC_TRY(h.in(coords, size_t(offsets[n_segments]), &d_coords));
    TSC_TRY(h.in(quads, size_t(quad0) * 4, &d_quads));
    hipLaunchKernelGGL(k_torsion_fingerprints_seg, dim3(grid_for(elem0, 256, 256 * 8)), dim3(256), 0, c->stream, d_coords, d_quads, d_segs, int(n_segments),
                       elem0, tf);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

// One schedule slot of prune_conformers_tfd (tscode/numba_functions.py:171-199) for the n_open segments whose gate is open in it, in ONE
// launch: segment q has n_structs[q] fingerprints of n_quads[q] angles at tf + elem0[q] and its rows at first + row0[q]; d, k,
// num_active and thresh are its own.  first i32[total_rows] (host) comes back as -1 wherever no open segment lies.
extern "C" __attribute__((visibility("default"))) int tsc_tfd_batch_pass_dev(tsc_ctx *c, const float *tf, int64_t tf_count, const int64_t *elem0,
                                                                             const int64_t *row0, const int32_t *n_structs, const int32_t *n_quads,
                                                                             const int64_t *d, const int64_t *k, const int64_t *num_active,
                                                                             const double *thresh, int64_t n_open, int64_t total_rows, int32_t *first) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_tfd_batch_pass_dev";
    TSC_REQUIRE(c && (first || total_rows == 0), "%s: null argument", who);
    TSC_REQUIRE(n_open >= 0 && n_open < INT_MAX && total_rows >= 0 && tf_count >= 0, "%s: %lld segments, %lld rows, %lld fingerprint elements", who,
                (long long)n_open, (long long)total_rows, (long long)tf_count);
    TSC_REQUIRE(n_open == 0 || (elem0 && row0 && n_structs && n_quads && d && k && num_active && thresh), "%s: null argument", who);
    std::vector<TfdPassSegment> segs{};   // (in front of the HostCall)
    segs.resize(size_t(n_open));
    int64_t wave0 = 0, row_end = 0;
    for (int64_t q = 0; q < n_open; ++q) {
        const int64_t N = n_structs[q], T = n_quads[q];
        TSC_REQUIRE(N >= 1 && T >= 0, "%s: segment %lld: %lld structures (at least 1), %lld quadruplets", who, (long long)q, (long long)N, (long long)T);
        TSC_REQUIRE(d[q] > 0 && k[q] > 0 && num_active[q] >= 0 && num_active[q] <= N && d[q] <= N / k[q],
                    "%s: segment %lld: bad pass geometry (n = %lld, d = %lld, k = %lld, active = %lld)", who, (long long)q, (long long)N, (long long)d[q],
                    (long long)k[q], (long long)num_active[q]);
        TSC_REQUIRE(row0[q] >= row_end && row0[q] + N <= total_rows, "%s: segment %lld: rows %lld .. %lld overlap the segment before or pass %lld", who,
                    (long long)q, (long long)row0[q], (long long)(row0[q] + N), (long long)total_rows);
        TSC_REQUIRE(elem0[q] >= 0 && elem0[q] <= tf_count && N * T <= tf_count - elem0[q], "%s: segment %lld: fingerprints %lld .. %lld of %lld", who,
                    (long long)q, (long long)elem0[q], (long long)(elem0[q] + N * T), (long long)tf_count);
        TSC_REQUIRE(tf || N * T == 0, "%s: null argument", who);
        row_end = row0[q] + N;
        TfdPassSegment &g = segs[size_t(q)];
        g.wave0 = wave0, g.row0 = row0[q], g.elem0 = elem0[q], g.d = d[q], g.k = k[q], g.num_active = num_active[q], g.thresh = thresh[q];
        g.N = int32_t(N), g.T = int32_t(T);
        wave0 += N;
    }
    if (total_rows == 0) return 0;
    HostCall h(c);
    const TfdPassSegment *d_segs;
    int32_t *d_first;
    TSC_TRY(h.in(segs.data(), segs.size(), &d_segs));
    TSC_TRY(h.out(first, size_t(total_rows), &d_first));
    TSC_HIP(hipMemsetAsync(d_first, 0xff, size_t(total_rows) * sizeof(int32_t), c->stream));
    if (wave0 > 0) {
        hipLaunchKernelGGL(k_tfd_first_similar_seg, dim3(grid_for(wave0, 4, 256 * 16)), dim3(256), 0, c->stream, tf, d_segs, int(n_open), wave0, d_first);
        TSC_HIP(hipGetLastError());
    }
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// alignment, k-means and pick of many ensembles (diverse_batch.hpp)

namespace {

// the work items of one segmented kernel: for every listed segment the workgroups (bx, by) of the grid (nx, ny) the single call launches
template <typename F>
void add_items(std::vector<DvItem> &items, const std::vector<DvSegment> &segs, const std::vector<int> &order, F &&grid) {
    for (int s : order) {
        int nx = 0, ny = 1;
        grid(segs[size_t(s)], &nx, &ny);
        for (int by = 0; by < ny; ++by)
            for (int bx = 0; bx < nx; ++bx) items.push_back(DvItem{s, bx, by, 0});
    }
}

struct DvTable {   // a table on the device and its length
    const DvItem *dev = nullptr;
    unsigned count = 0;
};

int upload_items(HostCall &h, std::vector<DvItem> &all, std::vector<std::pair<size_t, size_t>> &spans, std::vector<DvTable *> &tables) {
    const DvItem *d_all;
    TSC_TRY(h.in(all.data(), all.size(), &d_all));
    for (size_t q = 0; q < tables.size(); ++q) tables[q]->dev = d_all + spans[q].first, tables[q]->count = unsigned(spans[q].second);
    return 0;
}

// lloyd's assign() (diverse.hip) picks the template width of k_kmeans_assign from k alone
int assign_width(int k) {
    const int tiles = ceil_div(k, 16), blocks = ceil_div(tiles, 8);
    return ceil_div(tiles, blocks);
}

}  // namespace

// tsc_diverse_select (tscode/torsion_module.py:882-922) on n_segments ensembles at once: per segment the single call's results, bit for bit.
extern "C" __attribute__((visibility("default"))) int tsc_diverse_select_batch(tsc_ctx *c, const double *structures, const int64_t *offsets,
                                                                               const int32_t *n_structs, const int32_t *n_atoms, const int32_t *k,
                                                                               int64_t n_segments, int32_t *init_rows, const double *u,
                                                                               const double *energies, const uint8_t *flags, int max_iter, double tol,
                                                                               double *aligned_out, int32_t *labels, int32_t *picked, int32_t *n_iter) {
    TSC_API_GUARD_BEGIN
    const char *who = "tsc_diverse_select_batch";
    TSC_REQUIRE(c, "%s: null argument", who);
    TSC_REQUIRE(n_segments >= 0 && n_segments <= (1 << 20), "%s: %lld segments", who, (long long)n_segments);
    if (n_segments == 0) return 0;
    TSC_REQUIRE(structures && offsets && n_structs && n_atoms && k && init_rows && flags && aligned_out && labels && picked && n_iter, "%s: null argument", who);
    TSC_REQUIRE(max_iter >= 1 && std::isfinite(tol) && tol >= 0.0, "%s: max_iter = %d, tol = %g", who, max_iter, tol);
    TSC_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    const int S = int(n_segments);
    // everything that can be refused is refused here, before anything touches the device; the message names the segment
    std::vector<DvSegment> segs{};
    segs.resize(size_t(S));
    std::vector<int32_t> rows_host{};   // (both in front of the HostCall: they outlive the call's wait for the stream)
    int64_t row0 = 0, c0 = 0, part0 = 0, k0 = 0, d0 = 0, sp0 = 0;
    bool any_seeded = false, any_energies = false;
    for (int s = 0; s < S; ++s) {
        char name[64];
        snprintf(name, sizeof(name), "%s: segment %d", who, s);
        TSC_REQUIRE((flags[s] & ~3) == 0, "%s: flags %d (1 = energies, 2 = seeded)", name, int(flags[s]));
        const int64_t N = n_structs[s];
        TSC_TRY(check_shape(name, N, n_atoms[s]));
        const int D = 3 * n_atoms[s];
        TSC_TRY(check_k(name, N, D, k[s]));
        TSC_REQUIRE(offsets[s + 1] - offsets[s] == N * D, "%s: offsets span %lld doubles, the segment is %lld x %d x 3", name,
                    (long long)(offsets[s + 1] - offsets[s]), (long long)N, n_atoms[s]);
        const bool seeded = (flags[s] & 2) != 0, has_e = (flags[s] & 1) != 0;
        if (seeded) {
            TSC_REQUIRE(u, "%s: seeded without uniforms", name);
            TSC_TRY(check_uniforms(name, u + k0, k[s]));
        } else {
            for (int j = 0; j < k[s]; ++j) TSC_REQUIRE(init_rows[k0 + j] >= 0 && init_rows[k0 + j] < N, "%s: init row %d out of range", name, init_rows[k0 + j]);
        }
        TSC_TRY(check_finite(name, "structures", structures + offsets[s], size_t(N) * D));
        if (has_e) {
            TSC_REQUIRE(energies, "%s: energies flagged without an energies array", name);
            for (int64_t i = 0; i < N; ++i) TSC_REQUIRE(!std::isnan(energies[row0 + i]), "%s: energies[%lld] is NaN", name, (long long)i);
        }
        DvSegment &g = segs[size_t(s)];
        g.x0 = offsets[s], g.row0 = row0, g.c0 = c0, g.part0 = part0;
        g.N = int32_t(N), g.n = n_atoms[s], g.D = D, g.k = k[s];
        g.k0 = int32_t(k0), g.d0 = int32_t(d0), g.sp0 = int32_t(sp0);
        g.chunks = int(std::max<int64_t>(1, std::min<int64_t>(64, N / 256)));   // col_stats (diverse.hip)
        g.slices = ceil_div(D, 64);
        g.has_energies = has_e, g.seeded = seeded, g.pad = 0;
        g.inv_N = 1.0 / double(N), g.inv_D = 1.0 / double(D);
        any_seeded |= seeded, any_energies |= has_e;
        row0 += N, c0 += int64_t(k[s]) * D, part0 += int64_t(g.chunks) * D, k0 += k[s], d0 += D, sp0 += int64_t(k[s]) * g.slices;
        TSC_REQUIRE(row0 < INT32_MAX && c0 < INT32_MAX, "%s: the batch passes %d rows or centre elements", name, INT32_MAX - 1);
    }
    const int64_t total_rows = row0, total_k = k0, total_doubles = offsets[S];
    // first seeds as seed_dev (diverse.hip) forms them; the rows of the other segments as given
    rows_host.assign(init_rows, init_rows + total_k);
    for (int s = 0; s < S; ++s)
        if (segs[size_t(s)].seeded)
            rows_host[size_t(segs[size_t(s)].k0)] = int32_t(std::min<int64_t>(segs[size_t(s)].N - 1, int64_t(u[segs[size_t(s)].k0] * double(segs[size_t(s)].N))));

    // ---- work-item tables: exactly the workgroups each segment's own grids have
    std::vector<int> all_segs, seeded_segs;
    all_segs.resize(size_t(S));
    std::iota(all_segs.begin(), all_segs.end(), 0);
    for (int s = 0; s < S; ++s)
        if (segs[size_t(s)].seeded) seeded_segs.push_back(s);
    std::stable_sort(seeded_segs.begin(), seeded_segs.end(), [&](int a, int b) { return segs[size_t(a)].k > segs[size_t(b)].k; });
    std::vector<DvItem> items;
    std::vector<std::pair<size_t, size_t>> spans;
    std::vector<DvTable *> tables;
    DvTable t_rows4, t_k4, t_colpart, t_colfin, t_k, t_update, t_seed_rows4, t_seed_seg, t_assign[8];
    auto table = [&](DvTable &t, const std::vector<int> &order, auto &&grid) {
        const size_t at = items.size();
        add_items(items, segs, order, grid);
        spans.push_back({at, items.size() - at});
        tables.push_back(&t);
    };
    table(t_rows4, all_segs, [](const DvSegment &g, int *nx, int *) { *nx = ceil_div(g.N, 4); });
    table(t_k4, all_segs, [](const DvSegment &g, int *nx, int *) { *nx = ceil_div(g.k, 4); });
    table(t_colpart, all_segs, [](const DvSegment &g, int *nx, int *ny) { *nx = ceil_div(g.D, 64), *ny = g.chunks; });
    table(t_colfin, all_segs, [](const DvSegment &g, int *nx, int *) { *nx = ceil_div(g.D, 256); });
    table(t_k, all_segs, [](const DvSegment &g, int *nx, int *) { *nx = g.k; });
    table(t_update, all_segs, [](const DvSegment &g, int *nx, int *ny) { *nx = g.k, *ny = g.slices; });
    for (int w = 1; w <= 8; ++w) {
        std::vector<int> of_width;
        for (int s = 0; s < S; ++s)
            if (assign_width(segs[size_t(s)].k) == w) of_width.push_back(s);
        table(t_assign[w - 1], of_width, [](const DvSegment &g, int *nx, int *) { *nx = ceil_div(g.N, KA_ROWS); });
    }
    table(t_seed_rows4, seeded_segs, [](const DvSegment &g, int *nx, int *) { *nx = ceil_div(g.N, 4); });
    table(t_seed_seg, seeded_segs, [](const DvSegment &, int *nx, int *) { *nx = 1; });
    // seeded segments with k > j are a prefix of the seeded tables: their lengths per j
    const int max_seed_k = seeded_segs.empty() ? 0 : segs[size_t(seeded_segs[0])].k;
    std::vector<unsigned> seed_segs_at(size_t(max_seed_k) + 1, 0), seed_rows4_at(size_t(max_seed_k) + 1, 0);
    for (int j = 1; j < max_seed_k; ++j)
        for (int s : seeded_segs)
            if (segs[size_t(s)].k > j) seed_segs_at[size_t(j)] += 1, seed_rows4_at[size_t(j)] += unsigned(ceil_div(segs[size_t(s)].N, 4));

    std::vector<DvState> state_host(size_t(S), DvState{1, 0, 0, 0, 0.0});
    DvSummary summary_host{0, 0};
    HostCall h(c);
    Scratch &sc = h.scratch();
    DvBatch b{};
    TSC_TRY(upload_items(h, items, spans, tables));
    TSC_TRY(h.in(segs.data(), segs.size(), &b.segs));
    TSC_TRY(h.in(state_host.data(), state_host.size(), &b.state));
    TSC_TRY(h.in(structures, size_t(total_doubles), &b.in));
    TSC_TRY(sc.get(size_t(total_doubles), &b.al));
    TSC_TRY(sc.get(size_t(total_doubles), &b.X));
    TSC_TRY(sc.get(size_t(c0), &b.C));
    TSC_TRY(sc.get(size_t(total_rows), &b.xn));
    TSC_TRY(sc.get(size_t(total_k), &b.cn));
    TSC_TRY(sc.get(size_t(total_rows), &b.own_d2));
    TSC_TRY(sc.get(size_t(sp0), &b.shift_part));
    TSC_TRY(sc.get(size_t(d0), &b.mean));
    TSC_TRY(sc.get(size_t(d0), &b.var));
    TSC_TRY(sc.get(size_t(S), &b.mv));
    TSC_TRY(sc.get(size_t(part0), &b.part));
    TSC_TRY(sc.get(size_t(total_rows), &b.labels));
    TSC_TRY(sc.get(size_t(total_k), &b.counts));
    TSC_TRY(sc.get(size_t(total_k) + S, &b.offs));
    TSC_TRY(sc.get(size_t(total_rows), &b.members));
    TSC_TRY(sc.get(size_t(S), &b.changed));
    TSC_TRY(sc.get(size_t(S), &b.ctl));
    TSC_TRY(h.in(rows_host.data(), rows_host.size(), &b.rows));
    TSC_TRY(h.out(picked, size_t(total_k), &b.picked));
    if (any_energies) TSC_TRY(h.in(energies, size_t(total_rows), &b.energies));
    DvSummary *d_summary;
    TSC_TRY(sc.get(1, &d_summary));

    hipLaunchKernelGGL(k_align_structures_seg, dim3(t_rows4.count), dim3(256), 0, c->stream, b, t_rows4.dev);
    TSC_HIP(hipGetLastError());
    TSC_TRY(h.fetch(aligned_out, b.al, size_t(total_doubles)));
    TSC_HIP(hipMemcpyAsync(b.X, b.al, size_t(total_doubles) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (any_seeded) {   // seeds chosen here, on the aligned features, and handed back: one pair of launches per seed index
        TSC_TRY(h.in(u, size_t(total_k), &b.u));
        TSC_TRY(sc.get(size_t(total_rows), &b.min_d2));
        for (int j = 1; j < max_seed_k; ++j) {
            hipLaunchKernelGGL(k_kmeans_seed_update_seg, dim3(seed_rows4_at[size_t(j)]), dim3(256), 0, c->stream, b, t_seed_rows4.dev, j - 1);
            hipLaunchKernelGGL(k_kmeans_seed_pick_seg, dim3(seed_segs_at[size_t(j)]), dim3(1024), 0, c->stream, b, t_seed_seg.dev, j);
        }
        TSC_HIP(hipGetLastError());
    }
    TSC_TRY(h.fetch(init_rows, b.rows, size_t(total_k)));
    // centre_features (diverse.hip) per segment; mean(var) stays on the device, where the control kernel forms the tolerance
    hipLaunchKernelGGL(k_col_partial_seg, dim3(t_colpart.count), dim3(256), 0, c->stream, b, t_colpart.dev, 0);
    hipLaunchKernelGGL(k_col_finish_seg, dim3(t_colfin.count), dim3(256), 0, c->stream, b, t_colfin.dev, 0);
    hipLaunchKernelGGL(k_centre_rows_seg, dim3(t_rows4.count), dim3(256), 0, c->stream, b, t_rows4.dev);
    hipLaunchKernelGGL(k_col_partial_seg, dim3(t_colpart.count), dim3(256), 0, c->stream, b, t_colpart.dev, 1);
    hipLaunchKernelGGL(k_col_finish_seg, dim3(t_colfin.count), dim3(256), 0, c->stream, b, t_colfin.dev, 1);
    hipLaunchKernelGGL(k_mean_var_seg, dim3(unsigned(S)), dim3(1024), 0, c->stream, b);
    hipLaunchKernelGGL(k_gather_rows_seg, dim3(t_k4.count), dim3(256), 0, c->stream, b, t_k4.dev);
    TSC_HIP(hipGetLastError());

    // lloyd_run (diverse.hip) for all segments in lockstep; a finished segment's workgroups return at once
    auto assign_and_bucket = [&](int gate) -> int {
        hipLaunchKernelGGL(k_row_norms_seg, dim3(t_k4.count), dim3(256), 0, c->stream, b, t_k4.dev, 1, gate);
        TSC_HIP(hipMemsetAsync(b.changed, 0, size_t(S) * sizeof(int), c->stream));
        for (int w = 1; w <= 8; ++w) {
            const DvTable &t = t_assign[w - 1];
            if (t.count)
                with_width(w, [&](auto width) {
                    hipLaunchKernelGGL(k_kmeans_assign_seg<decltype(width)::value>, dim3(t.count), dim3(256), 0, c->stream, b, t.dev, gate);
                });
        }
        hipLaunchKernelGGL(k_label_count_seg, dim3(t_k.count), dim3(256), 0, c->stream, b, t_k.dev, gate);
        hipLaunchKernelGGL(k_label_bucket_seg, dim3(t_k.count), dim3(256), 0, c->stream, b, t_k.dev, gate);
        TSC_HIP(hipGetLastError());
        return 0;
    };
    hipLaunchKernelGGL(k_row_norms_seg, dim3(t_rows4.count), dim3(256), 0, c->stream, b, t_rows4.dev, 0, int(DV_ALL));
    TSC_HIP(hipMemsetAsync(b.labels, 0xff, size_t(total_rows) * sizeof(int32_t), c->stream));
    for (int it = 0; it < max_iter; ++it) {
        TSC_TRY(assign_and_bucket(DV_LIVE));
        hipLaunchKernelGGL(k_own_d2_seg, dim3(t_rows4.count), dim3(256), 0, c->stream, b, t_rows4.dev, int(DV_LIVE));
        hipLaunchKernelGGL(k_kmeans_relocate_seg, dim3(unsigned(S)), dim3(256), 0, c->stream, b, int(DV_LIVE));
        hipLaunchKernelGGL(k_kmeans_update_seg, dim3(t_update.count), dim3(256), 0, c->stream, b, t_update.dev, int(DV_LIVE));
        TSC_HIP(hipMemsetAsync(d_summary, 0, sizeof(DvSummary), c->stream));
        hipLaunchKernelGGL(k_kmeans_control_seg, dim3(unsigned(S)), dim3(64), 0, c->stream, b, max_iter, tol, d_summary);
        TSC_HIP(hipGetLastError());
        TSC_TRY(h.fetch(&summary_host, d_summary, 1));   // the ONE record the host reads per iteration
        TSC_HIP(hipStreamSynchronize(c->stream));
        if (summary_host.live == 0) break;
    }
    if (summary_host.need_final) TSC_TRY(assign_and_bucket(DV_FINAL));
    hipLaunchKernelGGL(k_diverse_pick_seg, dim3(t_k.count), dim3(256), 0, c->stream, b, t_k.dev);
    TSC_HIP(hipGetLastError());
    TSC_TRY(h.fetch(labels, b.labels, size_t(total_rows)));
    TSC_TRY(h.fetch(state_host.data(), b.state, state_host.size()));
    TSC_TRY(h.finish());
    for (int s = 0; s < S; ++s) n_iter[s] = state_host[size_t(s)].n_iter;
    return 0;
    TSC_API_GUARD_END
}
