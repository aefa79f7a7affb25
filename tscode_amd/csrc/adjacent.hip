// adjacent.hip -- the adjacent rows: greedy filters, csearch rotations, TFD, moments of inertia, the embed drivers
// gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "embed_transform.hpp"
#include "scan_kernels.hpp"
#include "gather_rows.hpp"
#include "prune_api.hpp"
#include "group_filter.hpp"
#include "csearch_kernels.hpp"
#include "tfd_kernels.hpp"
#include "moi_kernels.hpp"
#include "host_order.hpp"
#include "trimolecular.hpp"
#include "embed_prune_plan.hpp"

#include <memory>

// --------------------------------------------------------------------------------------------------
// greedy per-group filter

extern "C" __attribute__((visibility("default"))) int tsc_greedy_group_filter_dev(tsc_ctx *c, const double *poses, const int32_t *group_off_dev, int n_groups,
                                                                             int64_t n_poses, int n_atoms, double rmsd_thr, uint8_t *accepted) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && poses && group_off_dev && accepted, "tsc_greedy_group_filter_dev: null argument");
    TSC_REQUIRE(n_groups >= 0 && n_poses >= 0 && n_atoms > 0 && rmsd_thr > 0, "bad sizes");
    if (n_groups == 0 || n_poses == 0) return 0;
    DeviceGuard guard(c->device);
    Scratch s(c);
    double *G;
    TSC_TRY(s.get(size_t(n_poses), &G));
    hipLaunchKernelGGL(k_greedy_group_filter, dim3(n_groups), dim3(256), 0, c->stream, poses, group_off_dev, n_groups, n_atoms, rmsd_thr,
                       accepted, G);
    TSC_HIP(hipGetLastError());
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_greedy_group_filter(tsc_ctx *c, const double *poses, const int32_t *group_off, int n_groups, int n_atoms,
                                                                         double rmsd_thr, uint8_t *accepted) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && poses && group_off && accepted, "tsc_greedy_group_filter: null argument");
    TSC_REQUIRE(n_groups >= 0 && n_atoms > 0 && rmsd_thr > 0, "bad sizes");
    if (n_groups == 0) return 0;
    TSC_REQUIRE(group_off[0] == 0, "group_off must start at 0");
    for (int g = 0; g < n_groups; ++g)
        TSC_REQUIRE(group_off[g + 1] >= group_off[g] && group_off[g + 1] - group_off[g] <= GF_MAX_GROUP,
                    "group %d: sizes must be in [0, %d]", g, GF_MAX_GROUP);
    const int64_t n_poses = group_off[n_groups];
    if (n_poses == 0) return 0;
    HostCall h(c);
    double *d_poses;
    int32_t *d_off;
    uint8_t *d_acc;
    TSC_TRY(h.in(poses, size_t(n_poses) * n_atoms * 3, &d_poses));
    TSC_TRY(h.in(group_off, size_t(n_groups) + 1, &d_off));
    TSC_TRY(h.out(accepted, size_t(n_poses), &d_acc));
    TSC_TRY(tsc_greedy_group_filter_dev(c, d_poses, d_off, n_groups, n_poses, n_atoms, rmsd_thr, d_acc));
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// conformational-search rotations

static int csearch_args(int n_atoms, int n_tors, int64_t n_cand, double thresh, int64_t max_clashes, CsearchArgs *a) {
    TSC_REQUIRE(n_atoms > 0 && n_tors >= 0 && n_cand >= 0, "bad sizes (%d atoms, %d torsions, %lld candidates)", n_atoms, n_tors, (long long)n_cand);
    TSC_REQUIRE(n_atoms <= 65535 && torsion_lists_bytes(n_tors, n_atoms) + csearch_wave_bytes(n_atoms) <= 150 * 1024,
                "%d atoms x %d torsions exceed the LDS staging of the csearch kernels", n_atoms, n_tors);
    a->n = n_atoms, a->n_tors = n_tors, a->n_cand = n_cand;
    a->sq_bound = clash_sq_bound(thresh), a->max_clashes = max_clashes;
    return 0;
}

// wavefronts per workgroup (4, 2 or 1) that fit the LDS, and the dynamic LDS size of the launch
static int csearch_waves(int n_atoms, int n_tors, size_t *lds) {
    int w = 4;
    while (w > 1 && torsion_lists_bytes(n_tors, n_atoms) + w * csearch_wave_bytes(n_atoms) > 150 * 1024) w >>= 1;
    *lds = torsion_lists_bytes(n_tors, n_atoms) + w * csearch_wave_bytes(n_atoms);
    return w;
}

static int check_torsions(const int32_t *torsions, int n_tors, int n_atoms) {
    for (int t = 0; t < n_tors; ++t)
        for (int q = 0; q < 4; ++q)
            TSC_REQUIRE(torsions[4 * t + q] >= 0 && torsions[4 * t + q] < n_atoms, "torsion %d: atom index %d out of range", t, torsions[4 * t + q]);
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_csearch_rotate_dev(tsc_ctx *c, const double *coords, int n_atoms, const int32_t *torsions,
                                                                             const uint8_t *masks, int n_tors, const int32_t *angles, int64_t n_cand,
                                                                             double thresh, int64_t max_clashes, double *out, int32_t *rotated_bonds) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && out && rotated_bonds && torsions && masks && angles, "tsc_csearch_rotate_dev: null argument");
    CsearchArgs a;
    TSC_TRY(csearch_args(n_atoms, n_tors, n_cand, thresh, max_clashes, &a));
    if (n_cand == 0) return 0;
    DeviceGuard guard(c->device);
    size_t lds;
    const int waves = csearch_waves(n_atoms, n_tors, &lds);
    TSC_TRY(lds_attribute(&k_csearch_rotate, lds));
    hipLaunchKernelGGL(k_csearch_rotate, dim3(grid_for(n_cand, waves, 256 * 8)), dim3(64 * waves), lds, c->stream, a, coords, torsions, masks, angles, out,
                       rotated_bonds);
    TSC_HIP(hipGetLastError());
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_csearch_rotate(tsc_ctx *c, const double *coords, int n_atoms, const int32_t *torsions,
                                                                         const uint8_t *masks, int n_tors, const int32_t *angles, int64_t n_cand,
                                                                         double thresh, int64_t max_clashes, double *out, int32_t *rotated_bonds) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && out && rotated_bonds && (n_tors == 0 || (torsions && masks && angles)), "tsc_csearch_rotate: null argument");
    TSC_REQUIRE(n_atoms > 0 && n_tors >= 0 && n_cand >= 0, "bad sizes");
    TSC_TRY(check_torsions(torsions, n_tors, n_atoms));
    if (n_cand == 0) return 0;
    HostCall h(c);
    double *d_coords, *d_out;
    int32_t *d_tors, *d_angles, *d_rb;
    uint8_t *d_masks;
    TSC_TRY(h.in(coords, size_t(n_atoms) * 3, &d_coords));
    TSC_TRY(h.in(torsions, size_t(n_tors) * 4, &d_tors));
    TSC_TRY(h.in(masks, size_t(n_tors) * n_atoms, &d_masks));
    TSC_TRY(h.in(angles, size_t(n_cand) * n_tors, &d_angles));
    TSC_TRY(h.out(out, size_t(n_cand) * n_atoms * 3, &d_out));
    TSC_TRY(h.out(rotated_bonds, size_t(n_cand), &d_rb));
    TSC_TRY(tsc_csearch_rotate_dev(c, d_coords, n_atoms, d_tors, d_masks, n_tors, d_angles, n_cand, thresh, max_clashes, d_out, d_rb));
    return h.finish();
    TSC_API_GUARD_END
}

// The per-set checks of the multi kernel and the widest set's torsion count: csearch_args' LDS bound holds for every set
static int csearch_multi_sets(int n_atoms, const int32_t *set_off, int n_sets, int *t_widest) {
    TSC_REQUIRE(n_atoms > 0 && n_sets > 0 && set_off && set_off[0] == 0, "bad sizes (%d atoms, %d torsion sets; set_off must start at 0)", n_atoms, n_sets);
    int widest = 0;
    for (int k = 0; k < n_sets; ++k) {
        const int t = set_off[k + 1] - set_off[k];
        TSC_REQUIRE(t >= 0, "torsion set %d: set_off must not decrease", k);
        TSC_REQUIRE(n_atoms <= 65535 && torsion_lists_bytes(t, n_atoms) + csearch_wave_bytes(n_atoms) <= 150 * 1024,
                    "torsion set %d: %d atoms x %d torsions exceed the LDS staging of the csearch kernels", k, n_atoms, t);
        widest = std::max(widest, t);
    }
    *t_widest = widest;
    return 0;
}

// Host arrays.  Cuts the candidates (cand_start ascending: the candidates of one start are contiguous) into the work items of
// k_csearch_rotate_multi: (lo, hi, first torsion of the set, torsions of the set), at most one candidate per wavefront of a
// workgroup, never across two starts of different sets.  items == NULL only counts.
extern "C" __attribute__((visibility("default"))) int tsc_csearch_multi_plan(const int32_t *cand_start, int64_t n_cand, const int32_t *start_set, int n_starts,
                                                                             const int32_t *set_off, int n_sets, int n_atoms, int32_t *items,
                                                                             int64_t items_cap, int64_t *n_items) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(n_items && (n_cand == 0 || cand_start) && (n_starts == 0 || start_set), "tsc_csearch_multi_plan: null argument");
    TSC_REQUIRE(n_cand >= 0 && n_cand < INT32_MAX && n_starts >= 0, "bad sizes (%lld candidates, %d starts)", (long long)n_cand, n_starts);
    int widest;
    TSC_TRY(csearch_multi_sets(n_atoms, set_off, n_sets, &widest));
    for (int s = 0; s < n_starts; ++s) TSC_REQUIRE(start_set[s] >= 0 && start_set[s] < n_sets, "start %d: torsion set %d out of range", s, start_set[s]);
    size_t lds;
    const int waves = csearch_waves(n_atoms, widest, &lds);
    int64_t count = 0;
    for (int64_t lo = 0; lo < n_cand;) {
        const int s = cand_start[lo];
        TSC_REQUIRE(s >= 0 && s < n_starts && (lo == 0 || s >= cand_start[lo - 1]), "candidate %lld: start %d out of range or out of order", (long long)lo, s);
        const int k = start_set[s];
        int64_t hi = lo + 1;
        while (hi < n_cand && hi - lo < waves && cand_start[hi] >= 0 && cand_start[hi] < n_starts && cand_start[hi] >= cand_start[hi - 1] &&
               start_set[cand_start[hi]] == k)
            ++hi;
        if (items) {
            TSC_REQUIRE(count < items_cap, "tsc_csearch_multi_plan: more than %lld work items", (long long)items_cap);
            items[4 * count] = int32_t(lo), items[4 * count + 1] = int32_t(hi), items[4 * count + 2] = set_off[k], items[4 * count + 3] = set_off[k + 1] - set_off[k];
        }
        ++count, lo = hi;
    }
    *n_items = count;
    return 0;
    TSC_API_GUARD_END
}

// set_off is a HOST array (it sizes the launch); everything else lives on the device
extern "C" __attribute__((visibility("default"))) int tsc_csearch_rotate_multi_dev(tsc_ctx *c, const double *starts, int n_atoms, const int32_t *torsions,
                                                                                   const uint8_t *masks, const int32_t *set_off, int n_sets,
                                                                                   const int32_t *angles, int t_max, const int32_t *cand_start,
                                                                                   const int32_t *cand_row, int64_t n_cand, const int32_t *items,
                                                                                   int64_t n_items, double thresh, int64_t max_clashes, double *out,
                                                                                   int32_t *rotated_bonds) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && set_off, "tsc_csearch_rotate_multi_dev: null argument");
    int widest;
    TSC_TRY(csearch_multi_sets(n_atoms, set_off, n_sets, &widest));
    TSC_REQUIRE(t_max >= widest && n_items >= 0 && n_items <= n_cand, "bad sizes (table %d wide, widest set %d; %lld work items, %lld candidates)", t_max,
                widest, (long long)n_items, (long long)n_cand);
    CsearchMultiArgs ma;
    TSC_TRY(csearch_args(n_atoms, widest, n_items, thresh, max_clashes, &ma.a));
    TSC_REQUIRE(n_cand < INT32_MAX, "too many candidates");
    if (n_cand == 0) return 0;
    TSC_REQUIRE(starts && out && rotated_bonds && cand_start && cand_row && items && (widest == 0 || (torsions && masks && angles)),
                "tsc_csearch_rotate_multi_dev: null argument");
    DeviceGuard guard(c->device);
    size_t lds;
    const int waves = csearch_waves(n_atoms, widest, &lds);
    ma.t_max = t_max, ma.lists_bytes = torsion_lists_bytes(widest, n_atoms);
    TSC_TRY(lds_attribute(&k_csearch_rotate_multi, lds));
    hipLaunchKernelGGL(k_csearch_rotate_multi, dim3(grid_for(n_items, 1, 256 * 8)), dim3(64 * waves), lds, c->stream, ma, starts, torsions, masks, angles,
                       cand_start, cand_row, items, out, rotated_bonds);
    TSC_HIP(hipGetLastError());
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_csearch_rotate_multi(tsc_ctx *c, const double *starts, int n_starts, int n_atoms, const int32_t *torsions,
                                                                               const uint8_t *masks, const int32_t *set_off, int n_sets,
                                                                               const int32_t *start_set, const int32_t *angles, int64_t n_rows, int t_max,
                                                                               const int32_t *cand_start, const int32_t *cand_row, int64_t n_cand,
                                                                               double thresh, int64_t max_clashes, double *out, int32_t *rotated_bonds) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && set_off && (n_cand == 0 || (starts && start_set && cand_start && cand_row && out && rotated_bonds)),
                "tsc_csearch_rotate_multi: null argument");
    TSC_REQUIRE(n_starts >= 0 && n_rows >= 0 && n_rows < INT32_MAX && n_cand >= 0 && t_max >= 0, "bad sizes");
    int64_t n_items = 0;
    TSC_TRY(tsc_csearch_multi_plan(cand_start, n_cand, start_set, n_starts, set_off, n_sets, n_atoms, nullptr, 0, &n_items));
    const int n_tors = set_off[n_sets];
    TSC_REQUIRE(n_tors == 0 || (torsions && masks), "tsc_csearch_rotate_multi: null argument");
    TSC_TRY(check_torsions(torsions, n_tors, n_atoms));
    for (int64_t m = 0; m < n_cand; ++m) TSC_REQUIRE(cand_row[m] >= 0 && cand_row[m] < n_rows, "candidate %lld: angle row %d out of range", (long long)m, cand_row[m]);
    if (n_cand == 0) return 0;
    TSC_REQUIRE(n_rows * t_max == 0 || angles, "tsc_csearch_rotate_multi: null argument");
    std::vector<int32_t> items(size_t(n_items) * 4);   // (declared in front of the HostCall that uploads it)
    TSC_TRY(tsc_csearch_multi_plan(cand_start, n_cand, start_set, n_starts, set_off, n_sets, n_atoms, items.data(), n_items, &n_items));
    HostCall h(c);
    double *d_starts, *d_out;
    int32_t *d_tors, *d_angles, *d_cs, *d_cr, *d_items, *d_rb;
    uint8_t *d_masks;
    TSC_TRY(h.in(starts, size_t(n_starts) * n_atoms * 3, &d_starts));
    TSC_TRY(h.in(torsions, size_t(n_tors) * 4, &d_tors));
    TSC_TRY(h.in(masks, size_t(n_tors) * n_atoms, &d_masks));
    TSC_TRY(h.in(angles, size_t(n_rows) * t_max, &d_angles));
    TSC_TRY(h.in(cand_start, size_t(n_cand), &d_cs));
    TSC_TRY(h.in(cand_row, size_t(n_cand), &d_cr));
    TSC_TRY(h.in(items.data(), items.size(), &d_items));
    TSC_TRY(h.out(out, size_t(n_cand) * n_atoms * 3, &d_out));
    TSC_TRY(h.out(rotated_bonds, size_t(n_cand), &d_rb));
    TSC_TRY(tsc_csearch_rotate_multi_dev(c, d_starts, n_atoms, d_tors, d_masks, set_off, n_sets, d_angles, t_max, d_cs, d_cr, n_cand, d_items, n_items, thresh,
                                         max_clashes, d_out, d_rb));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_csearch_select_dev(tsc_ctx *c, const double *cand, const int32_t *rotated_bonds, int n_atoms,
                                                                             const int32_t *seg_off, const int32_t *seg_start, const int32_t *seg_a0, int n_seg,
                                                                             int n_out, int64_t max_tries, int32_t *kept_count, int32_t *done,
                                                                             int32_t *rows_consumed, double *kept_rows, int64_t capacity,
                                                                             int64_t *n_kept_host) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && n_kept_host, "tsc_csearch_select_dev: null argument");
    TSC_REQUIRE(n_atoms > 0 && n_seg >= 0 && capacity >= 0, "bad sizes (%d atoms, %d segments, room for %lld rows)", n_atoms, n_seg, (long long)capacity);
    *n_kept_host = 0;
    if (n_seg == 0) return 0;
    TSC_REQUIRE(cand && rotated_bonds && seg_off && seg_start && seg_a0 && kept_count && done && rows_consumed && (capacity == 0 || kept_rows),
                "tsc_csearch_select_dev: null argument");
    DeviceGuard guard(c->device);
    Scratch s(c);
    int32_t *seg_kept, *total;
    TSC_TRY(s.get(size_t(n_seg), &seg_kept));
    TSC_TRY(s.get(1, &total));
    hipLaunchKernelGGL(k_csearch_select, dim3(grid_for(n_seg, 4, INT32_MAX)), dim3(256), 0, c->stream, rotated_bonds, seg_off, seg_start, seg_a0, n_seg, n_out,
                       (long long)max_tries, kept_count, done, rows_consumed, seg_kept);
    hipLaunchKernelGGL(k_csearch_compact, dim3(grid_for(n_seg, 4, INT32_MAX)), dim3(256), 0, c->stream, cand, rotated_bonds, seg_off, (const int32_t *)seg_kept,
                       n_seg, n_atoms * 3, (long long)capacity, kept_rows, total);
    TSC_HIP(hipGetLastError());
    int32_t kept = 0;
    TSC_TRY(read_i32(c, total, &kept));
    TSC_REQUIRE(kept <= capacity, "tsc_csearch_select_dev: %d rows kept, room for %lld (the rows past it were not written)", kept, (long long)capacity);
    *n_kept_host = kept;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_rotate_dihedral(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms, const int32_t *torsion,
                                                                          const uint8_t *mask, const double *angles, double *out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && torsion && mask && angles && out, "tsc_rotate_dihedral: null argument");
    TSC_REQUIRE(n_structs >= 0 && n_atoms > 0, "bad sizes");
    TSC_REQUIRE(out != coords, "tsc_rotate_dihedral: out must not alias coords");
    for (int q = 1; q <= 2; ++q) TSC_REQUIRE(torsion[q] >= 0 && torsion[q] < n_atoms, "torsion index %d out of range", torsion[q]);
    if (n_structs == 0) return 0;
    HostCall h(c);
    double *d_c, *d_o, *d_a;
    uint8_t *d_m;
    TSC_TRY(h.in(coords, size_t(n_structs) * n_atoms * 3, &d_c));
    TSC_TRY(h.in(angles, size_t(n_structs), &d_a));
    TSC_TRY(h.in(mask, size_t(n_atoms), &d_m));
    TSC_TRY(h.out(out, size_t(n_structs) * n_atoms * 3, &d_o));
    hipLaunchKernelGGL(k_rotate_dihedral, dim3(grid_for(n_structs * n_atoms, 256)), dim3(256), 0, c->stream, (const double *)d_c, n_structs, n_atoms, int(torsion[1]),
                       int(torsion[2]), (const uint8_t *)d_m, (const double *)d_a, d_o);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_torsion_comp_check(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                             const int32_t *torsion, const uint8_t *mask, double thresh,
                                                                             int64_t max_clashes, int32_t *ok) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && torsion && mask && ok, "tsc_torsion_comp_check: null argument");
    CsearchArgs a;
    TSC_TRY(csearch_args(n_atoms, 1, n_structs, thresh, max_clashes, &a));
    TSC_TRY(check_torsions(torsion, 1, n_atoms));
    if (n_structs == 0) return 0;
    HostCall h(c);
    double *d_coords;
    int32_t *d_tors, *d_ok;
    uint8_t *d_mask;
    TSC_TRY(h.in(coords, size_t(n_structs) * n_atoms * 3, &d_coords));
    TSC_TRY(h.in(torsion, size_t(4), &d_tors));
    TSC_TRY(h.in(mask, size_t(n_atoms), &d_mask));
    TSC_TRY(h.out(ok, size_t(n_structs), &d_ok));
    size_t lds;
    const int waves = csearch_waves(n_atoms, 1, &lds);
    TSC_TRY(lds_attribute(&k_torsion_comp_check, lds));
    hipLaunchKernelGGL(k_torsion_comp_check, dim3(grid_for(n_structs, waves, 256 * 8)), dim3(64 * waves), lds, c->stream, a, (const double *)d_coords,
                       (const int32_t *)d_tors, (const uint8_t *)d_mask, d_ok);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// torsion-fingerprint pruning

extern "C" __attribute__((visibility("default"))) int tsc_torsion_fingerprints(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                               const int32_t *quads, int n_quads, float *out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && quads && out, "tsc_torsion_fingerprints: null argument");
    TSC_REQUIRE(n_structs >= 0 && n_atoms > 0 && n_quads >= 0, "bad sizes");
    for (int q = 0; q < 4 * n_quads; ++q) TSC_REQUIRE(quads[q] >= 0 && quads[q] < n_atoms, "quadruplet atom index %d out of range", quads[q]);
    if (n_structs == 0 || n_quads == 0) return 0;
    HostCall h(c);
    double *d_coords;
    int32_t *d_quads;
    float *d_out;
    TSC_TRY(h.in(coords, size_t(n_structs) * n_atoms * 3, &d_coords));
    TSC_TRY(h.in(quads, size_t(n_quads) * 4, &d_quads));
    TSC_TRY(h.out(out, size_t(n_structs) * n_quads, &d_out));
    hipLaunchKernelGGL(k_torsion_fingerprints, dim3(grid_for(n_structs * n_quads, 256, 256 * 8)), dim3(256), 0, c->stream, (const double *)d_coords,
                       n_structs, n_atoms, (const int32_t *)d_quads, n_quads, d_out);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_tfd_first_similar(tsc_ctx *c, const float *tf, int64_t n_structs, int n_quads, int64_t d,
                                                                            int64_t k, int64_t num_active, double thresh, int32_t *first) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && tf && first, "tsc_tfd_first_similar: null argument");
    if (n_structs == 0) return 0;
    TSC_REQUIRE(n_structs >= 0 && n_quads >= 0 && d > 0 && k > 0 && num_active >= 0 && num_active <= n_structs && d * k <= n_structs,
                "bad pass geometry (n = %lld, d = %lld, k = %lld, active = %lld)", (long long)n_structs, (long long)d, (long long)k, (long long)num_active);
    TSC_REQUIRE(n_structs < INT32_MAX, "too many structures");
    if (n_structs == 0) return 0;
    HostCall h(c);
    float *d_tf;
    int32_t *d_first;
    TSC_TRY(h.in(tf, size_t(n_structs) * n_quads, &d_tf));
    TSC_TRY(h.out(first, size_t(n_structs), &d_first));
    hipLaunchKernelGGL(k_tfd_first_similar, dim3(grid_for(n_structs, 4, 256 * 16)), dim3(256), 0, c->stream, (const float *)d_tf, n_structs, n_quads, d, k,
                       num_active, thresh, d_first);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

// the graph step of the similarity prunings on the host (host_order.hpp): no device involved
extern "C" __attribute__((visibility("default"))) int tsc_host_graph_step(const int64_t *rel_i, const int64_t *rel_j, const int64_t *chunk_ptr,
                                                                          const int64_t *chunk_off, const int64_t *chunk_len, int64_t n_chunks,
                                                                          int64_t n_total, uint8_t *keep) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(rel_i && rel_j && chunk_ptr && chunk_off && chunk_len && keep && n_chunks >= 0 && n_total >= 0, "tsc_host_graph_step: bad argument");
    int64_t longest = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        TSC_REQUIRE(chunk_ptr[c + 1] >= chunk_ptr[c] && chunk_off[c] >= 0 && chunk_len[c] >= 0 && chunk_off[c] + chunk_len[c] <= n_total,
                    "chunk %lld: bad bounds", (long long)c);
        for (int64_t q = chunk_ptr[c]; q < chunk_ptr[c + 1]; ++q)
            TSC_REQUIRE(rel_i[q] >= 0 && rel_i[q] < chunk_len[c] && rel_j[q] >= 0 && rel_j[q] < chunk_len[c] && rel_i[q] != rel_j[q],
                        "match %lld lies outside its chunk", (long long)q);
        longest = std::max(longest, chunk_len[c]);
    }
    std::vector<int32_t> index_of(size_t(longest), -1);
    for (int64_t c = 0; c < n_chunks; ++c)
        tsc_host::graph_step_chunk(rel_i + chunk_ptr[c], rel_j + chunk_ptr[c], chunk_ptr[c + 1] - chunk_ptr[c], chunk_off[c], keep, index_of);
    return 0;
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// moments of inertia, embed scores

extern "C" __attribute__((visibility("default"))) int tsc_inertia_moments(tsc_ctx *c, const double *structures, int64_t n_structs, int n_atoms,
                                                                          const double *masses, double *out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && masses && out && n_structs >= 0 && n_atoms > 0, "tsc_inertia_moments: bad argument");
    if (n_structs == 0) return 0;
    HostCall h(c);
    double *d_s, *d_m, *d_o;
    TSC_TRY(h.in(structures, size_t(n_structs) * n_atoms * 3, &d_s));
    TSC_TRY(h.in(masses, size_t(n_atoms), &d_m));
    TSC_TRY(h.out(out, size_t(n_structs) * 3, &d_o));
    hipLaunchKernelGGL(k_inertia_moments, dim3(grid_for(n_structs, 256, 256 * 8)), dim3(256), 0, c->stream, (const double *)d_s, n_structs, n_atoms,
                       (const double *)d_m, d_o);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_moi_first_similar(tsc_ctx *c, const double *moments, int64_t n_structs, double max_deviation,
                                                                            int32_t *first) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && moments && first && n_structs >= 0 && n_structs < INT32_MAX, "tsc_moi_first_similar: bad argument");
    if (n_structs == 0) return 0;
    HostCall h(c);
    double *d_m;
    int32_t *d_f;
    TSC_TRY(h.in(moments, size_t(n_structs) * 3, &d_m));
    TSC_TRY(h.out(first, size_t(n_structs), &d_f));
    hipLaunchKernelGGL(k_moi_first_similar, dim3(grid_for(n_structs, 4, 256 * 16)), dim3(256), 0, c->stream, (const double *)d_m, n_structs, max_deviation, d_f);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_scores(tsc_ctx *c, const double *structures, int64_t n_structs, int n_atoms,
                                                                       const int32_t *indices, const double *distances, int n_c, float *scores,
                                                                       double *fitness_error) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && structures && indices && distances && scores && fitness_error && n_structs >= 0 && n_atoms > 0 && n_c >= 0, "tsc_embed_scores: bad argument");
    for (int64_t q = 0; q < n_structs * n_c * 2; ++q) TSC_REQUIRE(indices[q] >= 0 && indices[q] < n_atoms, "constrained index %d out of range", indices[q]);
    if (n_structs == 0) return 0;
    HostCall h(c);
    double *d_s, *d_d, *d_e;
    int32_t *d_i;
    float *d_sc;
    TSC_TRY(h.in(structures, size_t(n_structs) * n_atoms * 3, &d_s));
    TSC_TRY(h.in(indices, size_t(n_structs) * n_c * 2, &d_i));
    TSC_TRY(h.in(distances, size_t(n_structs) * n_c, &d_d));
    TSC_TRY(h.out(scores, size_t(n_structs), &d_sc));
    TSC_TRY(h.out(fitness_error, size_t(n_structs), &d_e));
    hipLaunchKernelGGL(k_embed_scores, dim3(grid_for(n_structs, 256, 256 * 8)), dim3(256), 0, c->stream, (const double *)d_s, n_structs, n_atoms,
                       (const int32_t *)d_i, (const double *)d_d, n_c, d_sc, d_e);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// string-embed pose parameters

extern "C" __attribute__((visibility("default"))) int tsc_string_embed_params_dev(tsc_ctx *c, const double *p1, const double *p2, const double *ref_vec,
                                                                                  const double *mol_vec, const int32_t *conf_pair, int64_t n_sites,
                                                                                  const double *angles, int n_angles, double *rot, double *pos,
                                                                                  int32_t *conf_idx) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && p1 && p2 && ref_vec && mol_vec && conf_pair && angles && rot && pos && conf_idx, "tsc_string_embed_params_dev: null argument");
    TSC_REQUIRE(n_sites >= 0 && n_angles >= 0, "bad sizes");
    if (n_sites == 0 || n_angles == 0) return 0;
    DeviceGuard guard(c->device);
    hipLaunchKernelGGL(k_string_embed_params, dim3(grid_for(n_sites * n_angles, 256, 256 * 8)), dim3(256), 0, c->stream, p1, p2, ref_vec, mol_vec,
                       conf_pair, n_sites, angles, n_angles, rot, pos, conf_idx);
    TSC_HIP(hipGetLastError());
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_string_embed_params(tsc_ctx *c, const double *p1, const double *p2, const double *ref_vec,
                                                                              const double *mol_vec, const int32_t *conf_pair, int64_t n_sites,
                                                                              const double *angles, int n_angles, double *rot, double *pos,
                                                                              int32_t *conf_idx) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && p1 && p2 && ref_vec && mol_vec && conf_pair && angles && rot && pos && conf_idx, "tsc_string_embed_params: null argument");
    TSC_REQUIRE(n_sites >= 0 && n_angles >= 0, "bad sizes");
    if (n_sites == 0 || n_angles == 0) return 0;
    HostCall h(c);
    double *d_p1, *d_p2, *d_rv, *d_mv, *d_ang, *d_rot, *d_pos;
    int32_t *d_cp, *d_ci;
    const size_t N = size_t(n_sites) * n_angles;
    TSC_TRY(h.in(p1, size_t(n_sites) * 3, &d_p1));
    TSC_TRY(h.in(p2, size_t(n_sites) * 3, &d_p2));
    TSC_TRY(h.in(ref_vec, size_t(n_sites) * 3, &d_rv));
    TSC_TRY(h.in(mol_vec, size_t(n_sites) * 3, &d_mv));
    TSC_TRY(h.in(conf_pair, size_t(n_sites) * 2, &d_cp));
    TSC_TRY(h.in(angles, size_t(n_angles), &d_ang));
    TSC_TRY(h.out(rot, N * 18, &d_rot));
    TSC_TRY(h.out(pos, N * 6, &d_pos));
    TSC_TRY(h.out(conf_idx, N * 2, &d_ci));
    TSC_TRY(tsc_string_embed_params_dev(c, d_p1, d_p2, d_rv, d_mv, d_cp, n_sites, d_ang, n_angles, d_rot, d_pos, d_ci));
    return h.finish();
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_cyclical_embed_params(tsc_ctx *c, const double *start, const double *end,
                                                                                const double *direction, const double *pivot, const double *meanpoint,
                                                                                const double *r0, const double *r1, const int32_t *n_reactive,
                                                                                const double *angle, int64_t n, double *rot, double *pos) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && start && end && direction && pivot && meanpoint && r0 && r1 && n_reactive && angle && rot && pos, "tsc_cyclical_embed_params: null argument");
    TSC_REQUIRE(n >= 0, "bad size");
    for (int64_t q = 0; q < n; ++q) TSC_REQUIRE(n_reactive[q] == 1 || n_reactive[q] == 2, "row %lld: n_reactive must be 1 or 2", (long long)q);
    if (n == 0) return 0;
    HostCall h(c);
    const double *host[7] = {start, end, direction, pivot, meanpoint, r0, r1};
    double *dev[7], *d_angle, *d_rot, *d_pos;
    int32_t *d_nr;
    for (int i = 0; i < 7; ++i) TSC_TRY(h.in(host[i], size_t(n) * 3, &dev[i]));
    TSC_TRY(h.in(n_reactive, size_t(n), &d_nr));
    TSC_TRY(h.in(angle, size_t(n), &d_angle));
    TSC_TRY(h.out(rot, size_t(n) * 9, &d_rot));
    TSC_TRY(h.out(pos, size_t(n) * 3, &d_pos));
    hipLaunchKernelGGL(k_cyclical_embed_params, dim3(grid_for(n, 256, 256 * 8)), dim3(256), 0, c->stream, (const double *)dev[0], (const double *)dev[1],
                       (const double *)dev[2], (const double *)dev[3], (const double *)dev[4], (const double *)dev[5], (const double *)dev[6],
                       (const int32_t *)d_nr, (const double *)d_angle, n, d_rot, d_pos);
    TSC_HIP(hipGetLastError());
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// the embed loops as drivers: string_embed (tscode/embeds.py:91-120) and cyclical_embed (:636-717, :771-847)

// is_new_structure over fingerprints on the device (tfd.hpp, tfd_kernels.hpp): super-blocks of TG_SUPER candidates, three launches each.
// d_acc u8[n], d_list i32[n], d_nk i32[1] (the number kept, on the device)
static int launch_tfd_greedy(tsc_ctx *c, Scratch &s, const float *d_tf, int64_t n, int T, double thresh, uint8_t *d_acc, int32_t *d_list, int32_t *d_nk) {
    TSC_REQUIRE(T <= 12288, "fingerprints of %d torsions: the greedy filter takes up to 12288", T);
    // per super-block: dead u8[TG_SUPER] and, right behind it, nz u64[TG_WORDS] -- one memset clears both
    uint8_t *d_flags;
    unsigned long long *d_sim;
    float *d_kfp;  // the kept fingerprints once more, compact and in the order they were kept (k_tfd_greedy_prior)
    TSC_TRY(s.get(size_t(TG_SUPER) + TG_WORDS * sizeof(unsigned long long), &d_flags));
    TSC_TRY(s.get(size_t(TG_SUPER) * TG_WORDS, &d_sim));
    TSC_TRY(s.get(std::max<size_t>(size_t(n) * T, 1), &d_kfp));
    int32_t *d_nk_before;
    TSC_TRY(s.get(1, &d_nk_before));
    unsigned long long *d_nz = reinterpret_cast<unsigned long long *>(d_flags + TG_SUPER);
    const size_t lds_pairs = 64 * T <= 12288 ? size_t(64) * std::max(T, 1) * sizeof(float) : 0;
    TSC_HIP(hipMemsetAsync(d_nk, 0, sizeof(int32_t), c->stream));
    for (int64_t base = 0; base < n; base += TG_SUPER) {
        const int nc = int(std::min<int64_t>(TG_SUPER, n - base));
        TSC_HIP(hipMemsetAsync(d_flags, 0, size_t(TG_SUPER) + TG_WORDS * sizeof(unsigned long long), c->stream));
        if (base > 0)
            hipLaunchKernelGGL(k_tfd_greedy_prior, dim3(ceil_div(nc, 256), 64), dim3(256), 0, c->stream, d_tf, base, nc, T, thresh, (const float *)d_kfp,
                               (const int32_t *)d_nk, d_flags);
        hipLaunchKernelGGL(k_tfd_greedy_pairs, dim3(TG_WORDS, ceil_div(nc, 256)), dim3(256), lds_pairs, c->stream, d_tf, base, nc, T, thresh, d_sim, d_nz);
        hipLaunchKernelGGL(k_tfd_greedy_replay, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)d_sim, (const unsigned long long *)d_nz, base, nc,
                           (const uint8_t *)d_flags, d_acc, d_list, d_nk, d_nk_before);
        if (base + TG_SUPER < n && T > 0)  // (the last super-block's fingerprints are compared with nothing any more)
            hipLaunchKernelGGL(k_tfd_greedy_keep, dim3(1), dim3(256), 0, c->stream, d_tf, T, (const int32_t *)d_list, (const int32_t *)d_nk_before,
                               (const int32_t *)d_nk, d_kfp);
    }
    TSC_HIP(hipGetLastError());
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_tfd_greedy_filter(tsc_ctx *c, const float *tf, int64_t n_structs, int n_quads, double thresh,
                                                                            uint8_t *accepted, int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && tf && accepted, "tsc_tfd_greedy_filter: null argument");
    TSC_REQUIRE(n_structs >= 0 && n_structs < INT32_MAX && n_quads >= 0, "bad sizes");
    if (n_kept) *n_kept = 0;
    if (n_structs == 0) return 0;
    int32_t nk = 0;
    HostCall h(c);
    float *d_tf;
    uint8_t *d_acc;
    int32_t *d_list, *d_nk;
    TSC_TRY(h.in(tf, std::max<size_t>(size_t(n_structs) * n_quads, 1), &d_tf));
    TSC_TRY(h.out(accepted, size_t(n_structs), &d_acc));
    TSC_TRY(h.scratch().get(size_t(n_structs), &d_list));
    TSC_TRY(h.scratch().get(1, &d_nk));
    TSC_TRY(launch_tfd_greedy(c, h.scratch(), d_tf, n_structs, n_quads, thresh, d_acc, d_list, d_nk));
    TSC_TRY(h.fetch(&nk, d_nk, 1));
    TSC_TRY(h.finish());
    if (n_kept) *n_kept = nk;
    return 0;
    TSC_API_GUARD_END
}

// What the embed drivers share once the pose parameters are on the device, in two halves.  The front half: clash verdicts of all candidates,
// the passing poses embedded in candidate order, a filter over them (`filter(d_structs, n_pass, d_pos_scan, d_total, d_acc)`), both verdicts
// per candidate (clash_ok fetched, kept registered with the call) and the two counts on the host.  What it leaves on the device, in blocks of
// the call's scratch, is what a back half reads: the passing poses and the two index lists.
struct EmbedFiltered {
    int32_t n_pass = 0, n_kept = 0;
    double *structs = nullptr;    // f64[n_pass, n, 3]: the passing poses, the very buffer the filter read
    int32_t *act = nullptr;       // i32[n_pass]: candidate of every passing pose
    int32_t *act2 = nullptr;      // i32[n_kept]: passing pose of every kept pose
    // (the group drivers: the parameters of every candidate, cyclical_groups_front)
    const int32_t *ci = nullptr;
    const double *rot = nullptr, *pos = nullptr;
};

template <typename Filter>
static int embed_filter_front(tsc_ctx *c, HostCall &h, const double *d_frags, const FragTable &ft, const int64_t *frag_off, const int32_t *n_atoms,
                              const int32_t *n_conf, const int32_t *d_ci, const double *d_rot, const double *d_pos, int64_t N, double clash_thresh,
                              int64_t max_clashes, uint8_t *clash_ok, uint8_t *kept, EmbedFiltered *f, Filter filter) {
    hipStream_t st = c->stream;
    Scratch &s = h.scratch();
    const int n = ft.n_total;
    uint8_t *d_mask, *d_kept_full, *d_acc;
    int32_t *bsum, *act, *pos_scan, *total, *act2, *total2;
    TSC_TRY(s.get(size_t(N), &d_mask));
    TSC_TRY(h.out(kept, size_t(N), &d_kept_full));
    TSC_TRY(s.get(scan_bsum_count(N), &bsum));
    TSC_TRY(s.get(size_t(N), &act));
    TSC_TRY(s.get(size_t(N) + 1, &pos_scan));
    TSC_TRY(s.get(1, &total));
    TSC_TRY(s.get(size_t(N), &act2));
    TSC_TRY(s.get(1, &total2));
    TSC_TRY(tsc_embed_clash_mask_dev(c, d_frags, frag_off, n_atoms, n_conf, ft.n_mols, d_ci, d_rot, d_pos, N, clash_thresh, max_clashes, d_mask, nullptr));
    TSC_TRY(scan_mask(st, d_mask, N, bsum, pos_scan, act, nullptr, total));
    TSC_TRY(h.fetch(clash_ok, d_mask, size_t(N)));   // (here, in front of the first wait)
    TSC_HIP(hipMemsetAsync(d_kept_full, 0, size_t(N), st));
    f->act = act, f->act2 = act2;
    TSC_TRY(read_i32(c, total, &f->n_pass));
    const int32_t n_pass = f->n_pass;
    if (n_pass > 0) {
        double *d_structs;
        TSC_TRY(s.get(size_t(n_pass) * n * 3, &d_structs));
        TSC_TRY(s.get(size_t(n_pass), &d_acc));
        hipLaunchKernelGGL(k_transform, dim3(grid_for(n_pass, TR_POSES, 256 * 64)), dim3(256), transform_lds_bytes(ft.n_mols), st, d_frags, ft, d_ci, d_rot, d_pos,
                           (const int32_t *)act, int64_t(n_pass), d_structs, (const int32_t *)nullptr, 0, (double *)nullptr, (const int32_t *)nullptr);
        TSC_HIP(hipGetLastError());
        f->structs = d_structs;
        TSC_TRY(filter(d_structs, n_pass, pos_scan, total, d_acc));
        hipLaunchKernelGGL(k_scatter_flags, dim3(grid_for(n_pass, 256, 1024)), dim3(256), 0, st, (const uint8_t *)d_acc, (const int32_t *)act, (const int32_t *)total,
                           d_kept_full);
        TSC_TRY(scan_mask(st, d_acc, n_pass, bsum, nullptr, act2, nullptr, total2));
        TSC_TRY(read_i32(c, total2, &f->n_kept));
    }
    return 0;
}

// The back half of the calls that hand the kept poses to the host: compacted, copied out, then the call's one wait for the stream.
static int embed_filter_fetch(tsc_ctx *c, HostCall &h, int n, const EmbedFiltered &f, double *poses, int64_t poses_capacity, int64_t *n_kept_out) {
    if (poses && f.n_kept > 0) {
        double *d_out;
        TSC_REQUIRE(f.n_kept <= poses_capacity, "poses holds %lld rows, %d poses were kept", (long long)poses_capacity, f.n_kept);
        TSC_TRY(h.scratch().get(size_t(f.n_kept) * n * 3, &d_out));
        TSC_TRY(launch_gather_rows(c->stream, f.structs, f.act2, f.n_kept, n * 3, nullptr, n * 3, d_out));
        TSC_TRY(h.fetch(poses, d_out, size_t(f.n_kept) * n * 3));
    }
    TSC_TRY(h.finish());
    *n_kept_out = f.n_kept;
    return 0;
}

template <typename Filter>
static int embed_filter_run(tsc_ctx *c, HostCall &h, const double *d_frags, const FragTable &ft, const int64_t *frag_off, const int32_t *n_atoms,
                            const int32_t *n_conf, const int32_t *d_ci, const double *d_rot, const double *d_pos, int64_t N, double clash_thresh,
                            int64_t max_clashes, uint8_t *clash_ok, uint8_t *kept, double *poses, int64_t poses_capacity, int64_t *n_pass_out,
                            int64_t *n_kept_out, Filter filter) {
    EmbedFiltered f;
    const int rc = embed_filter_front(c, h, d_frags, ft, frag_off, n_atoms, n_conf, d_ci, d_rot, d_pos, N, clash_thresh, max_clashes, clash_ok, kept, &f, filter);
    *n_pass_out = f.n_pass;
    TSC_TRY(rc);
    return embed_filter_fetch(c, h, ft.n_total, f, poses, poses_capacity, n_kept_out);
}

extern "C" __attribute__((visibility("default"))) int tsc_string_embed(tsc_ctx *c, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                                                                       const int32_t *n_conf, const double *p1, const double *p2, const double *ref_vec,
                                                                       const double *mol_vec, const int32_t *conf_pair, int64_t n_sites, const double *angles,
                                                                       int n_angles, double clash_thresh, int64_t max_clashes, const int32_t *quads, int n_quads,
                                                                       double tfd_thresh, uint8_t *clash_ok, uint8_t *kept, double *poses,
                                                                       int64_t poses_capacity, int64_t *n_pass, int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && frags && frag_off && n_atoms && n_conf && p1 && p2 && ref_vec && mol_vec && conf_pair && angles && clash_ok && kept && n_pass && n_kept,
                "tsc_string_embed: null argument");
    TSC_REQUIRE(n_sites >= 0 && n_angles >= 0 && n_quads >= 0 && (n_quads == 0 || quads), "bad sizes");
    const int64_t N = n_sites * n_angles;
    TSC_REQUIRE(N < INT32_MAX, "too many candidates");
    *n_pass = *n_kept = 0;
    if (N == 0) return 0;
    FragTable ft;
    TSC_TRY(make_frag_table(frag_off, n_atoms, n_conf, 2, &ft));
    for (int64_t q = 0; q < n_sites; ++q)
        TSC_REQUIRE(conf_pair[2 * q] >= 0 && conf_pair[2 * q] < n_conf[0] && conf_pair[2 * q + 1] >= 0 && conf_pair[2 * q + 1] < n_conf[1],
                    "site %lld: conformer index out of range", (long long)q);
    for (int q = 0; q < 4 * n_quads; ++q) TSC_REQUIRE(quads[q] >= 0 && quads[q] < ft.n_total, "quadruplet atom index %d out of range", quads[q]);
    HostCall h(c);
    Scratch &s = h.scratch();
    double *d_frags, *d_p1, *d_p2, *d_rv, *d_mv, *d_ang, *d_rot, *d_pos;
    int32_t *d_cp, *d_ci, *d_quads = nullptr;
    TSC_TRY(h.in(frags, size_t(frags_total_doubles(frag_off, n_atoms, n_conf, 2)), &d_frags));
    TSC_TRY(h.in(p1, size_t(n_sites) * 3, &d_p1));
    TSC_TRY(h.in(p2, size_t(n_sites) * 3, &d_p2));
    TSC_TRY(h.in(ref_vec, size_t(n_sites) * 3, &d_rv));
    TSC_TRY(h.in(mol_vec, size_t(n_sites) * 3, &d_mv));
    TSC_TRY(h.in(conf_pair, size_t(n_sites) * 2, &d_cp));
    TSC_TRY(h.in(angles, size_t(n_angles), &d_ang));
    if (n_quads) TSC_TRY(h.in(quads, size_t(n_quads) * 4, &d_quads));
    TSC_TRY(s.get(size_t(N) * 18, &d_rot));
    TSC_TRY(s.get(size_t(N) * 6, &d_pos));
    TSC_TRY(s.get(size_t(N) * 2, &d_ci));
    TSC_TRY(tsc_string_embed_params_dev(c, d_p1, d_p2, d_rv, d_mv, d_cp, n_sites, d_ang, n_angles, d_rot, d_pos, d_ci));
    const int n = ft.n_total;
    // is_new_structure (:47-69, :119): torsion fingerprints of the passing poses, then the greedy filter over the whole list
    auto filter = [&](const double *d_structs, int32_t np, const int32_t *, const int32_t *, uint8_t *d_acc) -> int {
        float *d_tf;
        int32_t *d_list, *d_nk;
        TSC_TRY(s.get(std::max<size_t>(size_t(np) * n_quads, 1), &d_tf));
        TSC_TRY(s.get(size_t(np), &d_list));
        TSC_TRY(s.get(1, &d_nk));
        if (n_quads)
            hipLaunchKernelGGL(k_torsion_fingerprints, dim3(grid_for(int64_t(np) * n_quads, 256, 256 * 8)), dim3(256), 0, c->stream, d_structs, int64_t(np), n,
                               (const int32_t *)d_quads, n_quads, d_tf);
        TSC_HIP(hipGetLastError());
        return launch_tfd_greedy(c, s, d_tf, int64_t(np), n_quads, tfd_thresh, d_acc, d_list, d_nk);
    };
    return embed_filter_run(c, h, d_frags, ft, frag_off, n_atoms, n_conf, d_ci, d_rot, d_pos, N, clash_thresh, max_clashes, clash_ok, kept, poses, poses_capacity,
                            n_pass, n_kept, filter);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_cyclical_embed(tsc_ctx *c, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                                                                         const int32_t *n_conf, int n_mols, const double *start, const double *end,
                                                                         const double *direction, const double *pivot, const double *meanpoint, const double *r0,
                                                                         const double *r1, const int32_t *n_reactive, const double *angle, const int32_t *conf_idx,
                                                                         int64_t n_poses, const int32_t *group_off, int n_groups, double clash_thresh,
                                                                         int64_t max_clashes, double rmsd_thr, uint8_t *clash_ok, uint8_t *kept, double *poses,
                                                                         int64_t poses_capacity, int64_t *n_pass, int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && frags && frag_off && n_atoms && n_conf && start && end && direction && pivot && meanpoint && r0 && r1 && n_reactive && angle && conf_idx &&
                    group_off && clash_ok && kept && n_pass && n_kept,
                "tsc_cyclical_embed: null argument");
    TSC_REQUIRE(n_poses >= 0 && n_poses < INT32_MAX && n_groups >= 0 && rmsd_thr > 0, "bad sizes");
    *n_pass = *n_kept = 0;
    if (n_poses == 0) return 0;
    FragTable ft;
    TSC_TRY(make_frag_table(frag_off, n_atoms, n_conf, n_mols, &ft));
    const int64_t rows = n_poses * n_mols;
    for (int64_t q = 0; q < rows; ++q) {
        TSC_REQUIRE(n_reactive[q] == 1 || n_reactive[q] == 2, "row %lld: n_reactive must be 1 or 2", (long long)q);
        TSC_REQUIRE(conf_idx[q] >= 0 && conf_idx[q] < n_conf[q % n_mols], "row %lld: conformer index out of range", (long long)q);
    }
    TSC_REQUIRE(n_groups > 0 && group_off[0] == 0 && group_off[n_groups] == n_poses, "group_off must run from 0 to n_poses");
    for (int g = 0; g < n_groups; ++g)
        TSC_REQUIRE(group_off[g + 1] >= group_off[g] && group_off[g + 1] - group_off[g] <= GF_MAX_GROUP, "group %d: sizes must be in [0, %d]", g, GF_MAX_GROUP);
    HostCall h(c);
    Scratch &s = h.scratch();
    const double *host[7] = {start, end, direction, pivot, meanpoint, r0, r1};
    double *d_frags, *dev[7], *d_angle, *d_rot, *d_pos;
    int32_t *d_nr, *d_ci, *d_goff, *d_goff_pass;
    TSC_TRY(h.in(frags, size_t(frags_total_doubles(frag_off, n_atoms, n_conf, n_mols)), &d_frags));
    for (int i = 0; i < 7; ++i) TSC_TRY(h.in(host[i], size_t(rows) * 3, &dev[i]));
    TSC_TRY(h.in(n_reactive, size_t(rows), &d_nr));
    TSC_TRY(h.in(angle, size_t(rows), &d_angle));
    TSC_TRY(h.in(conf_idx, size_t(rows), &d_ci));
    TSC_TRY(h.in(group_off, size_t(n_groups) + 1, &d_goff));
    TSC_TRY(s.get(size_t(n_groups) + 1, &d_goff_pass));
    TSC_TRY(s.get(size_t(rows) * 9, &d_rot));
    TSC_TRY(s.get(size_t(rows) * 3, &d_pos));
    hipLaunchKernelGGL(k_cyclical_embed_params, dim3(grid_for(rows, 256, 256 * 8)), dim3(256), 0, c->stream, (const double *)dev[0], (const double *)dev[1],
                       (const double *)dev[2], (const double *)dev[3], (const double *)dev[4], (const double *)dev[5], (const double *)dev[6],
                       (const int32_t *)d_nr, (const double *)d_angle, rows, d_rot, d_pos);
    TSC_HIP(hipGetLastError());
    const int n = ft.n_total;
    // not _rmsd_similarity(pose, angular_poses, rmsd_thr=1) (:715, :843): greedy inside each group of passing poses
    auto filter = [&](const double *d_structs, int32_t np, const int32_t *pos_scan, const int32_t *total, uint8_t *d_acc) -> int {
        hipLaunchKernelGGL(k_group_offsets_after_filter, dim3(grid_for(n_groups + 1, 256, 1024)), dim3(256), 0, c->stream, (const int32_t *)d_goff, n_groups, pos_scan,
                           n_poses, total, d_goff_pass);
        TSC_HIP(hipGetLastError());
        return tsc_greedy_group_filter_dev(c, d_structs, d_goff_pass, n_groups, np, n, rmsd_thr, d_acc);
    };
    return embed_filter_run(c, h, d_frags, ft, frag_off, n_atoms, n_conf, d_ci, d_rot, d_pos, n_poses, clash_thresh, max_clashes, clash_ok, kept, poses,
                            poses_capacity, n_pass, n_kept, filter);
    TSC_API_GUARD_END
}

// What tsc_cyclical_embed_groups and a slab of an embed-and-prune run (tsc_embed_prune_add_groups) share.  The checks of one slab of groups,
// in two steps around the caller's "no groups: nothing to do":
static int check_group_slab_sizes(int64_t n_groups, int n_angles, double rmsd_thr) {
    TSC_REQUIRE(n_angles >= 1 && n_angles <= GF_MAX_GROUP, "%d angle sets per group: must be in [1, %d]", n_angles, GF_MAX_GROUP);
    TSC_REQUIRE(n_groups >= 0 && n_groups < INT32_MAX / n_angles, "%lld groups of %d poses: too many candidates", (long long)n_groups, n_angles);
    TSC_REQUIRE(rmsd_thr > 0, "bad sizes");
    return 0;
}
static int check_group_slab_records(const int32_t *n_conf, int n_mols, const int32_t *n_reactive, const int32_t *conf_idx, int64_t n_groups) {
    for (int64_t q = 0; q < n_groups * n_mols; ++q) {
        TSC_REQUIRE(n_reactive[q] == 1 || n_reactive[q] == 2, "group %lld, molecule %d: n_reactive must be 1 or 2", (long long)(q / n_mols), int(q % n_mols));
        TSC_REQUIRE(conf_idx[q] >= 0 && conf_idx[q] < n_conf[q % n_mols], "group %lld, molecule %d: conformer index out of range", (long long)(q / n_mols),
                    int(q % n_mols));
    }
    return 0;
}

// ... and the device work of one slab up to the kept flags: the records uploaded, the parameters of every pose, then embed_filter_front with
// the greedy filter inside each group.  d_frags is on the device already (uploaded by the call, or once by the run).  `goff` is the caller's,
// declared in front of its HostCall: it is uploaded from and must outlive the call's last wait.
static int cyclical_groups_front(tsc_ctx *c, HostCall &h, std::vector<int32_t> &goff, const double *d_frags, const FragTable &ft, const int64_t *frag_off,
                                 const int32_t *n_atoms, const int32_t *n_conf, const double *const host[7], const int32_t *n_reactive, const int32_t *conf_idx,
                                 const double *angles, int64_t n_groups, int n_angles, double clash_thresh, int64_t max_clashes, double rmsd_thr,
                                 uint8_t *clash_ok, uint8_t *kept, EmbedFiltered *f) {
    const int n_mols = ft.n_mols;
    const int64_t items = n_groups * n_mols, n_poses = n_groups * n_angles, rows = n_poses * n_mols;
    goff.resize(size_t(n_groups) + 1);
    for (int64_t g = 0; g <= n_groups; ++g) goff[size_t(g)] = int32_t(g * n_angles);
    Scratch &s = h.scratch();
    double *dev[7], *d_angles, *d_rot, *d_pos;
    int32_t *d_nr, *d_cg, *d_ci, *d_goff, *d_goff_pass;
    for (int i = 0; i < 7; ++i) TSC_TRY(h.in(host[i], size_t(items) * 3, &dev[i]));
    TSC_TRY(h.in(n_reactive, size_t(items), &d_nr));
    TSC_TRY(h.in(conf_idx, size_t(items), &d_cg));
    TSC_TRY(h.in(angles, size_t(n_angles) * n_mols, &d_angles));
    TSC_TRY(h.in(goff.data(), size_t(n_groups) + 1, &d_goff));
    TSC_TRY(s.get(size_t(n_groups) + 1, &d_goff_pass));
    TSC_TRY(s.get(size_t(rows) * 9, &d_rot));
    TSC_TRY(s.get(size_t(rows) * 3, &d_pos));
    TSC_TRY(s.get(size_t(rows), &d_ci));
    // a wavefront per chunk of 64 / n_mols groups, four per workgroup; 768 workgroups fill 256 CUs at the three waves per SIMD the kernel's
    // registers allow, and more chunks than that are walked in further passes
    hipLaunchKernelGGL(k_cyclical_embed_group_params, dim3(grid_for(ceil_div(n_groups, int64_t(64 / n_mols)), CGP_WAVES, 768)), dim3(64 * CGP_WAVES), 0, c->stream,
                       (const double *)dev[0], (const double *)dev[1], (const double *)dev[2], (const double *)dev[3], (const double *)dev[4],
                       (const double *)dev[5], (const double *)dev[6], (const int32_t *)d_nr, (const int32_t *)d_cg, (const double *)d_angles, n_groups, n_mols,
                       n_angles, d_rot, d_pos, d_ci);
    TSC_HIP(hipGetLastError());
    f->ci = d_ci, f->rot = d_rot, f->pos = d_pos;
    const int n = ft.n_total;
    const int ng = int(n_groups);
    auto filter = [&](const double *d_structs, int32_t np, const int32_t *pos_scan, const int32_t *total, uint8_t *d_acc) -> int {
        hipLaunchKernelGGL(k_group_offsets_after_filter, dim3(grid_for(ng + 1, 256, 1024)), dim3(256), 0, c->stream, (const int32_t *)d_goff, ng, pos_scan, n_poses,
                           total, d_goff_pass);
        TSC_HIP(hipGetLastError());
        return tsc_greedy_group_filter_dev(c, d_structs, d_goff_pass, ng, np, n, rmsd_thr, d_acc);
    };
    return embed_filter_front(c, h, d_frags, ft, frag_off, n_atoms, n_conf, d_ci, d_rot, d_pos, n_poses, clash_thresh, max_clashes, clash_ok, kept, f, filter);
}

// The same embed from one record per (group, molecule) and one angle table shared by all groups: pose g * n_angles + a is record g under
// angle set a, what tsc_cyclical_embed computes on the rows a caller would expand from them.  Per pose nothing is uploaded or checked.
extern "C" __attribute__((visibility("default"))) int tsc_cyclical_embed_groups(tsc_ctx *c, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                                                                                const int32_t *n_conf, int n_mols, const double *start, const double *end,
                                                                                const double *direction, const double *pivot, const double *meanpoint,
                                                                                const double *r0, const double *r1, const int32_t *n_reactive,
                                                                                const int32_t *conf_idx, const double *angles, int64_t n_groups, int n_angles,
                                                                                double clash_thresh, int64_t max_clashes, double rmsd_thr, uint8_t *clash_ok,
                                                                                uint8_t *kept, double *poses, int64_t poses_capacity, int64_t *n_pass,
                                                                                int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && frags && frag_off && n_atoms && n_conf && start && end && direction && pivot && meanpoint && r0 && r1 && n_reactive && conf_idx && angles &&
                    clash_ok && kept && n_pass && n_kept,
                "tsc_cyclical_embed_groups: null argument");
    TSC_REQUIRE(n_mols == 2 || n_mols == 3, "tsc_cyclical_embed_groups: %d molecules, the cyclical embed takes 2 or 3", n_mols);
    TSC_TRY(check_group_slab_sizes(n_groups, n_angles, rmsd_thr));
    *n_pass = *n_kept = 0;
    if (n_groups == 0) return 0;
    FragTable ft;
    TSC_TRY(make_frag_table(frag_off, n_atoms, n_conf, n_mols, &ft));
    TSC_TRY(check_group_slab_records(n_conf, n_mols, n_reactive, conf_idx, n_groups));
    std::vector<int32_t> goff;
    HostCall h(c);
    const double *host[7] = {start, end, direction, pivot, meanpoint, r0, r1};
    double *d_frags;
    TSC_TRY(h.in(frags, size_t(frags_total_doubles(frag_off, n_atoms, n_conf, n_mols)), &d_frags));
    EmbedFiltered f;
    const int rc = cyclical_groups_front(c, h, goff, d_frags, ft, frag_off, n_atoms, n_conf, host, n_reactive, conf_idx, angles, n_groups, n_angles, clash_thresh,
                                         max_clashes, rmsd_thr, clash_ok, kept, &f);
    *n_pass = f.n_pass;
    TSC_TRY(rc);
    return embed_filter_fetch(c, h, ft.n_total, f, poses, poses_capacity, n_kept);
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// the groups of a three-molecule cyclical embed (trimolecular.hpp; tscode/embeds.py:312-465 inside the loop of :636-655)

// HIP-event time of the kernel of the calling thread's latest tsc_trimolecular_groups, taken only under the context option "pass_timing" >= 1
// (tools/trimolecular_profile.py); -1 otherwise
static thread_local float g_trimolecular_ms = -1.f;

extern "C" __attribute__((visibility("default"))) int tsc_trimolecular_groups_timings(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "tsc_trimolecular_groups_timings: null argument");
    *ms = g_trimolecular_ms;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_trimolecular_groups(
    tsc_ctx *c, const double *frags, const int64_t *frag_off, const int32_t *n_atoms, const int32_t *n_conf, const int32_t *reactive, const int32_t *n_reactive,
    const int64_t *reactive_cumnums, const int32_t *n_rows, const int32_t *conf, const double *pivot, const double *meanpoint, const int64_t *cumnums,
    const double *tri_poly, const double *tri_cost, const double *directions, const uint8_t *mask, const int64_t *base, int64_t n_triples, int64_t n_groups,
    double *blocks, int64_t *group_ids, int32_t *best) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && frags && frag_off && n_atoms && n_conf && reactive && n_reactive && reactive_cumnums && n_rows, "tsc_trimolecular_groups: null argument");
    TSC_REQUIRE(n_triples >= 0 && n_groups >= 0 && n_groups < INT32_MAX, "tsc_trimolecular_groups: %lld triples, %lld groups", (long long)n_triples,
                (long long)n_groups);
    FragTable ft;
    TSC_TRY(make_frag_table(frag_off, n_atoms, n_conf, 3, &ft));
    TriTables tb;
    memset(&tb, 0, sizeof(tb));
    const int64_t *row = reactive_cumnums;
    for (int m = 0; m < 3; ++m) {
        tb.frag_off[m] = frag_off[m], tb.n_atoms[m] = n_atoms[m], tb.n_reactive[m] = n_reactive[m], tb.n_rows[m] = n_rows[m];
        TSC_REQUIRE(n_reactive[m] == 1 || n_reactive[m] == 2, "tsc_trimolecular_groups: molecule %d has %d reactive atoms, must be 1 or 2", m, n_reactive[m]);
        for (int k = 0; k < n_reactive[m]; ++k) {
            TSC_REQUIRE(reactive[2 * m + k] >= 0 && reactive[2 * m + k] < n_atoms[m], "tsc_trimolecular_groups: reactive atom %d of molecule %d with %d atoms",
                        reactive[2 * m + k], m, n_atoms[m]);
            tb.reactive[m][k] = reactive[2 * m + k];
        }
        TSC_REQUIRE(n_rows[m] >= 0 && n_rows[m] <= TG_MAX_ROWS, "tsc_trimolecular_groups: molecule %d has %d reactive_cumnums rows, at most %d are taken", m,
                    n_rows[m], TG_MAX_ROWS);
        for (int r = 0; r < n_rows[m]; ++r, row += 2) {
            TSC_REQUIRE(row[0] >= 0 && row[0] < n_atoms[m], "tsc_trimolecular_groups: reactive_cumnums row %d of molecule %d names atom %lld of %d", r, m,
                        (long long)row[0], n_atoms[m]);
            tb.row_atom[m][r] = int(row[0]), tb.row_cum[m][r] = row[1];
        }
    }
    g_trimolecular_ms = -1.f;
    if (n_triples == 0) {
        TSC_REQUIRE(n_groups == 0, "tsc_trimolecular_groups: %lld groups from no triple", (long long)n_groups);
        return 0;
    }
    TSC_REQUIRE(conf && pivot && meanpoint && cumnums && tri_poly && tri_cost && directions && mask && base, "tsc_trimolecular_groups: null argument");
    TSC_REQUIRE(n_groups == 0 || (blocks && group_ids && best), "tsc_trimolecular_groups: null output");
    // a group's slot is base[triple] + the orientation's rank among the mask's bits: the bases must be the masks' running count, or a record
    // would land outside the outputs
    int64_t running = 0;
    for (int64_t t = 0; t < n_triples; ++t) {
        TSC_REQUIRE(base[t] == running, "tsc_trimolecular_groups: triple %lld: base %lld, the orientation masks in front of it count %lld", (long long)t,
                    (long long)base[t], (long long)running);
        running += __builtin_popcount(mask[t]);
        for (int m = 0; m < 3; ++m)
            TSC_REQUIRE(conf[3 * t + m] >= 0 && conf[3 * t + m] < n_conf[m], "tsc_trimolecular_groups: triple %lld, molecule %d: conformer %d of %d",
                        (long long)t, m, conf[3 * t + m], n_conf[m]);
        if (!mask[t]) continue;
        // over the orientations every cumnum of the three pivots turns up in some pair of `ids`: each must be some molecule's reactive atom
        for (int q = 0; q < 6; ++q) {
            bool found = false;
            for (int m = 0; m < 3 && !found; ++m)
                for (int r = 0; r < tb.n_rows[m] && !found; ++r) found = tb.row_cum[m][r] == cumnums[6 * t + q];
            TSC_REQUIRE(found, "tsc_trimolecular_groups: triple %lld: cumnum %lld of molecule %d's pivot is in no molecule's reactive_cumnums", (long long)t,
                        (long long)cumnums[6 * t + q], q / 2);
        }
    }
    TSC_REQUIRE(running == n_groups, "tsc_trimolecular_groups: the orientation masks count %lld groups, n_groups is %lld", (long long)running, (long long)n_groups);
    if (n_groups == 0) return 0;
    HostCall h(c);
    const size_t T = size_t(n_triples), G = size_t(n_groups);
    const double *d_frags, *d_pivot, *d_mean, *d_poly, *d_cost, *d_dir;
    const int32_t *d_conf;
    const int64_t *d_cum, *d_base;
    const uint8_t *d_mask;
    double *d_blocks;
    int64_t *d_ids;
    int32_t *d_best;
    TSC_TRY(h.in(frags, size_t(frags_total_doubles(frag_off, n_atoms, n_conf, 3)), &d_frags));
    TSC_TRY(h.in(conf, T * 3, &d_conf));
    TSC_TRY(h.in(pivot, T * 9, &d_pivot));
    TSC_TRY(h.in(meanpoint, T * 9, &d_mean));
    TSC_TRY(h.in(cumnums, T * 6, &d_cum));
    TSC_TRY(h.in(tri_poly, T * 9, &d_poly));
    TSC_TRY(h.in(tri_cost, T * 9, &d_cost));
    TSC_TRY(h.in(directions, T * 9, &d_dir));
    TSC_TRY(h.in(mask, T, &d_mask));
    TSC_TRY(h.in(base, T, &d_base));
    TSC_TRY(h.out(blocks, G * 3 * TG_RECORD, &d_blocks));
    TSC_TRY(h.out(group_ids, G * 6, &d_ids));
    TSC_TRY(h.out(best, G, &d_best));
    StageTimer tm(c);
    tm.begin();
    // a wavefront per triple, TG_WAVES per workgroup; 512 workgroups are two per CU, and more triples than that are walked in further passes
    hipLaunchKernelGGL(k_trimolecular_groups, dim3(grid_for(n_triples, TG_WAVES, 512)), dim3(64 * TG_WAVES), 0, c->stream, d_frags, tb, d_conf, d_pivot, d_mean,
                       d_cum, d_poly, d_cost, d_dir, d_mask, d_base, n_triples, d_blocks, d_ids, d_best);
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_trimolecular_ms);
    TSC_HIP(launched);
    return h.finish();
    TSC_API_GUARD_END
}

// --------------------------------------------------------------------------------------------------
// a cyclical embed whose kept poses are pruned by RMSD where they are (tscode/embeds.py:657-717 / :785-847, then tscode/rmsd_pruning.py:164-206)
//
// The run owns, on the device: the fragment stacks; and per kept pose, in candidate order over all slabs, its heavy atoms (what the prune
// reads) and its parameters (what the pose is embedded from again once the prune has spoken).  Nothing per pose crosses to the host but two
// flag bytes per candidate and, at the end, the poses that were asked for.

struct tsc_embed_prune : Owned {
    using Owned::Owned;
    FragTable ft{};
    int64_t frag_off[MAX_MOLS] = {};
    int32_t n_atoms[MAX_MOLS] = {}, n_conf[MAX_MOLS] = {};
    int n_heavy = 0;
    double *frags = nullptr;
    int32_t *sel = nullptr;          // i32[n_heavy * 3]: the doubles of a pose that are its heavy atoms' (launch_gather_rows)
    double *heavy = nullptr, *rot = nullptr, *pos = nullptr;   // f64[cap, n_heavy * 3], [cap, n_mols * 9], [cap, n_mols * 3]
    int32_t *ci = nullptr;           // i32[cap, n_mols]
    uint8_t *survived = nullptr;     // u8[n_kept] once tsc_embed_prune_run has run
    int64_t cap = 0, n_kept = 0, n_survived = 0;
    bool pruned = false;
};

// cand[r] = act[act2[r]]: the candidate of every kept pose, from the candidate of every passing pose and the passing pose of every kept one
static __global__ __launch_bounds__(256) void k_kept_candidates(const int32_t *__restrict__ act, const int32_t *__restrict__ act2, int n_kept,
                                                                int32_t *__restrict__ cand) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n_kept; r += gridDim.x * 256) cand[r] = act[act2[r]];
}

// dst[r][w] = src[idx[r]][w] for rows of `row` 32-bit words (k_gather_rows moves 64-bit words; a row of three conformer indices is 12 bytes)
static __global__ __launch_bounds__(256) void k_gather_rows_i32(const int32_t *__restrict__ src, const int32_t *__restrict__ idx, int64_t n_out, int row,
                                                                int32_t *__restrict__ dst) {
    const int64_t total = n_out * row;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t r = e / row;
        dst[e] = src[int64_t(idx[r]) * row + (e - r * row)];
    }
}

// room for `need` rows in the run's four buffers: what they hold moves to blocks twice the size (embed_prune_plan.hpp), on the stream
static int embed_prune_reserve(tsc_embed_prune *r, int64_t need) {
    tsc_ctx *c = r->ctx;
    const int64_t cap = ep_grown_capacity(r->cap, need);
    TSC_REQUIRE(cap >= 0, "tsc_embed_prune_add_groups: %lld kept poses are more than a prune takes (%lld)", (long long)need, (long long)EP_MAX_ROWS);
    if (cap == r->cap) return 0;
    const int nm = r->ft.n_mols;
    const size_t row_bytes[4] = {size_t(r->n_heavy) * 24, size_t(nm) * 72, size_t(nm) * 24, size_t(nm) * 4};
    void *old[4] = {r->heavy, r->rot, r->pos, r->ci}, *grown[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < 4 && !rc; ++i) rc = r->take(size_t(cap) * row_bytes[i], &grown[i]);
    for (int i = 0; i < 4 && !rc; ++i)
        if (r->n_kept > 0 && hipMemcpyAsync(grown[i], old[i], size_t(r->n_kept) * row_bytes[i], hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = fail(TSC_ERR_HIP, "tsc_embed_prune_add_groups: the copy into the grown buffers failed");
    // the run keeps one set of four: the old ones are recycled in stream order, behind the copies
    void *const *gone = rc ? grown : old;
    for (int i = 0; i < 4; ++i) r->give_back(gone[i]);
    if (rc) return rc;
    r->heavy = static_cast<double *>(grown[0]), r->rot = static_cast<double *>(grown[1]), r->pos = static_cast<double *>(grown[2]);
    r->ci = static_cast<int32_t *>(grown[3]);
    r->cap = cap;
    return 0;
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_destroy(tsc_embed_prune *r) {
    TSC_API_GUARD_BEGIN
    return destroy_owned(r);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_create(tsc_ctx *c, const double *frags, const int64_t *frag_off, const int32_t *n_atoms,
                                                                             const int32_t *n_conf, int n_mols, const int32_t *heavy_idx, int n_heavy,
                                                                             tsc_embed_prune **out) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && frags && frag_off && n_atoms && n_conf && heavy_idx && out, "tsc_embed_prune_create: null argument");
    *out = nullptr;
    TSC_REQUIRE(n_mols == 2 || n_mols == 3, "tsc_embed_prune_create: %d molecules, the cyclical embed takes 2 or 3", n_mols);
    FragTable ft;
    TSC_TRY(make_frag_table(frag_off, n_atoms, n_conf, n_mols, &ft));
    TSC_REQUIRE(n_heavy >= 1 && n_heavy <= ft.n_total, "tsc_embed_prune_create: %d heavy atoms of %d atoms: at least one, at most all", n_heavy, ft.n_total);
    std::vector<int32_t> sel(size_t(n_heavy) * 3);
    for (int a = 0; a < n_heavy; ++a) {
        TSC_REQUIRE(heavy_idx[a] >= 0 && heavy_idx[a] < ft.n_total, "tsc_embed_prune_create: heavy_idx[%d] = %d is not an atom of the %d", a, heavy_idx[a],
                    ft.n_total);
        TSC_REQUIRE(a == 0 || heavy_idx[a] > heavy_idx[a - 1], "tsc_embed_prune_create: heavy_idx[%d] = %d does not increase", a, heavy_idx[a]);
        for (int k = 0; k < 3; ++k) sel[size_t(a) * 3 + k] = heavy_idx[a] * 3 + k;
    }
    // the run's blocks are the call's until everything is in place: an error hands them back behind an idle stream
    HostCall h(c);
    std::unique_ptr<tsc_embed_prune> run(new tsc_embed_prune(c));
    run->ft = ft, run->n_heavy = n_heavy;
    for (int m = 0; m < n_mols; ++m) run->frag_off[m] = frag_off[m], run->n_atoms[m] = n_atoms[m], run->n_conf[m] = n_conf[m];
    TSC_TRY(h.in(frags, size_t(frags_total_doubles(frag_off, n_atoms, n_conf, n_mols)), &run->frags));
    TSC_TRY(h.in(sel.data(), sel.size(), &run->sel));
    TSC_TRY(h.finish());
    run->take_blocks(h.scratch());
    c->owned.adopt(run.get());   // (listed once complete: destroyed with the context, tsc_ctx_destroy)
    *out = run.release();
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_add_groups(tsc_embed_prune *r, const double *start, const double *end, const double *direction,
                                                                                 const double *pivot, const double *meanpoint, const double *r0, const double *r1,
                                                                                 const int32_t *n_reactive, const int32_t *conf_idx, const double *angles,
                                                                                 int64_t n_groups, int n_angles, double clash_thresh, int64_t max_clashes,
                                                                                 double rmsd_thr_filter, uint8_t *clash_ok, uint8_t *kept, int64_t *n_pass,
                                                                                 int64_t *n_kept) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && start && end && direction && pivot && meanpoint && r0 && r1 && n_reactive && conf_idx && angles && clash_ok && kept && n_pass && n_kept,
                "tsc_embed_prune_add_groups: null argument");
    if (r->pruned) return fail(TSC_ERR_STATE, "tsc_embed_prune_add_groups: the run has been pruned (tsc_embed_prune_run); a further slab needs a new run");
    TSC_TRY(check_group_slab_sizes(n_groups, n_angles, rmsd_thr_filter));
    *n_pass = *n_kept = 0;
    if (n_groups == 0) return 0;
    tsc_ctx *c = r->ctx;
    const int n_mols = r->ft.n_mols, n = r->ft.n_total;
    TSC_TRY(check_group_slab_records(r->n_conf, n_mols, n_reactive, conf_idx, n_groups));
    std::vector<int32_t> goff;
    HostCall h(c);
    const double *host[7] = {start, end, direction, pivot, meanpoint, r0, r1};
    EmbedFiltered f;
    const int rc = cyclical_groups_front(c, h, goff, r->frags, r->ft, r->frag_off, r->n_atoms, r->n_conf, host, n_reactive, conf_idx, angles, n_groups, n_angles,
                                         clash_thresh, max_clashes, rmsd_thr_filter, clash_ok, kept, &f);
    *n_pass = f.n_pass;
    TSC_TRY(rc);
    if (f.n_kept > 0) {
        // the kept poses' heavy atoms out of the buffer the filter read, and their parameters, behind what earlier slabs left
        TSC_TRY(embed_prune_reserve(r, r->n_kept + f.n_kept));
        int32_t *cand;
        TSC_TRY(h.scratch().get(size_t(f.n_kept), &cand));
        hipLaunchKernelGGL(k_kept_candidates, dim3(grid_for(f.n_kept, 256, 1024)), dim3(256), 0, c->stream, (const int32_t *)f.act, (const int32_t *)f.act2, f.n_kept,
                           cand);
        TSC_HIP(hipGetLastError());
        const int64_t at = r->n_kept;
        TSC_TRY(launch_gather_rows(c->stream, f.structs, f.act2, f.n_kept, n * 3, r->sel, r->n_heavy * 3, r->heavy + ep_row_offset(at, r->n_heavy * 3)));
        TSC_TRY(launch_gather_rows(c->stream, f.rot, cand, f.n_kept, n_mols * 9, nullptr, n_mols * 9, r->rot + ep_row_offset(at, n_mols * 9)));
        TSC_TRY(launch_gather_rows(c->stream, f.pos, cand, f.n_kept, n_mols * 3, nullptr, n_mols * 3, r->pos + ep_row_offset(at, n_mols * 3)));
        hipLaunchKernelGGL(k_gather_rows_i32, dim3(grid_for(int64_t(f.n_kept) * n_mols, 256, 1024)), dim3(256), 0, c->stream, f.ci, (const int32_t *)cand,
                           int64_t(f.n_kept), n_mols, r->ci + ep_row_offset(at, n_mols));
        TSC_HIP(hipGetLastError());
    }
    TSC_TRY(h.finish());   // (the kept flags; the slab's pose buffer goes back to the cache with the call)
    r->n_kept += f.n_kept;
    *n_kept = f.n_kept;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_count(tsc_embed_prune *r, int64_t *n_kept_total) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && n_kept_total, "tsc_embed_prune_count: null argument");
    *n_kept_total = r->n_kept;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_run(tsc_embed_prune *r, double rmsd_thr, int mode, uint8_t *survived, tsc_pass_stats *stats,
                                                                          int *n_passes, int64_t *n_survived) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && n_survived && (survived || r->n_kept == 0), "tsc_embed_prune_run: null argument");
    TSC_REQUIRE(mode == 0 || mode == 1, "tsc_embed_prune_run: mode %d (0: reference-exact, 1: cache-free)", mode);
    TSC_REQUIRE(rmsd_thr > 0, "tsc_embed_prune_run: rmsd_thr = %g must be positive", rmsd_thr);
    *n_survived = 0;
    if (n_passes) *n_passes = 0;
    tsc_ctx *c = r->ctx;
    if (r->n_kept == 0) {   // (nothing is launched)
        r->pruned = true, r->n_survived = 0;
        return 0;
    }
    DeviceGuard guard(c->device);
    if (!r->survived) TSC_TRY(r->get(size_t(r->n_kept), &r->survived));
    r->pruned = true, r->n_survived = 0;   // (from here on the set of kept poses is closed, whatever becomes of the prune)
    TSC_TRY(tsc_prune_rmsd_dev(c, r->heavy, r->n_kept, r->n_heavy, rmsd_thr, mode, r->survived, stats, n_passes));
    TSC_HIP(hipMemcpyAsync(survived, r->survived, size_t(r->n_kept), hipMemcpyDeviceToHost, c->stream));
    TSC_HIP(hipStreamSynchronize(c->stream));
    int64_t count = 0;
    for (int64_t i = 0; i < r->n_kept; ++i) count += survived[i] != 0;
    r->n_survived = count;
    *n_survived = count;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_embed_prune_poses(tsc_embed_prune *r, int which, double *poses, int64_t capacity) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(r && poses, "tsc_embed_prune_poses: null argument");
    TSC_REQUIRE(which == 0 || which == 1, "tsc_embed_prune_poses: which = %d (0: the survivors, 1: every kept pose)", which);
    if (which == 0 && !r->pruned) return fail(TSC_ERR_STATE, "tsc_embed_prune_poses: the survivors are known once tsc_embed_prune_run has run");
    const int64_t rows = which == 0 ? r->n_survived : r->n_kept;
    TSC_REQUIRE(capacity >= rows, "tsc_embed_prune_poses: poses holds %lld rows, %lld are asked for", (long long)capacity, (long long)rows);
    if (rows == 0) return 0;
    tsc_ctx *c = r->ctx;
    const int n = r->ft.n_total;
    HostCall h(c);
    Scratch &s = h.scratch();
    int32_t *act = nullptr;
    if (which == 0) {
        int32_t *bsum;
        TSC_TRY(s.get(scan_bsum_count(r->n_kept), &bsum));
        TSC_TRY(s.get(size_t(r->n_kept), &act));
        TSC_TRY(scan_mask(c->stream, r->survived, r->n_kept, bsum, nullptr, act, nullptr, nullptr));
    }
    // the kernel, and the parameters, that embedded these poses for the filter: the same values come out
    double *d_out;
    TSC_TRY(s.get(size_t(rows) * n * 3, &d_out));
    hipLaunchKernelGGL(k_transform, dim3(grid_for(rows, TR_POSES, 256 * 64)), dim3(256), transform_lds_bytes(r->ft.n_mols), c->stream, (const double *)r->frags, r->ft,
                       (const int32_t *)r->ci, (const double *)r->rot, (const double *)r->pos, (const int32_t *)act, rows, d_out, (const int32_t *)nullptr, 0,
                       (double *)nullptr, (const int32_t *)nullptr);
    TSC_HIP(hipGetLastError());
    TSC_TRY(h.fetch(poses, (const double *)d_out, size_t(rows) * n * 3));
    return h.finish();
    TSC_API_GUARD_END
}
