// diverse_batch.hpp -- alignment, k-means and the diverse-conformer pick (diverse.hpp) for many small ensembles per launch.
//
// A batch is S segments, each an ensemble of its own with its own N, n_atoms and k.  Every kernel here is the segmented form of a
// kernel of diverse.hpp: a workgroup reads its work item (segment, place in the segment's own grid) from a table the host built from the
// segments' sizes, forms the segment's pointers and calls the dv_* function the single-ensemble kernel calls.  A segment's decomposition
// -- the chunks of the column statistics, the 64-row tiles and centre blocks of the assignment, the 64-column slices of the update, the
// pieces of the 1024-thread sums -- depends on its own N, D and k only, so its results are those of tsc_diverse_select on it alone, bit
// for bit.  There are no empty workgroups of a "largest segment x S" grid: a table holds exactly the workgroups its segments need.
//
// The Lloyd loop's control is on the device, per segment (DvState): k_kmeans_control_seg applies lloyd_run's rule -- labels repeated, or
// shift <= the segment's own tolerance, or max_iter -- and the workgroups of a finished segment return at once.  Nothing waits on
// anything another workgroup writes inside a launch; the host reads one DvSummary per iteration and stops when no segment is live.
#pragma once
#include "diverse.hpp"
#include "diverse_align_kernel.hpp"

namespace tsc {

struct DvSegment {
    int64_t x0;     // first double of the segment in structures / aligned / X
    int64_t row0;   // first row in the arrays with an entry per structure
    int64_t c0;     // first double of its centres
    int64_t part0;  // first double of its column partials
    int32_t N, n, D, k;
    int32_t k0;     // first entry in the arrays with an entry per cluster (offs: k0 + segment index)
    int32_t d0;     // first entry in the arrays with an entry per column
    int32_t sp0;    // first entry of its shift partials
    int32_t chunks, slices, has_energies, seeded, pad;
    double inv_N, inv_D;   // 1 / N and 1 / D as the single call's host code forms them
};
struct DvItem {
    int32_t seg, bx, by, pad;
};
struct DvState {
    int32_t live;         // the Lloyd loop of the segment goes on
    int32_t need_final;   // it ended otherwise than by repeated labels: one more assignment and bucket
    int32_t it, n_iter;
    double tol_abs;
};
struct DvSummary {
    int32_t live, need_final;
};
// which segments a launch of the Lloyd loop serves
enum DvGate : int { DV_ALL = 0, DV_LIVE = 1, DV_FINAL = 2 };
__device__ inline bool dv_gate_open(const DvState *__restrict__ st, int seg, int gate) {
    return gate == DV_ALL || (gate == DV_LIVE ? st[seg].live != 0 : st[seg].need_final != 0);
}

// device arrays of a batch (every block belongs to the call's Scratch)
struct DvBatch {
    const DvSegment *segs;
    DvState *state;
    const double *in;
    double *al, *X, *C, *xn, *cn, *own_d2, *shift_part, *mean, *var, *mv, *part, *min_d2;
    const double *u, *energies;
    int32_t *labels, *counts, *offs, *members, *rows, *picked;
    int *changed;
    KmControl *ctl;
};

inline __global__ __launch_bounds__(256) void k_align_structures_seg(DvBatch b, const DvItem *__restrict__ items) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    dv_align_structures(b.in + g.x0, g.N, g.n, nullptr, g.n, b.al + g.x0, it.bx);
}

// squares: 0 = the means of X, 1 = the variances of the centred X (both scaled by 1 / N)
inline __global__ __launch_bounds__(256) void k_col_partial_seg(DvBatch b, const DvItem *__restrict__ items, int squares) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    dv_col_partial(b.X + g.x0, g.N, g.D, squares, b.part + g.part0, it.bx, it.by, g.chunks);
}
inline __global__ __launch_bounds__(256) void k_col_finish_seg(DvBatch b, const DvItem *__restrict__ items, int squares) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    dv_col_finish(b.part + g.part0, g.chunks, g.D, g.inv_N, (squares ? b.var : b.mean) + g.d0, it.bx);
}
// X[i, d] -= mean[d]: a wavefront per row (one subtraction per element, whatever the decomposition)
inline __global__ __launch_bounds__(256) void k_centre_rows_seg(DvBatch b, const DvItem *__restrict__ items) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    const int lane = threadIdx.x & 63;
    const int64_t r = int64_t(it.bx) * 4 + (threadIdx.x >> 6);
    if (r >= g.N) return;
    double *x = b.X + g.x0 + r * g.D;
    const double *v = b.mean + g.d0;
    for (int d = lane; d < g.D; d += 64) x[d] += -1.0 * v[d];
}
// mv[s] = mean(var): one workgroup of 1024 per segment
inline __global__ __launch_bounds__(1024) void k_mean_var_seg(DvBatch b) {
    const DvSegment g = b.segs[blockIdx.x];
    dv_sum_fixed(b.var + g.d0, int64_t(g.D), g.inv_D, b.mv + blockIdx.x);
}
// C[c] = X[rows[c]]: a wavefront per centre
inline __global__ __launch_bounds__(256) void k_gather_rows_seg(DvBatch b, const DvItem *__restrict__ items) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    const int lane = threadIdx.x & 63;
    const int c = it.bx * 4 + (threadIdx.x >> 6);
    if (c >= g.k) return;
    const double *x = b.X + g.x0 + int64_t(b.rows[g.k0 + c]) * g.D;
    double *o = b.C + g.c0 + int64_t(c) * g.D;
    for (int d = lane; d < g.D; d += 64) o[d] = x[d];
}

// centres != 0: the norms of the centres (gated), else of the rows
inline __global__ __launch_bounds__(256) void k_row_norms_seg(DvBatch b, const DvItem *__restrict__ items, int centres, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    if (centres)
        dv_row_norms(b.C + g.c0, int64_t(g.k), g.D, b.cn + g.k0, it.bx);
    else
        dv_row_norms(b.X + g.x0, g.N, g.D, b.xn + g.row0, it.bx);
}

// the segments of one template width (call.hpp: with_width), as lloyd's assign() chooses it from k
template <int NT>
__global__ __launch_bounds__(256) void k_kmeans_assign_seg(DvBatch b, const DvItem *__restrict__ items, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    dv_kmeans_assign<NT>(b.X + g.x0, g.N, g.D, b.C + g.c0, g.k, b.xn + g.row0, b.cn + g.k0, b.labels + g.row0, b.own_d2 + g.row0, b.changed + it.seg, it.bx);
}

inline __global__ __launch_bounds__(256) void k_label_count_seg(DvBatch b, const DvItem *__restrict__ items, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    dv_label_count(b.labels + g.row0, g.N, b.counts + g.k0, it.bx);
}
inline __global__ __launch_bounds__(256) void k_label_bucket_seg(DvBatch b, const DvItem *__restrict__ items, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    dv_label_bucket(b.labels + g.row0, g.N, b.counts + g.k0, g.k, b.offs + g.k0 + it.seg, b.members + g.row0, it.bx);
}
inline __global__ __launch_bounds__(256) void k_own_d2_seg(DvBatch b, const DvItem *__restrict__ items, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    dv_own_d2(b.X + g.x0, g.N, g.D, b.C + g.c0, b.labels + g.row0, b.counts + g.k0, g.k, 1, b.own_d2 + g.row0, it.bx);
}
// one workgroup per segment
inline __global__ __launch_bounds__(256) void k_kmeans_relocate_seg(DvBatch b, int gate) {
    const int seg = blockIdx.x;
    if (!dv_gate_open(b.state, seg, gate)) return;
    const DvSegment g = b.segs[seg];
    dv_kmeans_relocate(b.own_d2 + g.row0, g.N, b.labels + g.row0, b.counts + g.k0, g.k, b.ctl + seg);
}
inline __global__ __launch_bounds__(256) void k_kmeans_update_seg(DvBatch b, const DvItem *__restrict__ items, int gate) {
    const DvItem it = items[blockIdx.x];
    if (!dv_gate_open(b.state, it.seg, gate)) return;
    const DvSegment g = b.segs[it.seg];
    dv_kmeans_update(b.X + g.x0, g.D, b.members + g.row0, b.offs + g.k0 + it.seg, b.counts + g.k0, b.ctl + it.seg, b.C + g.c0, b.shift_part + g.sp0, it.bx,
                     it.by, g.slices);
}
// One wavefront per segment: the iteration's shift in the single call's order, then lloyd_run's rule on the segment's own state.  A live
// segment adds itself to the summary the host reads (zeroed by the host in front of the launch; integer atomics only).
inline __global__ __launch_bounds__(64) void k_kmeans_control_seg(DvBatch b, int max_iter, double tol, DvSummary *__restrict__ summary) {
    const int seg = blockIdx.x;
    DvState *st = b.state + seg;
    if (!st->live) {
        if (threadIdx.x == 0 && st->need_final) atomicAdd(&summary->need_final, 1);
        return;
    }
    const DvSegment g = b.segs[seg];
    KmControl *ctl = b.ctl + seg;
    dv_kmeans_control(b.shift_part + g.sp0, g.k * g.slices, b.changed + seg, ctl);
    if (threadIdx.x != 0) return;
    const int it = st->it + 1;
    const double tol_abs = b.mv[seg] * tol;   // mean(var(X, axis = 0)) * tol, scikit-learn's _tolerance
    int live = 1, need_final = 0;
    if (ctl->changed == 0)                    // labels == labels of the iteration before: strict convergence
        live = 0;
    else if (ctl->shift <= tol_abs || it >= max_iter)
        live = 0, need_final = 1;
    st->it = it, st->tol_abs = tol_abs, st->live = live, st->need_final = need_final;
    if (!live) st->n_iter = it;
    if (live) atomicAdd(&summary->live, 1);
    if (need_final) atomicAdd(&summary->need_final, 1);
}

inline __global__ __launch_bounds__(256) void k_diverse_pick_seg(DvBatch b, const DvItem *__restrict__ items) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    // the pick sees differences centre - member only: the centred features and centres serve as they are
    dv_diverse_pick(b.X + g.x0, g.n, b.members + g.row0, b.offs + g.k0 + it.seg, b.counts + g.k0, b.C + g.c0, g.k,
                    g.has_energies ? b.energies + g.row0 : nullptr, b.picked + g.k0, it.bx);
}

// k-means++ for the seeded segments with k > j, which the host lists first (seeded segments in order of decreasing k): the launch of
// index j covers a prefix of the tables.  Seeds are chosen on the ALIGNED features, as in tsc_diverse_select.
inline __global__ __launch_bounds__(256) void k_kmeans_seed_update_seg(DvBatch b, const DvItem *__restrict__ items, int j) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    dv_kmeans_seed_update(b.al + g.x0, g.N, g.D, b.rows + g.k0, j, b.min_d2 + g.row0, it.bx);
}
inline __global__ __launch_bounds__(1024) void k_kmeans_seed_pick_seg(DvBatch b, const DvItem *__restrict__ items, int j) {
    const DvItem it = items[blockIdx.x];
    const DvSegment g = b.segs[it.seg];
    dv_kmeans_seed_pick(b.min_d2 + g.row0, g.N, b.u + g.k0, j, b.rows + g.k0);
}

}  // namespace tsc
