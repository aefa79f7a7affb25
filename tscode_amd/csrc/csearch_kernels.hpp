// csearch_kernels.hpp -- the kernels of the conformational search and of the embeds' pose parameters, thin wrappers of the device
// functions of csearch.hpp.  Included only by adjacent.hip, which launches them.
#pragma once
#include "csearch.hpp"

namespace tsc {

// rotate_dihedral (tscode/utils.py:389-414) for a batch of structures that share torsion and mask: structure s turns its masked atoms by
// angles[s] DEGREES (any real number: tscode/torsion_module.py:984-1005 searches fractional corrections) about its own i2 - i3 bond,
// centre i3; no clash check, no walk-back.  One thread per (structure, atom); out must not alias coords (the axis atoms are read by
// every thread of a structure).
inline __global__ __launch_bounds__(256) void k_rotate_dihedral(const double *__restrict__ coords, int64_t n_structs, int n, int i2, int i3,
                                                          const uint8_t *__restrict__ mask, const double *__restrict__ angles, double *__restrict__ out) {
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < n_structs * n; e += int64_t(gridDim.x) * 256) {
        const int64_t s = e / n;
        const int a = int(e - s * n);
        const double *c = coords + s * n * 3;
        double v[3] = {c[3 * a], c[3 * a + 1], c[3 * a + 2]};
        if (mask[a]) {
            double R[9], cen[3];
            dihedral_rotation(c, i2, i3, angles[s], R, cen);
            const double d0 = v[0] - cen[0], d1 = v[1] - cen[1], d2 = v[2] - cen[2];  // (mat @ (coords[mask] - center).T).T + center, :412
            v[0] = (R[0] * d0 + R[1] * d1 + R[2] * d2) + cen[0];
            v[1] = (R[3] * d0 + R[4] * d1 + R[5] * d2) + cen[1];
            v[2] = (R[6] * d0 + R[7] * d1 + R[8] * d2) + cen[2];
        }
        out[e * 3] = v[0], out[e * 3 + 1] = v[1], out[e * 3 + 2] = v[2];
    }
}

// out [n_cand][n][3], rotated_bonds [n_cand]; angles [n_cand][n_tors] int32 degrees; masks [n_tors][n]; torsions [n_tors][4]
// dynamic LDS: torsion lists, then one csearch_wave_bytes(n) area per wavefront of the block
inline __global__ __launch_bounds__(256) void k_csearch_rotate(CsearchArgs a, const double *__restrict__ base, const int32_t *__restrict__ tors,
                                                         const uint8_t *__restrict__ masks, const int32_t *__restrict__ angles,
                                                         double *__restrict__ out, int32_t *__restrict__ rotated_bonds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, n = a.n, npad = (n + 2) & ~1;
    const TorsionLists L = torsion_lists_at(s_raw, a.n_tors, n);
    build_torsion_lists(L, masks, tors, a.n_tors, n);
    double *c = reinterpret_cast<double *>(s_raw + torsion_lists_bytes(a.n_tors, n) + size_t(wid) * csearch_wave_bytes(n));
    float *F = reinterpret_cast<float *>(c + size_t(n) * 3);
    double *step_rot = reinterpret_cast<double *>(F + size_t(3) * npad);
    for (int64_t m = int64_t(blockIdx.x) * nw + wid; m < a.n_cand; m += int64_t(gridDim.x) * nw)
        csearch_candidate(a, base, tors, a.n_tors, angles + m * a.n_tors, L, c, F, step_rot, out + m * n * 3, rotated_bonds + m, lane);
}

// The same candidates for many start structures and torsion sets in one launch (tscode/torsion_module.py:736-780: the loop over
// starting_points of clustered_csearch; tscode/embedder.py:1907-1939: one random_csearch per TS candidate).  Candidate m is
// (start cand_start[m], row cand_row[m] of the shared angle table, whose rows are t_max wide and zero-padded).  The host cuts the
// candidates into work items (lo, hi, first torsion of the set, torsions of the set) of at most one candidate per wavefront
// that never straddle a torsion set; a workgroup walks items with a grid stride and rebuilds its LDS torsion lists only when the
// set of its next item is not the one it holds.  dynamic LDS: the lists of the widest set, then one area per wavefront.
struct CsearchMultiArgs {
    CsearchArgs a;           // n_tors: unused (each item carries its own); n_cand: the number of work items
    int t_max;               // row stride of angles
    size_t lists_bytes;      // torsion_lists_bytes of the widest set
};

inline __global__ __launch_bounds__(256) void k_csearch_rotate_multi(CsearchMultiArgs ma, const double *__restrict__ starts, const int32_t *__restrict__ tors,
                                                               const uint8_t *__restrict__ masks, const int32_t *__restrict__ angles,
                                                               const int32_t *__restrict__ cand_start, const int32_t *__restrict__ cand_row,
                                                               const int32_t *__restrict__ items, double *__restrict__ out,
                                                               int32_t *__restrict__ rotated_bonds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, n = ma.a.n, npad = (n + 2) & ~1;
    double *c = reinterpret_cast<double *>(s_raw + ma.lists_bytes + size_t(wid) * csearch_wave_bytes(n));
    float *F = reinterpret_cast<float *>(c + size_t(n) * 3);
    double *step_rot = reinterpret_cast<double *>(F + size_t(3) * npad);
    int held_off = -1, held_n = -1;  // the set whose lists are in LDS
    TorsionLists L = torsion_lists_at(s_raw, 0, n);
    for (int64_t it = blockIdx.x; it < ma.a.n_cand; it += gridDim.x) {  // (block-uniform: every wavefront sees the same items)
        const int lo = items[4 * it], hi = items[4 * it + 1], t_off = items[4 * it + 2], n_tors = items[4 * it + 3];
        const int32_t *set_tors = tors + size_t(t_off) * 4;
        if (t_off != held_off || n_tors != held_n) {
            __syncthreads();  // nobody still walks the lists of the previous set
            L = torsion_lists_at(s_raw, n_tors, n);
            build_torsion_lists(L, masks + size_t(t_off) * n, set_tors, n_tors, n);
            held_off = t_off, held_n = n_tors;
        }
        const int64_t m = int64_t(lo) + wid;
        if (m < hi)
            csearch_candidate(ma.a, starts + size_t(cand_start[m]) * n * 3, set_tors, n_tors, angles + size_t(cand_row[m]) * ma.t_max, L, c, F, step_rot,
                              out + m * n * 3, rotated_bonds + m, lane);
    }
}

// One wavefront per segment g = candidates [seg_off[g], seg_off[g + 1]) of start seg_start[g], whose first row has index seg_a0[g]
// in its start's table.  State per start, carried from round to round: kept_count (in / out), done (in / out); rows_consumed (out)
// = rows of this segment the reference's loop would have walked.  seg_kept[g] = rows taken this round.
inline __global__ __launch_bounds__(256) void k_csearch_select(const int32_t *__restrict__ rotated_bonds, const int32_t *__restrict__ seg_off,
                                                         const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_a0, int n_seg, int n_out,
                                                         long long max_tries, int32_t *__restrict__ kept_count, int32_t *__restrict__ done,
                                                         int32_t *__restrict__ rows_consumed, int32_t *__restrict__ seg_kept) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_seg) return;
    const int s = seg_start[g];
    int taken = 0, consumed = 0, stopped = 0;
    if (!done[s]) taken = csearch_select_segment(rotated_bonds, seg_off[g], seg_off[g + 1], seg_a0[g], kept_count[s], n_out, max_tries, lane, &consumed, &stopped);
    if (lane == 0) {
        kept_count[s] += taken, rows_consumed[s] = consumed, seg_kept[g] = taken;
        if (stopped) done[s] = 1;
    }
}

// The rows k_csearch_select took, compacted in order into the output: segment g's slice begins at the sum of seg_kept over the
// segments before it and holds the first seg_kept[g] rows of the segment with rotated_bonds != 0 (the rows taken are a prefix of
// the rows kept).  One wavefront per segment; rows past `capacity` are not written; total[0] = rows taken by all segments.
inline __global__ __launch_bounds__(256) void k_csearch_compact(const double *__restrict__ cand, const int32_t *__restrict__ rotated_bonds,
                                                          const int32_t *__restrict__ seg_off, const int32_t *__restrict__ seg_kept, int n_seg,
                                                          int row_doubles, long long capacity, double *__restrict__ kept_rows,
                                                          int32_t *__restrict__ total) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_seg) return;
    long long off = 0;
    for (int h = lane; h < g; h += 64) off += seg_kept[h];
    for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d);
    const int want = seg_kept[g], lo = seg_off[g], hi = seg_off[g + 1];
    if (g == n_seg - 1 && lane == 0) total[0] = int32_t(off + want);
    int taken = 0;
    for (int b = lo; b < hi && taken < want; b += 64) {
        const int m = b + lane;
        const unsigned long long bk = __ballot(m < hi && rotated_bonds[m] != 0);
        for (unsigned long long rest = bk; rest && taken < want; rest &= rest - 1, ++taken) {
            const int j = __ffsll((long long)rest) - 1;
            const long long dst = off + taken;
            if (dst >= capacity) continue;
            const double *src = cand + size_t(b + j) * row_doubles;
            double *o = kept_rows + size_t(dst) * row_doubles;
            for (int e = lane; e < row_doubles; e += 64) o[e] = src[e];
        }
    }
}

// torsion_comp_check for a batch of structures sharing torsion and mask: ok[s] = 1 / 0
inline __global__ __launch_bounds__(256) void k_torsion_comp_check(CsearchArgs a, const double *__restrict__ coords, const int32_t *__restrict__ tors,
                                                             const uint8_t *__restrict__ mask, int32_t *__restrict__ ok) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, n = a.n, npad = (n + 2) & ~1;
    const TorsionLists L = torsion_lists_at(s_raw, 1, n);
    build_torsion_lists(L, mask, tors, 1, n);
    double *c = reinterpret_cast<double *>(s_raw + torsion_lists_bytes(1, n) + size_t(wid) * csearch_wave_bytes(n));
    float *F = reinterpret_cast<float *>(c + size_t(n) * 3);
    const int nm = L.count[0], nf = L.count[1];
    for (int64_t m = int64_t(blockIdx.x) * nw + wid; m < a.n_cand; m += int64_t(gridDim.x) * nw) {
        const double *src = coords + m * n * 3;
        for (int e = lane; e < n * 3; e += 64) c[e] = src[e];
        __builtin_amdgcn_wave_barrier();
        const double cmax_fixed = a.max_clashes == 0 ? stage_fixed_f32(c, L.fixed, nf, F, npad, lane) : 0.0;
        const int r = torsion_comp_check_lds(c, L.moved, nm, L.fixed, nf, F, npad, cmax_fixed, a.sq_bound, a.max_clashes, lane);
        if (lane == 0) ok[m] = r;
        __builtin_amdgcn_wave_barrier();
    }
}

inline __global__ __launch_bounds__(256) void k_string_embed_params(const double *__restrict__ p1, const double *__restrict__ p2,
                                                              const double *__restrict__ ref_vec, const double *__restrict__ mol_vec,
                                                              const int32_t *__restrict__ conf_pair, int64_t n_sites,
                                                              const double *__restrict__ angles, int n_angles, double *__restrict__ rot,
                                                              double *__restrict__ pos, int32_t *__restrict__ conf_idx) {
    const int64_t total = n_sites * n_angles;
    for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < total; q += int64_t(gridDim.x) * blockDim.x) {
        const int64_t s = q / n_angles;
        const double angle = angles[q - s * n_angles];
        const double rv[3] = {ref_vec[3 * s], ref_vec[3 * s + 1], ref_vec[3 * s + 2]};
        const double neg[3] = {-rv[0], -rv[1], -rv[2]};
        const double mv[3] = {mol_vec[3 * s], mol_vec[3 * s + 1], mol_vec[3 * s + 2]};
        double R0[9], R[9];
        rotation_matrix_from_vectors_dev(mv, neg, R0);
        if (angle != 0) {
            double dR[9];
            rot_mat_from_pointer_dev(rv, angle, dR);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) R[3 * i + j] = dR[3 * i] * R0[j] + dR[3 * i + 1] * R0[3 + j] + dR[3 * i + 2] * R0[6 + j];
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = R0[i];
        }
        double *ro = rot + q * 18, *po = pos + q * 6;
#pragma unroll
        for (int i = 0; i < 9; ++i) ro[i] = (i % 4 == 0) ? 1.0 : 0.0, ro[9 + i] = R[i];
        const double x = p2[3 * s], y = p2[3 * s + 1], z = p2[3 * s + 2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            po[i] = 0.0;
            po[3 + i] = p1[3 * s + i] - (R[3 * i] * x + R[3 * i + 1] * y + R[3 * i + 2] * z);
        }
        conf_idx[2 * q] = conf_pair[2 * s], conf_idx[2 * q + 1] = conf_pair[2 * s + 1];
    }
}

inline __global__ __launch_bounds__(256) void k_cyclical_embed_params(const double *__restrict__ start, const double *__restrict__ end,
                                                                const double *__restrict__ direction, const double *__restrict__ pivot,
                                                                const double *__restrict__ meanpoint, const double *__restrict__ r0,
                                                                const double *__restrict__ r1, const int32_t *__restrict__ n_reactive,
                                                                const double *__restrict__ angle, int64_t n, double *__restrict__ rot,
                                                                double *__restrict__ pos) {
    for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += int64_t(gridDim.x) * blockDim.x) {
        CyclicalAlign g;
        cyclical_align_dev(start + 3 * q, end + 3 * q, direction + 3 * q, pivot + 3 * q, meanpoint + 3 * q, r0 + 3 * q, r1 + 3 * q, n_reactive[q] == 2, g);
        cyclical_step_dev(g, angle[q], rot + 9 * q, pos + 3 * q);
    }
}

// The same rows from one record per (group, molecule) and one angle table for all groups (tsc_cyclical_embed_groups): pose g * A + a takes
// record g and angle set a.  A wavefront takes a chunk of whole groups, 64 / n_mols of them, in two phases:
//   1. one (group, molecule) record per lane: cyclical_align_dev -- the Jacobi sweep of align_vec_pair_dev -- once per record, all lanes
//      busy, its 18 doubles parked in LDS (record-minor, so the 64 lanes write 64 consecutive doubles);
//   2. the chunk's rows, which lie back to back in rot / pos, strided over the lanes: a lane fetches its row's record from LDS (neighbouring
//      lanes mostly share one: a broadcast) and does the angle's half, cyclical_step_dev; consecutive lanes write consecutive rows.
// So the sweep runs once per 64 records where the row kernel runs it once per 64 rows, and no lane idles while a group has fewer than 64
// angle sets.  (One wavefront per record with the sweep in front of its angle loop was tried first: on 36 angle sets it keeps 36 of 64
// lanes busy and took 1.8 times the row kernel's time -- lanes in lockstep make "once per wavefront" no cheaper than "once per 64 rows".)
// The four wavefronts of a block walk their chunks in step, so the barriers between the phases are block barriers.  Also writes the rows'
// conformer indices, which the embed reads per (pose, molecule).
constexpr int CGP_WAVES = 4;

inline __global__ __launch_bounds__(64 * CGP_WAVES) void k_cyclical_embed_group_params(
    const double *__restrict__ start, const double *__restrict__ end, const double *__restrict__ direction, const double *__restrict__ pivot,
    const double *__restrict__ meanpoint, const double *__restrict__ r0, const double *__restrict__ r1, const int32_t *__restrict__ n_reactive,
    const int32_t *__restrict__ conf_idx, const double *__restrict__ angles, int64_t n_groups, int n_mols, int n_angles, double *__restrict__ rot,
    double *__restrict__ pos, int32_t *__restrict__ conf_rows) {
    __shared__ double s_align[CGP_WAVES][18][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int per_chunk = 64 / n_mols;  // groups per wavefront and pass
    const int64_t n_chunks = (n_groups + per_chunk - 1) / per_chunk;
    double(*sa)[64] = s_align[wid];
    for (int64_t c0 = int64_t(blockIdx.x) * CGP_WAVES; c0 < n_chunks; c0 += int64_t(gridDim.x) * CGP_WAVES) {
        const int64_t g0 = (c0 + wid) * per_chunk;  // (a wavefront past the last chunk has nothing to do in either phase)
        const int groups_here = g0 < n_groups ? int(n_groups - g0 < per_chunk ? n_groups - g0 : per_chunk) : 0;
        const int items_here = groups_here * n_mols;
        if (lane < items_here) {
            const int64_t w = g0 * n_mols + lane;
            CyclicalAlign g;
            cyclical_align_dev(start + 3 * w, end + 3 * w, direction + 3 * w, pivot + 3 * w, meanpoint + 3 * w, r0 + 3 * w, r1 + 3 * w, n_reactive[w] == 2, g);
#pragma unroll
            for (int k = 0; k < 9; ++k) sa[k][lane] = g.A[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) sa[9 + k][lane] = g.axis[k], sa[12 + k][lane] = g.centre[k], sa[15 + k][lane] = g.shift[k];
        }
        __syncthreads();
        const int rows_here = items_here * n_angles;  // <= 64 * GF_MAX_GROUP
        const int64_t row0 = g0 * n_angles * n_mols;
        for (int r = lane; r < rows_here; r += 64) {
            const int t = r / n_mols, m = r - t * n_mols;  // row = (group * n_angles + a) * n_mols + m
            const int gl = t / n_angles, a = t - gl * n_angles;
            const int item = gl * n_mols + m;
            CyclicalAlign g;
#pragma unroll
            for (int k = 0; k < 9; ++k) g.A[k] = sa[k][item];
#pragma unroll
            for (int k = 0; k < 3; ++k) g.axis[k] = sa[9 + k][item], g.centre[k] = sa[12 + k][item], g.shift[k] = sa[15 + k][item];
            const int64_t row = row0 + r;
            cyclical_step_dev(g, angles[a * n_mols + m], rot + 9 * row, pos + 3 * row);
            conf_rows[row] = conf_idx[g0 * n_mols + item];
        }
        __syncthreads();
    }
}

}  // namespace tsc
