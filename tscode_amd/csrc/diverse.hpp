// diverse.hpp -- the end of a conformational search on the device: Kabsch alignment of an ensemble onto its first structure
// (tscode/hypermolecule_class.py:38-72, align_structures), Lloyd's k-means on the flattened aligned coordinates and one pick per
// cluster (tscode/torsion_module.py:849-924, most_diverse_conformers, which calls scikit-learn's KMeans at :889-890).
//
// All arithmetic is fp64 and every sum is taken in a fixed order (butterfly reductions, rows bucketed by label and added in row
// order): no floating-point atomics, so two calls on the same input return the same bits.  The only atomics are integer counts.
//
//   k_align_structures    one wavefront per structure: centroids over the index set, S = tgt^T ref, Horn's quaternion by the exact
//                         path of pair_math.hpp (exact_quaternion: Newton + adjugate, Jacobi fallback), all atoms rotated.
//   k_kmeans_assign       the hot path: labels[i] = argmin_c |x_i|^2 - 2 x_i.c + |c|^2.  A workgroup owns 64 rows (16 per wavefront) and
//                         walks D in slices of 32 through LDS, against a block of 16 NT centres; the products x.c run on the matrix
//                         cores (v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]; result register r of lane l
//                         is row (l >> 4) + 4 r, column l & 15).
//   k_label_bucket        rows sorted by label, row order kept inside a label (one workgroup per cluster).
//   k_kmeans_update       one workgroup per (cluster, 64 columns of D): the members' sum in bucket order, the relocation of empty
//                         clusters (scikit-learn's _relocate_empty_clusters_dense), the new centre and its squared shift.
//   k_diverse_pick        one workgroup per cluster: the member to keep (torsion_module.py:894-922).
//   k_kmeans_seed_update / k_kmeans_seed_pick   k-means++ without local trials, the uniforms given by the caller.
//
// Every kernel's body is a __device__ function (dv_*) of the problem's own pointers and sizes and of the workgroup's place in the
// problem's own grid; the __global__ kernel (diverse_kernels.hpp; none here) is its one-line wrapper.  The kernels of diverse_batch.hpp, which serve many ensembles
// per launch, look up (segment, local workgroup) and call the same function: a segment's sums are taken in the order the single call
// takes them, and its results are the single call's bit for bit.
#pragma once
#include "common.hpp"
#include "pair_math.hpp"

namespace tsc {

constexpr int DV_MAX_ATOMS = 512;  // as rot_corr.hpp: RC_MAX_ATOMS
constexpr int DV_MAX_K = 300;      // the reference's own gate (torsion_module.py:863)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// sum over the wavefront, the same bits in every lane (a + b == b + a)
__device__ inline double dv_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---------------------------------------------------------------------------------------------------
// align_structures (hypermolecule_class.py:46-72)

__device__ inline void dv_centroid(const double *__restrict__ s, const int32_t *__restrict__ idx, int n_idx, int lane, double c[3]) {
    double x = 0.0, y = 0.0, z = 0.0;
    for (int q = lane; q < n_idx; q += 64) {
        const int a = idx ? idx[q] : q;
        x += s[3 * a], y += s[3 * a + 1], z += s[3 * a + 2];
    }
    c[0] = dv_wave_sum(x) / double(n_idx), c[1] = dv_wave_sum(y) / double(n_idx), c[2] = dv_wave_sum(z) / double(n_idx);
}

// idx == null: every atom (n_idx == n).  Structure 0 is only centred (:53, :58); structure t >= 1 is centred on the mean of its indexed
// atoms (:55) and turned by the proper rotation that takes its indexed atoms onto the reference's (:63, :70).
__device__ inline void dv_align_structures(const double *__restrict__ in, int64_t N, int n, const int32_t *__restrict__ idx, int n_idx,
                                           double *__restrict__ out, int64_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t t = block * 4 + (threadIdx.x >> 6);
    if (t >= N) return;
    const double *ref = in, *tgt = in + t * n * 3;
    double *o = out + t * n * 3;
    double cr[3], ct[3];
    dv_centroid(ref, idx, n_idx, lane, cr);
    if (t == 0) {
        for (int a = lane; a < n; a += 64) o[3 * a] = ref[3 * a] - cr[0], o[3 * a + 1] = ref[3 * a + 1] - cr[1], o[3 * a + 2] = ref[3 * a + 2] - cr[2];
        return;
    }
    dv_centroid(tgt, idx, n_idx, lane, ct);
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Gp = 0.0, Gq = 0.0;   // p = target, q = reference: S = p^T q (pair_math.hpp)
    for (int q = lane; q < n_idx; q += 64) {
        const int a = idx ? idx[q] : q;
        const double px = tgt[3 * a] - ct[0], py = tgt[3 * a + 1] - ct[1], pz = tgt[3 * a + 2] - ct[2];
        const double qx = ref[3 * a] - cr[0], qy = ref[3 * a + 1] - cr[1], qz = ref[3 * a + 2] - cr[2];
        S[0] += px * qx, S[1] += px * qy, S[2] += px * qz;
        S[3] += py * qx, S[4] += py * qy, S[5] += py * qz;
        S[6] += pz * qx, S[7] += pz * qy, S[8] += pz * qz;
        Gp += px * px + py * py + pz * pz;
        Gq += qx * qx + qy * qy + qz * qz;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = dv_wave_sum(S[i]);
    Gp = dv_wave_sum(Gp), Gq = dv_wave_sum(Gq);
    double e[4];
    exact_quaternion(S, Gp, Gq, e);   // (every lane, on the same bits)
    double nn = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
    if (!(nn > 0.0) || !(nn < 1e300)) e[0] = 1.0, e[1] = e[2] = e[3] = 0.0, nn = 1.0;   // (no optimum to speak of: identity, finite and proper)
    nn = 1.0 / sqrt(nn);
    const double w = e[0] * nn, x = e[1] * nn, y = e[2] * nn, z = e[3] * nn;
    const double R00 = w * w + x * x - y * y - z * z, R01 = 2 * (x * y - w * z), R02 = 2 * (x * z + w * y);
    const double R10 = 2 * (x * y + w * z), R11 = w * w - x * x + y * y - z * z, R12 = 2 * (y * z - w * x);
    const double R20 = 2 * (x * z - w * y), R21 = 2 * (y * z + w * x), R22 = w * w - x * x - y * y + z * z;
    for (int a = lane; a < n; a += 64) {
        const double px = tgt[3 * a] - ct[0], py = tgt[3 * a + 1] - ct[1], pz = tgt[3 * a + 2] - ct[2];
        o[3 * a] = R00 * px + R01 * py + R02 * pz;
        o[3 * a + 1] = R10 * px + R11 * py + R12 * pz;
        o[3 * a + 2] = R20 * px + R21 * py + R22 * pz;
    }
}

// ---------------------------------------------------------------------------------------------------
// column statistics of X[N, D] in a fixed order: grid (ceil(D / 64), chunks), 256 threads = 64 columns x 4 row lanes

// (workgroup (bx, by) of a grid (ceil(D / 64), chunks))
__device__ inline void dv_col_partial(const double *__restrict__ X, int64_t N, int D, int squares, double *__restrict__ part, int bx, int by, int chunks) {
    __shared__ double s[4][64];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6, d = bx * 64 + col;
    const int64_t per = ceil_div<int64_t>(N, chunks), lo = per * by, hi = lo + per < N ? lo + per : N;
    double acc = 0.0;
    if (d < D)
        for (int64_t i = lo + g; i < hi; i += 4) {
            const double v = X[i * D + d];
            acc += squares ? v * v : v;
        }
    s[g][col] = acc;
    __syncthreads();
    if (g == 0 && d < D) part[size_t(by) * D + d] = ((s[0][col] + s[1][col]) + s[2][col]) + s[3][col];
}
// out[d] = scale * sum over the chunks, in chunk order
__device__ inline void dv_col_finish(const double *__restrict__ part, int chunks, int D, double scale, double *__restrict__ out, int block) {
    const int d = block * 256 + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int q = 0; q < chunks; ++q) acc += part[size_t(q) * D + d];
    out[d] = acc * scale;
}
// out[0] = scale * sum v[0 .. n) in a fixed order: one workgroup of 1024, a contiguous piece per thread, then a tree
__device__ inline void dv_sum_fixed(const double *__restrict__ v, int64_t n, double scale, double *__restrict__ out) {
    __shared__ double s[1024];
    const int64_t per = ceil_div<int64_t>(n, 1024), lo = per * threadIdx.x, hi = lo + per < n ? lo + per : n;
    double acc = 0.0;
    for (int64_t i = lo; i < hi; ++i) acc += v[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (int(threadIdx.x) < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0] * scale;
}
// out[r] = |X[r]|^2, one wavefront per row
__device__ inline void dv_row_norms(const double *__restrict__ X, int64_t rows, int D, double *__restrict__ out, int64_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t r = block * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = X[r * D + d];
        acc += v * v;
    }
    acc = dv_wave_sum(acc);
    if (lane == 0) out[r] = acc;
}

// ---------------------------------------------------------------------------------------------------
// the assignment step

constexpr int KA_ROWS = 64, KA_DS = 32, KA_LD = KA_DS + 4;   // (row stride 36 doubles: the 16 rows x 4 columns a wavefront reads fall on 64 distinct 8-byte slots)

template <int NT>
__device__ inline void dv_kmeans_assign(const double *__restrict__ X, int64_t N, int D, const double *__restrict__ C, int k,
                                        const double *__restrict__ xn, const double *__restrict__ cn, int32_t *__restrict__ labels,
                                        double *__restrict__ own_d2, int *__restrict__ changed, int64_t block) {
    __shared__ double sX[KA_ROWS * KA_LD];
    __shared__ double sC[NT * 16 * KA_LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, rc = lane & 15, g = lane >> 4;
    const int64_t row0 = block * KA_ROWS;
    double bd[4];
    int bc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bd[r] = INFINITY, bc[r] = 0;
    for (int c0 = 0; c0 < k; c0 += NT * 16) {
        f64x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < D; d0 += KA_DS) {
            __syncthreads();
            for (int e = threadIdx.x; e < KA_ROWS * KA_DS; e += 256) {
                const int r = e / KA_DS, d = e % KA_DS;
                const int64_t i = row0 + r;
                sX[r * KA_LD + d] = (i < N && d0 + d < D) ? X[i * D + d0 + d] : 0.0;
            }
            for (int e = threadIdx.x; e < NT * 16 * KA_DS; e += 256) {
                const int r = e / KA_DS, d = e % KA_DS, c = c0 + r;
                sC[r * KA_LD + d] = (c < k && d0 + d < D) ? C[int64_t(c) * D + d0 + d] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < KA_DS / 4; ++s) {
                const double a = sX[(wid * 16 + rc) * KA_LD + 4 * s + g];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sC[(t * 16 + rc) * KA_LD + 4 * s + g], acc[t], 0, 0, 0);
            }
        }
        // result register r of this lane: row g + 4 r of the wavefront's 16, centre c0 + 16 t + rc.  Centres ascend with t: strict < keeps the lowest
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = row0 + wid * 16 + g + 4 * r;
            const double xr = i < N ? xn[i] : 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = c0 + 16 * t + rc;
                const double d2 = c < k ? (xr - 2.0 * acc[t][r]) + cn[c] : INFINITY;
                if (d2 < bd[r]) bd[r] = d2, bc[r] = c;
            }
        }
    }
    int diff = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {   // the 16 lanes of a row: smallest distance, the lowest centre on a tie
            const double od = __shfl_xor(bd[r], off);
            const int oc = __shfl_xor(bc[r], off);
            if (od < bd[r] || (od == bd[r] && oc < bc[r])) bd[r] = od, bc[r] = oc;
        }
        const int64_t i = row0 + wid * 16 + g + 4 * r;
        if (rc == 0 && i < N) {
            diff += labels[i] != bc[r];
            labels[i] = bc[r];
            own_d2[i] = bd[r] > 0.0 ? bd[r] : 0.0;
        }
    }
    if (diff) atomicAdd(changed, diff);
}

// own_d2[i] = |x_i - C[labels[i]]|^2 by direct differences, one wavefront per row.  only_if_empty: nothing to do unless a cluster is
// empty (the relocation is what needs the exact values; the assignment's come from the expanded form)
__device__ inline bool dv_any_empty(const int32_t *__restrict__ counts, int k, int lane) {
    bool any = false;
    for (int c = lane; c < k; c += 64) any |= counts[c] == 0;
    return __ballot(any) != 0;
}
__device__ inline void dv_own_d2(const double *__restrict__ X, int64_t N, int D, const double *__restrict__ C, const int32_t *__restrict__ labels,
                                 const int32_t *__restrict__ counts, int k, int only_if_empty, double *__restrict__ own_d2, int64_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t i = block * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    if (only_if_empty && !dv_any_empty(counts, k, lane)) return;
    const double *c = C + int64_t(labels[i]) * D;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = X[i * D + d] - c[d];
        acc += v * v;
    }
    acc = dv_wave_sum(acc);
    if (lane == 0) own_d2[i] = acc;
}

// ---------------------------------------------------------------------------------------------------
// rows by label

__device__ inline int dv_block_sum_int(int v, int *s) {   // 256 threads; every thread gets the total
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if (lane == 0) s[wid] = v;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}
__device__ inline void dv_label_count(const int32_t *__restrict__ labels, int64_t N, int32_t *__restrict__ counts, int c) {
    __shared__ int s[4];
    int mine = 0;
    for (int64_t i = threadIdx.x; i < N; i += 256) mine += labels[i] == c;
    const int total = dv_block_sum_int(mine, s);
    if (threadIdx.x == 0) counts[c] = total;
}
// members[offs[c] .. offs[c] + counts[c]) = the rows of cluster c, ascending
__device__ inline void dv_label_bucket(const int32_t *__restrict__ labels, int64_t N, const int32_t *__restrict__ counts, int k, int32_t *__restrict__ offs,
                                       int32_t *__restrict__ members, int c) {
    __shared__ int s[4];
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int before = 0;
    for (int q = threadIdx.x; q < c; q += 256) before += counts[q];
    int base = dv_block_sum_int(before, s);
    if (threadIdx.x == 0) {
        offs[c] = base;
        if (c == k - 1) offs[k] = int(N);
    }
    for (int64_t i0 = 0; i0 < N; i0 += 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool is = i < N && labels[i] == c;
        const unsigned long long b = __ballot(is);
        __syncthreads();
        if (lane == 0) s_wave[wid] = __popcll(b);
        __syncthreads();
        int pre = 0;
        for (int q = 0; q < wid; ++q) pre += s_wave[q];
        if (is) members[base + pre + __popcll(b & ((1ull << lane) - 1ull))] = int32_t(i);
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
}

// ---------------------------------------------------------------------------------------------------
// the update step

// what the host reads back once per iteration, and the relocation table of the iteration (scikit-learn's
// _relocate_empty_clusters_dense: the j-th empty cluster, ascending, takes the row with the j-th largest distance to its own centre
// -- ties: the lower row -- and that row leaves the sum and the count of the cluster it is labelled with)
struct KmControl {
    int changed, n_empty;
    double shift;
    int n_rel, pad;
    int rel_e[DV_MAX_K], rel_f[DV_MAX_K], rel_from[DV_MAX_K];
};

__device__ inline void dv_kmeans_relocate(const double *__restrict__ own_d2, int64_t N, const int32_t *__restrict__ labels,
                                          const int32_t *__restrict__ counts, int k, KmControl *__restrict__ ctl) {
    __shared__ int s_empty[DV_MAX_K], s_chosen[DV_MAX_K], s_n;
    __shared__ double s_d[256];
    __shared__ int s_i[256];
    if (threadIdx.x == 0) {
        int n = 0;
        for (int c = 0; c < k; ++c)
            if (counts[c] == 0) s_empty[n++] = c;
        s_n = n;
        ctl->n_empty = n;
        ctl->n_rel = n < N ? n : int(N);
    }
    __syncthreads();
    const int n_rel = s_n < N ? s_n : int(N);
    for (int j = 0; j < n_rel; ++j) {
        double best = -1.0;
        int bi = -1;
        for (int64_t i = threadIdx.x; i < N; i += 256) {
            bool taken = false;
            for (int q = 0; q < j; ++q) taken |= s_chosen[q] == int(i);
            const double d = own_d2[i];
            if (!taken && d > best) best = d, bi = int(i);   // rows ascend inside a thread: the lowest row of a tie stays
        }
        s_d[threadIdx.x] = best, s_i[threadIdx.x] = bi;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (int(threadIdx.x) < w) {
                const double od = s_d[threadIdx.x + w];
                const int oi = s_i[threadIdx.x + w];
                if (oi >= 0 && (s_i[threadIdx.x] < 0 || od > s_d[threadIdx.x] || (od == s_d[threadIdx.x] && oi < s_i[threadIdx.x])))
                    s_d[threadIdx.x] = od, s_i[threadIdx.x] = oi;
            }
            __syncthreads();
        }
        const int f = s_i[0];
        if (f < 0) {   // no row left with a comparable distance (the entries refuse non-finite input; kept so that no index is ever -1)
            if (threadIdx.x == 0) ctl->n_rel = j;
            return;    // (block-uniform: every thread read the same s_i[0])
        }
        __syncthreads();   // (everybody has read s_i[0] before the next round writes it)
        if (threadIdx.x == 0) {
            s_chosen[j] = f;
            ctl->rel_e[j] = s_empty[j], ctl->rel_f[j] = f, ctl->rel_from[j] = labels[f];
        }
        __syncthreads();
    }
}

// grid (k, ceil(D / 64)); 256 threads = 64 columns x 4 member lanes.  C is updated in place; shift_part[c * slices + slice] = the
// slice's share of |C_new[c] - C[c]|^2
// (workgroup (c, slice) of a grid (k, slices))
__device__ inline void dv_kmeans_update(const double *__restrict__ X, int D, const int32_t *__restrict__ members, const int32_t *__restrict__ offs,
                                        const int32_t *__restrict__ counts, const KmControl *__restrict__ ctl, double *__restrict__ C,
                                        double *__restrict__ shift_part, int c, int slice, int slices) {
    __shared__ double s[4][64];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6, d = slice * 64 + col;
    const int m0 = offs[c], cnt = counts[c];
    double acc = 0.0;
    if (d < D)
        for (int j = g; j < cnt; j += 4) acc += X[int64_t(members[m0 + j]) * D + d];
    s[g][col] = acc;
    __syncthreads();
    if (g != 0) return;
    double sh = 0.0;
    if (d < D) {
        double sum = ((s[0][col] + s[1][col]) + s[2][col]) + s[3][col];
        int n = cnt;
        const int n_rel = ctl->n_rel;
        for (int j = 0; j < n_rel; ++j) {
            if (ctl->rel_f[j] < 0) break;
            const double xf = X[int64_t(ctl->rel_f[j]) * D + d];
            if (ctl->rel_from[j] == c) sum -= xf, n -= 1;
            if (ctl->rel_e[j] == c) sum = xf, n = 1;
        }
        const double old = C[int64_t(c) * D + d];
        const double nw = n > 0 ? sum / double(n) : old;
        C[int64_t(c) * D + d] = nw;
        sh = (nw - old) * (nw - old);
    }
    sh = dv_wave_sum(sh);
    if (col == 0) shift_part[size_t(c) * slices + slice] = sh;
}
// one wavefront: the iteration's shift, in a fixed order
__device__ inline void dv_kmeans_control(const double *__restrict__ shift_part, int n_part, const int *__restrict__ changed, KmControl *__restrict__ ctl) {
    double acc = 0.0;
    for (int q = threadIdx.x; q < n_part; q += 64) acc += shift_part[q];
    acc = dv_wave_sum(acc);
    if (threadIdx.x == 0) ctl->shift = acc, ctl->changed = *changed;
}

// ---------------------------------------------------------------------------------------------------
// the pick (torsion_module.py:894-922), one workgroup per cluster; picked[c] = -1 for an empty cluster.
//  energies: the member of lowest energy, the first in row order on a tie (sorted() is stable, :901).
//  no energies: the member of largest cumdist, the first on a tie (:919-921), where for the member at POSITION p of its cluster's
//  list  cumdist = sum over the centres c != p, over the atoms, of |centre_c[a] - member[a]|  -- the reference's `c` at :919 is the
//  loop variable of enumerate(cluster), the member's position, not its cluster; with p >= k no centre is left out.
__device__ inline void dv_diverse_pick(const double *__restrict__ X, int n, const int32_t *__restrict__ members, const int32_t *__restrict__ offs,
                                       const int32_t *__restrict__ counts, const double *__restrict__ C, int k, const double *__restrict__ energies,
                                       int32_t *__restrict__ picked, int c) {
    __shared__ double s_v[4];
    __shared__ int s_p[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int m0 = offs[c], cnt = counts[c], D = 3 * n;
    if (cnt == 0) {
        if (threadIdx.x == 0) picked[c] = -1;
        return;
    }
    double best = 0.0;
    int bp = -1;
    if (energies) {
        for (int p = threadIdx.x; p < cnt; p += 256) {
            const double v = -energies[members[m0 + p]];
            if (bp < 0 || v > best) best = v, bp = p;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int op = __shfl_xor(bp, off);
            if (op >= 0 && (bp < 0 || ov > best || (ov == best && op < bp))) best = ov, bp = op;
        }
    } else {
        for (int p = wid; p < cnt; p += 4) {
            const double *x = X + int64_t(members[m0 + p]) * D;
            double acc = 0.0;
            for (int e = lane; e < k * n; e += 64) {
                const int cc = e / n, a = e - cc * n;
                if (cc == p) continue;
                const double dx = C[int64_t(cc) * D + 3 * a] - x[3 * a], dy = C[int64_t(cc) * D + 3 * a + 1] - x[3 * a + 1],
                             dz = C[int64_t(cc) * D + 3 * a + 2] - x[3 * a + 2];
                acc += sqrt(dx * dx + dy * dy + dz * dz);
            }
            acc = dv_wave_sum(acc);
            if (bp < 0 || acc > best) best = acc, bp = p;
        }
    }
    if (lane == 0) s_v[wid] = best, s_p[wid] = bp;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q)
            if (s_p[q] >= 0 && (bp < 0 || s_v[q] > best || (s_v[q] == best && s_p[q] < bp))) best = s_v[q], bp = s_p[q];
        picked[c] = members[m0 + bp];
    }
}

// ---------------------------------------------------------------------------------------------------
// k-means++ seeding without local trials.  rows[j] is the seed chosen last; min_d2[i] = min(min_d2[i], |x_i - x_rows[j]|^2)
__device__ inline void dv_kmeans_seed_update(const double *__restrict__ X, int64_t N, int D, const int32_t *__restrict__ rows, int j,
                                             double *__restrict__ min_d2, int64_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t i = block * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double *y = X + int64_t(rows[j]) * D;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = X[i * D + d] - y[d];
        acc += v * v;
    }
    acc = dv_wave_sum(acc);
    if (lane == 0) min_d2[i] = (j == 0 || acc < min_d2[i]) ? acc : min_d2[i];
}
// rows[j] = the first row whose running sum of min_d2 (row order) exceeds u[j] * total.  One workgroup of 1024: a contiguous piece
// per thread, a scan of the pieces' sums, then the piece that crosses the target is walked again.
__device__ inline void dv_kmeans_seed_pick(const double *__restrict__ min_d2, int64_t N, const double *__restrict__ u, int j, int32_t *__restrict__ rows) {
    __shared__ double s[1024];
    __shared__ int s_first;
    const int t = threadIdx.x;
    const int64_t per = ceil_div<int64_t>(N, 1024), lo = per * t < N ? per * t : N, hi = lo + per < N ? lo + per : N;
    double acc = 0.0;
    for (int64_t i = lo; i < hi; ++i) acc += min_d2[i];
    s[t] = acc;
    if (t == 0) s_first = 1024;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan of the pieces
        const double add = t >= off ? s[t - off] : 0.0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const double target = u[j] * s[1023];
    const double incl = s[t], excl = t ? s[t - 1] : 0.0;
    if (incl > target && hi > lo) atomicMin(&s_first, t);
    __syncthreads();
    if (s_first == 1024) {
        if (t == 0) rows[j] = int32_t(N - 1);   // (total == 0: every row coincides with a seed)
        return;
    }
    if (t == s_first) {
        double run = excl;
        int64_t pick = hi - 1;
        for (int64_t i = lo; i < hi; ++i) {
            run += min_d2[i];
            if (run > target) {
                pick = i;
                break;
            }
        }
        rows[j] = int32_t(pick);
    }
}

// ---------------------------------------------------------------------------------------------------
// the limits of the entry points (diverse.hip, select_batch.hip), checked on the host arrays

// scikit-learn refuses NaN / infinity with a ValueError; here they would turn every distance into NaN (no row ever nearer to any
// centre) -- refused on the host arrays before anything touches the device
inline int check_finite(const char *who, const char *what, const double *v, size_t count) {
    for (size_t q = 0; q < count; ++q) TSC_REQUIRE(std::isfinite(v[q]), "%s: %s[%zu] is not finite", who, what, q);
    return 0;
}
inline int check_uniforms(const char *who, const double *u, int k) {
    for (int j = 0; j < k; ++j) TSC_REQUIRE(u[j] >= 0.0 && u[j] < 1.0, "%s: u[%d] not in [0, 1)", who, j);
    return 0;
}

inline int check_shape(const char *who, int64_t N, int n_atoms) {
    TSC_REQUIRE(N >= 1 && N < INT32_MAX, "%s: %lld structures (1 .. %d)", who, (long long)N, INT32_MAX - 1);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= DV_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, DV_MAX_ATOMS);
    return 0;
}
inline int check_k(const char *who, int64_t N, int64_t D, int k) {
    TSC_REQUIRE(N >= 1 && N < INT32_MAX, "%s: %lld rows (1 .. %d)", who, (long long)N, INT32_MAX - 1);
    TSC_REQUIRE(D >= 1 && D <= 3 * DV_MAX_ATOMS, "%s: %lld columns (1 .. %d)", who, (long long)D, 3 * DV_MAX_ATOMS);
    TSC_REQUIRE(k >= 1 && k <= DV_MAX_K, "%s: %d clusters (1 .. %d)", who, k, DV_MAX_K);
    TSC_REQUIRE(k <= N, "%s: %d clusters for %lld rows", who, k, (long long)N);
    return 0;
}

}  // namespace tsc
