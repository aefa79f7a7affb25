// embed_clash.hpp -- K1 (batched rigid-body embedding) and K2 (compenetration mask): the fragment table, the device functions,
// arguments, bounds and LDS sizes that the kernels and the host share.  No kernel here, so any unit may include it (host.hpp and
// call.hpp do); k_transform is in embed_transform.hpp, the clash kernels and k_all_dists in embed_clash_kernels.hpp.
//
// K1  out[s] = concat_m (R[s,m] @ X_m[c[s,m]].T).T + t[s,m]         reference embeds.py:961-969
// K2  mask[s] = count(all_dists(frag_b, frag_a) < thresh) <= max     reference numba_functions.py:59-105
//
// Both are HBM-streaming kernels: K1 writes n*24 B per pose, K2 reads n*24 B per pose.  K2 stages each
// pose once in LDS (one pose per LP-lane group of a wavefront), every lane owns one atom of the
// "later" fragments and walks the atoms of the earlier fragments, which all lanes of the group read
// from the same LDS address (a broadcast); the per-pose count is reduced with cross-lane shuffles.
#pragma once
#include "common.hpp"

namespace tsc {

constexpr int MAX_MOLS = 8;

struct FragTable {
    int n_mols;
    int n_total;                 // atoms per pose
    long long frag_off[MAX_MOLS];  // offset of fragment m in `frags`, in doubles
    int n_atoms[MAX_MOLS];
    int n_conf[MAX_MOLS];
    int atom_off[MAX_MOLS + 1];  // first atom of fragment m inside a pose
};

__device__ inline int frag_of_atom(const FragTable &ft, int a) {
    int m = 0;
#pragma unroll
    for (int k = 1; k < MAX_MOLS; ++k)
        if (k < ft.n_mols && a >= ft.atom_off[k]) m = k;
    return m;
}

// one atom of one pose: R x + t
__device__ inline void embed_atom(const double *__restrict__ frags, const FragTable &ft, const int32_t *__restrict__ conf_idx,
                                  const double *__restrict__ rot, const double *__restrict__ pos, int64_t s, int a, double out[3]) {
    int m = frag_of_atom(ft, a);
    int64_t sm = s * ft.n_mols + m;
    const double *X = frags + ft.frag_off[m] + (int64_t(conf_idx[sm]) * ft.n_atoms[m] + (a - ft.atom_off[m])) * 3;
    const double *R = rot + sm * 9;
    const double *t = pos + sm * 3;
    double x0 = X[0], x1 = X[1], x2 = X[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * x0 + R[3 * i + 1] * x1 + R[3 * i + 2] * x2 + t[i];
}

// one atom of one pose from pose parameters staged in LDS: R [entries][9], t [entries][3], conformer [entries],
// entry l = local pose * n_mols + fragment.  (Fetching R and t per atom from global memory costs 12 vector loads per
// atom, all hitting the same few lines: the address unit, not the bandwidth, then bounds the embedding kernels.)
__device__ inline void embed_atom_staged(const double *__restrict__ frags, const FragTable &ft, const double *sR, const double *sT, const int *sC,
                                         int local_pose, int a, double out[3]) {
    const int m = frag_of_atom(ft, a), l = local_pose * ft.n_mols + m;
    const double *X = frags + ft.frag_off[m] + (int64_t(sC[l]) * ft.n_atoms[m] + (a - ft.atom_off[m])) * 3;
    const double *R = sR + l * 9, *t = sT + l * 3;
    const double x0 = X[0], x1 = X[1], x2 = X[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * x0 + R[3 * i + 1] * x1 + R[3 * i + 2] * x2 + t[i];
}

// k_transform (embed_transform.hpp): poses per workgroup and round, and the dynamic LDS they take
constexpr int TR_POSES = 32;
__host__ __device__ inline size_t transform_lds_bytes(int n_mols) { return size_t(TR_POSES) * n_mols * (12 * sizeof(double) + sizeof(int)) + TR_POSES * sizeof(int64_t); }

struct ClashArgs {
    int64_t n_poses;
    int n;          // atoms per pose
    int first_row;  // first atom that owns a row of the count (atoms of fragments >= 1; 0 for ids=None)
    int self_mode;  // 1: ids=None -> count_clashes semantics (all ordered pairs i != j with 0 < d < 0.5)
    int lp;         // lanes per pose (power of two, <= 64)
    int n_mols;
    int atom_off[MAX_MOLS + 1];
    double sq_bound;  // d < thresh  <=>  d2 < sq_bound   (exact: see clash_sq_bound)
    long long max_clashes;
};

// Smallest double x with sqrt(x) >= thresh, so that (sqrt(d2) < thresh) == (d2 < x) for every d2:
// IEEE sqrt is correctly rounded and monotone.  Lets the kernels compare squared distances while
// giving the verdict of the reference's `all_dists(...) < thresh` (algebra.py:133-155, sqrt then <).
inline double clash_sq_bound(double thresh) {
    if (!(thresh > 0)) return 0.0;
    double x = thresh * thresh;
    while (std::sqrt(x) >= thresh) x = std::nextafter(x, 0.0);
    while (std::sqrt(x) < thresh) x = std::nextafter(x, INFINITY);
    return x;
}

typedef float clash_f32x2 __attribute__((ext_vector_type(2)));

// LDS bytes one wavefront of k_clash needs: the fp64 pose(s) and, for MINMODE, an fp32 copy as three arrays
__host__ __device__ inline size_t clash_lds_per_wave(int n, int lp, bool minmode) {
    const int ppw = 64 / lp, npad = (n + 1) & ~1;
    return size_t(ppw) * n * 3 * sizeof(double) + (minmode ? size_t(ppw) * 3 * npad * sizeof(float) : 0);
}

// MINMODE (max_clashes == 0, no counts wanted -- the pipeline's case): the verdict is "no inter-fragment distance
// below thresh", i.e. min d^2 >= sq_bound.  The minimum is taken in packed fp32 (two partner atoms per instruction,
// v_pk_add_f32 / v_pk_fma_f32 / v_min3_f32: 3.5 instructions per pair against 8 in fp64) on an fp32 copy of the pose,
// and decided with a rigorous error bound: with C = max |coordinate| of the pose, u = 2^-24 and e = 4 u C (1 + u) the
// computed s32 differs from the exact d^2 by at most 4 u s32 + 2 sqrt(3) e d + 3 e^2, so s32 >= hi = x0 + M means
// d^2 >= x0 and s32 < lo = x0 - M means d^2 < x0 (M below).  A pose whose minimum falls between lo and hi (a few in
// 10^4) is decided by the fp64 count like everything else.
// lo / hi of the comment above for the squared bound x0 and the coordinate bound cmax; false = no usable band (take fp64)
__device__ inline bool fp32_min_band(double x0, double cmax, float *lo_out, float *hi_out) {
    constexpr double U = 5.9604644775390625e-08;  // 2^-24
    const double e = 4.0 * U * cmax * (1.0 + U);
    const double M = 1.01 * (8.0 * U * x0 + (2.0 * 1.7320508075688774 * e * sqrt(x0) + 3.0 * e * e) * (1.0 + 4.0 * U));
    float lo = float(x0 - M), hi = float(x0 + M);
    if (double(lo) > x0 - M) lo = __uint_as_float(__float_as_uint(lo) - 1u);  // round towards the safe side (both > 0)
    if (double(hi) < x0 + M) hi = __uint_as_float(__float_as_uint(hi) + 1u);
    *lo_out = lo, *hi_out = hi;
    return cmax < 1.0e15 && x0 - M > 0.0;
}

inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace tsc
