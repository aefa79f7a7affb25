// descriptor.hpp -- the rotation-invariant descriptors of the prune's screen: constants, features, the fp32 limits and the descriptor
// rows of structures staged in LDS.  Device functions and constants only; the kernels that build moments, basis and descriptors are in
// descriptor_kernels.hpp (prune.hip), descriptor_basis.hpp (prune.hip, pipeline.hip) and pose_describe.hpp (pipeline.hip).
//
// rmsd_and_max_numba (tscode/rmsd_pruning.py:6-41) rotates p onto q ABOUT THE ORIGIN (it never centres).
// Write dev_a = |p_a R - q_a| for the deviation of atom a after the optimal rotation R; h * rmsd^2 = sum_a dev_a^2.
// Two families of quantities are untouched by R, and each bounds the deviations from below:
//
//   family 0  atom norms:           n_a(x) = |x_a|                      dev_a           >= | n_a(p) - n_a(q) |
//   family 1  atom-pair distances:  d_ab(x) = |x_a - x_b|               dev_a + dev_b   >= | d_ab(p) - d_ab(q) |
//             over DISJOINT pairs (a, b = a + h/2), so that             dev_a^2 + dev_b^2 >= (d_ab(p) - d_ab(q))^2 / 2
//
// Hence, with f0(x) = (n_a)_a and f1(x) = (d_ab / sqrt 2)_(a,b):   h * rmsd(p,q)^2 >= |f(p) - f(q)|^2 >= |Q^T (f(p) - f(q))|^2
// for either family and any Q with orthonormal columns.  A pair for which one of the two right-hand sides exceeds
// h * thr^2 cannot have rmsd < thr (:75) and is dropped without forming H = p^T q.  Q (KD columns per family) spans the
// leading principal axes of the feature vectors of the ensemble; the choice of Q (and of the atom pairs) only
// changes how many pairs are dropped, never a verdict.  Everything that survives takes the same sign test and
// explicit-rotation path as the register-tiled kernel (rmsd_tile.hpp).
//
// The screen runs in fp32 on mean-centred descriptors.  With M the largest |component| of the ensemble, every computed
// difference is within eta = 3 * 2^-24 * 2M of the exact one (rounding of both operands and of the subtraction), so
// s_exact >= s32 (1 - 2^-20) - 2 eta sqrt(KD s32); screen_limit32 turns h thr^2 into the fp32 limit above which that
// lower bound certainly exceeds h thr^2.  Pairs in the sliver between the two limits are simply not dropped.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace tsc {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KD = 8;              // descriptor dimensions per family
constexpr int NFAM = 2;            // feature families
constexpr int DW = KD * NFAM;      // doubles per structure descriptor
constexpr int DESC_SAMPLE = 4096;  // structures used to estimate the principal axes
constexpr int DESC_MAX_FEAT = 256; // features per family that enter the descriptor (any subset keeps the bound valid)
constexpr unsigned NONFINITE_BITS = 0x7fc00000u;  // what the running maximum of |descriptor| reads once a non-finite structure was seen

// floats per structure of the float32 copy of the heavy atoms (pair_stage1 below): x y z of four atoms per three float4, zero-padded
__host__ __device__ inline int heavy32_pitch(int h) { return 12 * ((h + 3) / 4); }

// feature a of family fam of the structure at x (h atoms, xyz triples)
__device__ inline double feature(const double *__restrict__ x, int h, int fam, int a) {
    if (fam == 0) return sqrt(x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1] + x[3 * a + 2] * x[3 * a + 2]);
    const int b = a + h / 2;
    const double dx = x[3 * a] - x[3 * b], dy = x[3 * a + 1] - x[3 * b + 1], dz = x[3 * a + 2] - x[3 * b + 2];
    return sqrt(0.5 * (dx * dx + dy * dy + dz * dz));
}

inline int n_features(int h, int fam) { return std::min(fam == 0 ? h : h / 2, DESC_MAX_FEAT); }

constexpr int MOM_BLOCKS = 32;   // partial moment matrices per family (descriptor_kernels.hpp: k_feature_moments)

// fp32 limit of the screen for an exact limit `limit` = h thr^2, from the largest descriptor magnitude dmax: every computed
// difference of two components is within eta = 3 * 2^-24 * 2 dmax of the exact one, the 8-term sum of squares carries at most
// 2^-20 relative error, so s_exact >= s32 (1 - 2^-20) - 2 eta sqrt(KD s32); the limit returned is the smallest s32 above which
// that lower bound certainly exceeds `limit`.  A NaN / inf dmax gives a limit that drops nothing.
__device__ inline float screen_limit32(float dmaxf, double limit) {
    const double dmax = (dmaxf >= 0.0f && dmaxf < 3.0e38f) ? double(dmaxf) : 3.0e38;
    const double eta = 3.0 * 5.9604644775390625e-08 * 2.0 * dmax;               // 3 * 2^-24 * 2 dmax
    const double a = 1.0 - 9.5367431640625e-07, b = 2.0 * eta * sqrt(double(KD));  // 1 - 2^-20
    const double x = (b + sqrt(b * b + 4.0 * a * limit)) / (2.0 * a);
    const double l32 = x * x * (1.0 + 1e-6) + 1e-30;
    float f = float(l32);
    if (double(f) < l32) f = __uint_as_float(__float_as_uint(f) + 1u);  // next float up (f > 0)
    return (l32 < 3.0e38) ? f : 3.4e38f;
}

// The same limit for the screen as the pair kernel computes it: S = fl(fl(|a|^2 + |b|^2) - 2 fl(a.b)) on the stored fp32
// vectors a, b (8-term fma chains), which costs 10 packed instructions per column instead of 16 for sum (a_k - b_k)^2.  With
// u = 2^-24 and g8 = 8u / (1 - 8u):  | |a|^2_fl - |a|^2 | <= g8 |a|^2,  | a.b_fl - a.b | <= g8 (|a|^2 + |b|^2) / 2,  so the
// exact T = |a - b|^2 satisfies  T >= S (1 - 2u) - E,  E = (2 g8 + u (1 + g8)) (|a|^2 + |b|^2) <= (2 g8 + u (1 + g8)) 2 KD M^2.
// The kernel's other association, S' = fl(|a|^2_fl - 2 fl(-|b|^2_fl / 2 + a.b)) (the chain of 8 fmas starts from the
// halved column norm, an exact scaling), carries g8 (|b|^2 (1 + g8) / 2 + (|a|^2 + |b|^2) / 2) in the chain, twice that after
// the exact factor, plus the two norm roundings: at most g8 (2 |a|^2 + 3 |b|^2)(1 + g8) <= 3 g8 (|a|^2 + |b|^2) (1 + g8)
// beside the final u: the E below (3 g8 in place of 2) covers both associations.
// The stored components are roundings of the exact descriptors, each difference within eta = 3 * 2^-24 * 2M of the exact
// one as above, so s_exact >= T - 2 eta sqrt(KD T) (increasing in T beyond KD eta^2): a pair whose S exceeds the returned
// value certainly has s_exact > limit.
__device__ inline float screen_limit32_dot(float dmaxf, double limit) {
    const double dmax = (dmaxf >= 0.0f && dmaxf < 3.0e38f) ? double(dmaxf) : 3.0e38;
    constexpr double U = 5.9604644775390625e-08, G8 = 8.0 * U / (1.0 - 8.0 * U);
    const double eta = 3.0 * U * 2.0 * dmax;
    const double b = 2.0 * eta * sqrt(double(KD));
    const double y = 0.5 * (b + sqrt(b * b + 4.0 * limit));   // sqrt of the smallest T with T - b sqrt(T) >= limit
    const double E = (3.0 * G8 * (1.0 + G8) + U * (1.0 + G8)) * 2.0 * double(KD) * dmax * dmax;
    const double l32 = (y * y + E) / (1.0 - 2.0 * U) * (1.0 + 1e-6) + 1e-30;
    float f = float(l32);
    if (double(f) < l32) f = __uint_as_float(__float_as_uint(f) + 1u);  // next float up (f > 0)
    return (l32 < 3.0e38) ? f : 3.4e38f;
}

}  // namespace tsc
