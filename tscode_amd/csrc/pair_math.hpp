// pair_math.hpp -- K3, the arithmetic of ONE pair: Kabsch-rotation RMSD (no centring), exactly and by the quartic tests.  Device functions
// only, no kernel: included by every kernel that compares two structures (the prune's pair kernels through pair_stages.hpp; csearch.hpp,
// diverse.hpp, rot_corr.hpp, cross.hpp, prune_batch.hpp) without any of the prune's pass machinery.
//
// Reference: tscode/rmsd_pruning.py.  rmsd_and_max_numba(p, q) (:6-41) rotates p onto q with the optimal
// PROPER rotation about the origin (SVD of H = p^T q with the det sign fix, no centring) and returns the
// RMSD and the largest per-atom deviation.  Two formulations of that same optimum are used here:
//
//  * the FILTER (tile kernel, every pair): the optimum satisfies  h * rmsd^2 = Gp + Gq - 2 * lmax,  where
//    lmax = s1 + s2 + sign(det H) * s3 is the largest root of the quartic  P(l) = l^4 + c2 l^2 + c1 l + c0,
//    c2 = -2 |H|_F^2, c1 = -8 det H, c0 = |H|_F^4 - 4 |cof H|_F^2   (characteristic polynomial of Horn's
//    4x4 quaternion matrix).  With L = (Gp + Gq - h thr^2) / 2, rmsd >= thr  <=>  lmax <= L, and since all
//    four roots are real, L > lmax  <=>  P(L) > 0, P'(L) > 0, P''(L) > 0 (for L > 0).  A pair is REJECTED
//    only when the three values exceed a rounding-error bound, so a rejection is always right; every
//    other pair goes to
//    (a second test of the same quartic ACCEPTS near-duplicates outright, see pair_verdict)
//  * the EXACT path (explicit rotation): the quaternion of the optimal rotation is the top eigenvector of
//    Horn's matrix (Newton for the eigenvalue + adjugate column, cyclic Jacobi when that degenerates, fp64);
//    p is rotated, the residual is formed atom by atom and rmsd = sqrt(sum |d|^2 / h), maxdev = max |d| are
//    compared with the thresholds exactly as the reference does (:75).  Values agree with the reference's
//    LAPACK path to ~1e-13.
//
#pragma once
#include "common.hpp"

namespace tsc {

// ---------------------------------------------------------------------------------------------------
// exact path

// Cyclic Jacobi on a symmetric 4x4 (full storage, constant indices only so it lives in registers).
// Returns the eigenvector of the largest eigenvalue in q[4].
__device__ inline void top_eigvec4(double A[4][4], double q[4]) {
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dia += A[i][i] * A[i][i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                double apq = A[p][r];
                if (apq != 0.0) {
                    double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    t = theta < 0.0 ? -t : t;
                    double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {  // columns p, r of A and V
                        double akp = A[k][p], akr = A[k][r];
                        A[k][p] = c * akp - s * akr;
                        A[k][r] = s * akp + c * akr;
                        double vkp = V[k][p], vkr = V[k][r];
                        V[k][p] = c * vkp - s * vkr;
                        V[k][r] = s * vkp + c * vkr;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {  // rows p, r of A
                        double apk = A[p][k], ark = A[r][k];
                        A[p][k] = c * apk - s * ark;
                        A[r][k] = s * apk + c * ark;
                    }
                }
            }
        }
    }
    double best = A[0][0];
    q[0] = V[0][0], q[1] = V[1][0], q[2] = V[2][0], q[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        bool b = A[k][k] > best;
        best = b ? A[k][k] : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = b ? V[i][k] : q[i];
    }
}

// The same cyclic Jacobi on matrices that live in memory (LDS): A[16], V[16] row-major, dynamic indices.  The register
// version above costs 64 VGPRs for its two matrices; a kernel that wants a small register footprint runs this one for
// the (rare) degenerate pairs, one lane at a time on a 256-byte area per wavefront.
__device__ inline void top_eigvec4_mem(double *A, double *V, double q[4]) {
#pragma nounroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma nounroll
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma nounroll
        for (int i = 0; i < 4; ++i) {
            dia += A[5 * i] * A[5 * i];
#pragma nounroll
            for (int j = i + 1; j < 4; ++j) off += A[4 * i + j] * A[4 * i + j];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma nounroll
        for (int p = 0; p < 3; ++p)
#pragma nounroll
            for (int r = p + 1; r < 4; ++r) {
                const double apq = A[4 * p + r];
                if (apq != 0.0) {
                    const double theta = (A[5 * r] - A[5 * p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    t = theta < 0.0 ? -t : t;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma nounroll
                    for (int k = 0; k < 4; ++k) {  // columns p, r of A and V
                        const double akp = A[4 * k + p], akr = A[4 * k + r];
                        A[4 * k + p] = c * akp - s * akr;
                        A[4 * k + r] = s * akp + c * akr;
                        const double vkp = V[4 * k + p], vkr = V[4 * k + r];
                        V[4 * k + p] = c * vkp - s * vkr;
                        V[4 * k + r] = s * vkp + c * vkr;
                    }
#pragma nounroll
                    for (int k = 0; k < 4; ++k) {  // rows p, r of A
                        const double apk = A[4 * p + k], ark = A[4 * r + k];
                        A[4 * p + k] = c * apk - s * ark;
                        A[4 * r + k] = s * apk + c * ark;
                    }
                }
            }
    }
    int kb = 0;
#pragma nounroll
    for (int k = 1; k < 4; ++k)
        if (A[5 * k] > A[5 * kb]) kb = k;
    for (int i = 0; i < 4; ++i) q[i] = V[4 * i + kb];
}

// 3x3 determinant of the minor of the symmetric 4x4 A that drops row I and column J, with the cofactor sign.
template <int I, int J>
__device__ inline double cofactor4(const double (&A)[4][4]) {
    constexpr int r0 = (I == 0) ? 1 : 0, r1 = (I <= 1) ? 2 : 1, r2 = (I <= 2) ? 3 : 2;
    constexpr int c0 = (J == 0) ? 1 : 0, c1 = (J <= 1) ? 2 : 1, c2 = (J <= 2) ? 3 : 2;
    const double d = A[r0][c0] * (A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1]) -
                     A[r0][c1] * (A[r1][c0] * A[r2][c2] - A[r1][c2] * A[r2][c0]) +
                     A[r0][c2] * (A[r1][c0] * A[r2][c1] - A[r1][c1] * A[r2][c0]);
    return ((I + J) & 1) ? -d : d;
}

// The explicit-rotation half of rmsd_and_max_numba (rmsd_pruning.py:19-39) given S = p^T q (:15) and the squared
// norms Gp, Gq.  The quaternion of the optimal proper rotation is the top eigenvector of Horn's matrix N(S):
//   fast path : largest root of the characteristic quartic by Newton from the upper bound (Gp+Gq)/2 (monotone), then
//               the eigenvector as the best-conditioned column of adj(N - l I);
//   fallback  : cyclic Jacobi, when the top eigenvalue is (nearly) degenerate and the adjugate collapses
//               (collinear / planar-through-origin / mirror-symmetric cases).
// A group of `lpp` consecutive lanes (a power of two, all converged, all holding the same S) may share one pair:
// lane `sub` of the group then takes atoms sub, sub + lpp, ... of the residual loop and the group reduces.
// Horn's matrix N(S), row-major into 16 doubles
__device__ inline void horn_matrix(const double S[9], double *M) {
    M[0] = S[0] + S[4] + S[8], M[5] = S[0] - S[4] - S[8], M[10] = -S[0] + S[4] - S[8], M[15] = -S[0] - S[4] + S[8];
    M[1] = M[4] = S[5] - S[7], M[2] = M[8] = S[6] - S[2], M[3] = M[12] = S[1] - S[3];
    M[6] = M[9] = S[1] + S[3], M[7] = M[13] = S[6] + S[2], M[11] = M[14] = S[5] + S[7];
}

// Fast way to the rotation quaternion e (not normalised): Newton for the top eigenvalue, then the best-conditioned column
// of adj(N - l I).  Returns false when the top eigenvalue is (nearly) degenerate and the adjugate collapses (collinear /
// planar-through-origin / mirror-symmetric cases): the caller then runs a Jacobi eigen-solver (top_eigvec4 / _mem).
__device__ inline bool rotation_quaternion_fast(const double S[9], double Gp, double Gq, double e[4]) {
    // characteristic quartic l^4 + c2 l^2 + c1 l + c0 (see the sign test below)
    const double F = S[0] * S[0] + S[1] * S[1] + S[2] * S[2] + S[3] * S[3] + S[4] * S[4] + S[5] * S[5] + S[6] * S[6] + S[7] * S[7] + S[8] * S[8];
    const double C0 = S[4] * S[8] - S[5] * S[7], C1 = S[5] * S[6] - S[3] * S[8], C2 = S[3] * S[7] - S[4] * S[6];
    const double C3 = S[2] * S[7] - S[1] * S[8], C4 = S[0] * S[8] - S[2] * S[6], C5 = S[1] * S[6] - S[0] * S[7];
    const double C6 = S[1] * S[5] - S[2] * S[4], C7 = S[2] * S[3] - S[0] * S[5], C8 = S[0] * S[4] - S[1] * S[3];
    const double det = S[0] * C0 + S[1] * C1 + S[2] * C2;
    const double CF = C0 * C0 + C1 * C1 + C2 * C2 + C3 * C3 + C4 * C4 + C5 * C5 + C6 * C6 + C7 * C7 + C8 * C8;
    const double c2 = -2.0 * F, c1 = -8.0 * det, c0 = F * F - 4.0 * CF;
    double lam = 0.5 * (Gp + Gq);
    if (!(lam > 0.0)) return false;
    for (int it = 0; it < 40; ++it) {
        const double l2 = lam * lam;
        const double P = l2 * l2 + c2 * l2 + c1 * lam + c0, P1 = 4.0 * l2 * lam + 2.0 * c2 * lam + c1;
        if (!(P1 > 0.0)) return false;
        const double dl = P / P1;
        lam -= dl;
        if (fabs(dl) <= 1e-15 * fabs(lam)) break;
    }
    double A[4][4];
    {
        double M[16];
        horn_matrix(S, M);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) A[i][j] = M[4 * i + j] - (i == j ? lam : 0.0);
    }
    const double d0 = cofactor4<0, 0>(A), d1 = cofactor4<1, 1>(A), d2 = cofactor4<2, 2>(A), d3 = cofactor4<3, 3>(A);
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) scale = fmax(scale, fabs(A[i][j]));
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2), a3 = fabs(d3);
    const double best = fmax(fmax(a0, a1), fmax(a2, a3));
    if (!(best > 1e-4 * scale * scale * scale)) return false;  // adj(A) = c v v^T with |c| large enough: any big column is v
    if (a0 == best) {
        e[0] = d0, e[1] = cofactor4<0, 1>(A), e[2] = cofactor4<0, 2>(A), e[3] = cofactor4<0, 3>(A);
    } else if (a1 == best) {
        e[0] = cofactor4<1, 0>(A), e[1] = d1, e[2] = cofactor4<1, 2>(A), e[3] = cofactor4<1, 3>(A);
    } else if (a2 == best) {
        e[0] = cofactor4<2, 0>(A), e[1] = cofactor4<2, 1>(A), e[2] = d2, e[3] = cofactor4<2, 3>(A);
    } else {
        e[0] = cofactor4<3, 0>(A), e[1] = cofactor4<3, 1>(A), e[2] = cofactor4<3, 2>(A), e[3] = d3;
    }
    return true;
}

// rmsd and max deviation of p rotated by the quaternion e (w, x, y, z; any length) against q (rmsd_pruning.py:29-39); lpp
// lanes share the pair (atoms sub, sub + lpp, ...) and reduce with a butterfly
__device__ inline void residual_rmsd_maxdev(const double *__restrict__ p, const double *__restrict__ q, int h, const double e[4], double &rmsd,
                                            double &maxdev, int sub = 0, int lpp = 1) {
    const double nn = 1.0 / sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    const double w = e[0] * nn, x = e[1] * nn, y = e[2] * nn, z = e[3] * nn;
    const double R00 = w * w + x * x - y * y - z * z, R01 = 2 * (x * y - w * z), R02 = 2 * (x * z + w * y);
    const double R10 = 2 * (x * y + w * z), R11 = w * w - x * x + y * y - z * z, R12 = 2 * (y * z - w * x);
    const double R20 = 2 * (x * z - w * y), R21 = 2 * (y * z + w * x), R22 = w * w - x * x - y * y + z * z;
    double ss = 0.0, mx = 0.0;
#pragma unroll 2
    for (int a = sub; a < h; a += lpp) {  // :29-39
        const double px = p[3 * a], py = p[3 * a + 1], pz = p[3 * a + 2];
        const double dx = R00 * px + R01 * py + R02 * pz - q[3 * a];
        const double dy = R10 * px + R11 * py + R12 * pz - q[3 * a + 1];
        const double dz = R20 * px + R21 * py + R22 * pz - q[3 * a + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        ss += d2;
        mx = d2 > mx ? d2 : mx;
    }
    for (int off = lpp >> 1; off > 0; off >>= 1) {
        ss += __shfl_xor(ss, off);
        mx = fmax(mx, __shfl_xor(mx, off));
    }
    rmsd = sqrt(ss / double(h));
    maxdev = sqrt(mx);  // max_a sqrt(d2_a) == sqrt(max_a d2_a): sqrt is monotone
}

// The quaternion e (w, x, y, z; any length) of the optimal proper rotation of p onto q, given S = p^T q and the squared norms
__device__ inline void exact_quaternion(const double S[9], double Gp, double Gq, double e[4]) {
    if (!rotation_quaternion_fast(S, Gp, Gq, e)) {
        double N[4][4], M[16];
        horn_matrix(S, M);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) N[i][j] = M[4 * i + j];
        top_eigvec4(N, e);
    }
}

__device__ inline void exact_rmsd_maxdev(const double *__restrict__ p, const double *__restrict__ q, int h, const double S[9],
                                         double Gp, double Gq, double &rmsd, double &maxdev, int sub = 0, int lpp = 1) {
    double e[4];
    exact_quaternion(S, Gp, Gq, e);
    residual_rmsd_maxdev(p, q, h, e, rmsd, maxdev, sub, lpp);
}

// rmsd_and_max_numba (rmsd_pruning.py:6-41) for one pair; p, q point at h consecutive xyz triples.
__device__ inline void rmsd_and_max_pair(const double *__restrict__ p, const double *__restrict__ q, int h, double &rmsd,
                                         double &maxdev) {
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Gp = 0.0, Gq = 0.0;
    for (int a = 0; a < h; ++a) {  // :15 cov_mat = p.T @ q
        const double px = p[3 * a], py = p[3 * a + 1], pz = p[3 * a + 2];
        const double qx = q[3 * a], qy = q[3 * a + 1], qz = q[3 * a + 2];
        S[0] += px * qx, S[1] += px * qy, S[2] += px * qz;
        S[3] += py * qx, S[4] += py * qy, S[5] += py * qz;
        S[6] += pz * qx, S[7] += pz * qy, S[8] += pz * qz;
        Gp += px * px + py * py + pz * pz;
        Gq += qx * qx + qy * qy + qz * qz;
    }
    exact_rmsd_maxdev(p, q, h, S, Gp, Gq, rmsd, maxdev);
}


// Fast tests on the characteristic quartic of Horn's matrix (described at the top of this file).
//   PAIR_DISSIMILAR  certainly rmsd >= thr:  P, P', P'' at L = (Gp + Gq - h thr^2) / 2 all exceed their rounding bounds, so
//                    L lies above the largest root l1 and h rmsd^2 = Gp + Gq - 2 l1 > h thr^2;
//   PAIR_SIMILAR     certainly similar (near-duplicates, the bulk of what a prune removes): with x = (Gp + Gq) / 2 - 2 thr^2 > 0,
//                    P''(x) > 0 and P'(x) > 0 put x above the largest root of P' (the roots of P'' are +-sqrt(|H|_F^2 / 3) and
//                    those of P' interlace them; the other region with both signs lies below the negative root of P''),
//                    hence above the second root l2 of P, and P(x) < 0 then puts it below the largest root l1 (all with
//                    rounding bounds), so h rmsd^2 = Gp + Gq - 2 l1 < 4 thr^2: rmsd < 2 thr / sqrt(h) <= thr
//                    for h >= 4, and maxdev <= sqrt(sum dev^2) = sqrt(h) rmsd < 2 thr -- both conditions of
//                    rmsd_pruning.py:75 hold without forming the rotation (needs maxdev_thr == 2 thr, as :95 sets it);
//   PAIR_UNDECIDED   everything else takes the explicit-rotation path.
enum { PAIR_DISSIMILAR = 0, PAIR_SIMILAR = 1, PAIR_UNDECIDED = 2 };

struct Quartic {
    double F, CF, c2, c1, c0;
};
__device__ inline Quartic horn_quartic(const double H[9]) {
    Quartic q;
    q.F = H[0] * H[0] + H[1] * H[1] + H[2] * H[2] + H[3] * H[3] + H[4] * H[4] + H[5] * H[5] + H[6] * H[6] + H[7] * H[7] + H[8] * H[8];
    const double C0 = H[4] * H[8] - H[5] * H[7], C1 = H[5] * H[6] - H[3] * H[8], C2 = H[3] * H[7] - H[4] * H[6];
    const double C3 = H[2] * H[7] - H[1] * H[8], C4 = H[0] * H[8] - H[2] * H[6], C5 = H[1] * H[6] - H[0] * H[7];
    const double C6 = H[1] * H[5] - H[2] * H[4], C7 = H[2] * H[3] - H[0] * H[5], C8 = H[0] * H[4] - H[1] * H[3];
    const double det = H[0] * C0 + H[1] * C1 + H[2] * C2;
    q.CF = C0 * C0 + C1 * C1 + C2 * C2 + C3 * C3 + C4 * C4 + C5 * C5 + C6 * C6 + C7 * C7 + C8 * C8;
    q.c2 = -2.0 * q.F, q.c1 = -8.0 * det, q.c0 = q.F * q.F - 4.0 * q.CF;
    return q;
}
// Rounding bound of the quartic tests: every comparison below is `value > kappa * (sum of the magnitudes of its terms)`.
// Derivation (u = 2^-53, gamma = h u, S^2 = Gp Gq, rho = ((Gp + Gq) / 2) / L >= S / L, L = the test point):
//   * H: an h-term fma chain per entry, |dH_ij| <= gamma sum_a |p_ai q_aj| <= gamma sqrt(sum p_ai^2 sum q_aj^2), so
//     |dH|_F <= gamma S, and |H|_F <= S (Cauchy-Schwarz);
//   * F = |H|_F^2:  dF <= 2 |H| |dH| <= 2 gamma S^2;  det: d det <= |cof H|_F |dH|_F <= gamma S^3;  CF = |cof H|_F^2:
//     dCF <= 2 |cof| 2 |H| |dH| <= 4 gamma S^4;  hence d(c2 L^2) <= 4 gamma S^2 L^2, d(c1 L) <= 8 gamma S^3 L,
//     d(c0) = 2 F dF + 4 dCF <= 20 gamma S^4: together <= 32 gamma rho^4 L^4 in P, and by the same steps
//     <= 4 gamma rho^3 (4 L^3) in P' and <= gamma rho^2 (6 L^2) in P'';
//   * the test point itself: Gp, Gq are 3h-term sums, |dL| <= 3 gamma (Gp + Gq) / 2 = 3 gamma rho L, which moves P by at most
//     |P'| |dL| <= 12 gamma rho L^4 (and P', P'' by less, relative to their term sums);
//   * evaluating the three polynomials: a few u times the term sums.
// All of it is below 64 h u rho^4 times the respective term sum (each sum contains L^4, 4 L^3, 6 L^2).  kappa is that
// bound, and never less than the 1e-12 the recorded runs were made with (which it exceeds only beyond about 140 heavy atoms
// or where the structures sit so close to the origin that L is small against Gp + Gq): a larger kappa only hands more pairs
// to the explicit-rotation path, it cannot change a verdict.  Structures far from the origin (the path never centres,
// rmsd_pruning.py:7-41) make Gp, Gq and L grow with the square of the offset while the margin P(L) ~ P'(l1) (L - l1) keeps
// L - l1 = h (rmsd^2 - thr^2) / 2: the tests decide less and less (at 10^4 A nothing) and everything takes the exact path.
// H FORMED FROM A FLOAT32 COPY of the coordinates (pair_stages.hpp, pair_H32: the first look at a pair that passed the screen reads half the
// bytes): p32 = p (1 + d), |d| <= 2^-24, products of two floats are exact in float64 and summed there, so
// |dH_ij| <= (2^-23 + 2^-48 + h u) sum_a |p_ai q_aj| and |dH|_F <= gamma32 S with gamma32 = 2.0001 * 2^-24 + h u.  The derivation above goes
// through with that gamma in the H terms (32 gamma32 rho^4) while the test point keeps its float64 bound (12 h u rho): below
// 64 gamma32 rho^4 together.  Such a test decides every pair whose margin is not tiny (|P(L)| is some 1e-3 .. 1e-1 of its term sum for
// the pairs a prune meets, kappa about 8e-6); the others are formed again from the float64 coordinates.
constexpr double QUARTIC_KAPPA_MIN = 1e-12;
__device__ inline double quartic_gamma64(int h) { return 1.1102230246251565e-16 * double(h); }
__device__ inline double quartic_gamma32(int h) { return 2.0001 * 5.9604644775390625e-08 + 1.1102230246251565e-16 * double(h); }
__device__ inline double quartic_kappa_g(double gamma, double half_sum, double L) {
    const double rho = half_sum / L, r2 = rho * rho;          // callers test L > 0 themselves
    const double k = 64.0 * gamma * r2 * r2;
    return (k > QUARTIC_KAPPA_MIN) ? k : QUARTIC_KAPPA_MIN;  // (a NaN k -- L == 0 -- keeps the minimum; the L > 0 test fails then)
}
__device__ inline double quartic_kappa(int h, double half_sum, double L) { return quartic_kappa_g(quartic_gamma64(h), half_sum, L); }

__device__ inline bool quartic_above_top_root(const Quartic &q, double L, double kappa) {
    const double L2 = L * L;
    const double t4 = L2 * L2, t2 = q.c2 * L2, t1 = q.c1 * L;
    const double P = t4 + t2 + t1 + q.c0;
    const double eP = kappa * (t4 + fabs(t2) + fabs(t1) + fabs(q.c0) + 4.0 * q.CF + q.F * q.F);
    const double P1 = 4.0 * L2 * L + 2.0 * q.c2 * L + q.c1;
    const double e1 = kappa * (4.0 * L2 * fabs(L) + 2.0 * fabs(q.c2 * L) + fabs(q.c1));
    const double P2 = 6.0 * L2 + q.c2;
    const double e2 = kappa * (6.0 * L2 + fabs(q.c2));
    return (L > 0.0) && (P > eP) && (P1 > e1) && (P2 > e2);
}
__device__ inline bool quartic_between_top_roots(const Quartic &q, double x, double kappa) {
    const double x2 = x * x;
    const double t4 = x2 * x2, t2 = q.c2 * x2, t1 = q.c1 * x;
    const double P = t4 + t2 + t1 + q.c0;
    const double eP = kappa * (t4 + fabs(t2) + fabs(t1) + fabs(q.c0) + 4.0 * q.CF + q.F * q.F);
    const double P1 = 4.0 * x2 * x + 2.0 * q.c2 * x + q.c1;
    const double e1 = kappa * (4.0 * x2 * fabs(x) + 2.0 * fabs(q.c2 * x) + fabs(q.c1));
    const double P2 = 6.0 * x2 + q.c2;
    const double e2 = kappa * (6.0 * x2 + fabs(q.c2));
    return (x > 0.0) && (P2 > e2) && (P1 > e1) && (P < -eP);
}

// half_sum = (Gp + Gq) / 2, L = half_sum - h thr^2 / 2, h = atoms per structure
__device__ inline bool certainly_dissimilar(const double H[9], double L, double half_sum, int h) {
    return quartic_above_top_root(horn_quartic(H), L, quartic_kappa(h, half_sum, L));
}

// half_sum = (Gp + Gq) / 2, half_h_thr2 = h thr^2 / 2, two_thr2 = 2 thr^2 (pass a negative two_thr2 to switch the
// near-duplicate test off: h < 4, or a maxdev threshold other than 2 thr)
__device__ inline int pair_verdict_g(const double H[9], double half_sum, double half_h_thr2, double two_thr2, double gamma) {
    const Quartic q = horn_quartic(H);
    const double L = half_sum - half_h_thr2;
    if (quartic_above_top_root(q, L, quartic_kappa_g(gamma, half_sum, L))) return PAIR_DISSIMILAR;
    const double x = half_sum - two_thr2;
    if (two_thr2 > 0.0 && quartic_between_top_roots(q, x, quartic_kappa_g(gamma, half_sum, x))) return PAIR_SIMILAR;
    return PAIR_UNDECIDED;
}
__device__ inline int pair_verdict(const double H[9], double half_sum, double half_h_thr2, double two_thr2, int h) {
    return pair_verdict_g(H, half_sum, half_h_thr2, two_thr2, quartic_gamma64(h));
}

}  // namespace tsc
