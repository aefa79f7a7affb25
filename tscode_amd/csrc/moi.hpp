// moi.hpp -- SURVEY.md 8(f) N4: moments of inertia (tscode/algebra.py:165-213), their pair search, embed scores.
//
// get_moi_similarity_matches recomputes the moments of structure j for every pair (i, j); here they are computed once per
// structure (one thread each: centre of mass, inertia tensor, cyclic Jacobi, eigenvalues ordered by absolute value as
// diagonalize does), then one wavefront per row looks for the first j > i whose three moments all lie within
// max_deviation (relative to row i's) -- the same launch shape as the torsion-fingerprint search (tfd.hpp).  The graph
// step of prune_by_moment_of_inertia stays on the host (tscode_amd/optimization_methods.py).
//
// No kernel here: the device functions.  The kernels of one ensemble and k_embed_scores are in moi_kernels.hpp, those that take many
// ensembles per launch in refine_batch.hpp.
#pragma once
#include "common.hpp"

namespace tsc {

// get_inertia_moments (algebra.py:165-186, diagonalize :207-213) of the structure c[n][3]: centre of mass, tensor, cyclic Jacobi,
// eigenvalues ordered by absolute value into out[3].  The plain and the segmented kernel both call this, so a moment cannot differ
// between the two routes.
__device__ inline void inertia_moments_of(const double *__restrict__ c, int n, const double *__restrict__ masses, double *__restrict__ out) {
    double tot = 0, com0 = 0, com1 = 0, com2 = 0;
    for (int a = 0; a < n; ++a) {  // algebra.py:215-223
        const double m = masses[a];
        tot += m, com0 += c[3 * a] * m, com1 += c[3 * a + 1] * m, com2 += c[3 * a + 2] * m;
    }
    com0 /= tot, com1 /= tot, com2 /= tot;
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < n; ++a) {  // :177-182
        const double x = c[3 * a] - com0, y = c[3 * a + 1] - com1, z = c[3 * a + 2] - com2, m = masses[a];
        const double r2 = x * x + y * y + z * z;
        A[0][0] += m * (r2 - x * x), A[0][1] += m * (-x * y), A[0][2] += m * (-x * z);
        A[1][1] += m * (r2 - y * y), A[1][2] += m * (-y * z), A[2][2] += m * (r2 - z * z);
    }
    A[1][0] = A[0][1], A[2][0] = A[0][2], A[2][1] = A[1][2];
    for (int sweep = 0; sweep < 60; ++sweep) {  // cyclic Jacobi, constant indices only
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-32 * dia)) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    t = theta < 0.0 ? -t : t;
                    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = cs * akp - sn * akq, A[k][q] = sn * akp + cs * akq;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = cs * apk - sn * aqk, A[q][k] = sn * apk + cs * aqk;
                    }
                }
            }
    }
    double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2], t;  // order by |eigenvalue| (:209)
    if (fabs(e0) > fabs(e1)) t = e0, e0 = e1, e1 = t;
    if (fabs(e1) > fabs(e2)) t = e1, e1 = e2, e2 = t;
    if (fabs(e0) > fabs(e1)) t = e0, e0 = e1, e1 = t;
    out[0] = e0, out[1] = e1, out[2] = e2;
}

// Row i of the pair search (algebra.py:188-205) over the moments mo[N][3], by one wavefront: the first j > i with
// all(|im_i - im_j| / im_i < max_deviation), -1 if none.  The same value in every lane; k_moi_first_similar and k_moi_first_similar_seg call this.
__device__ inline int32_t moi_first_similar_row(const double *__restrict__ mo, int64_t N, int64_t i, double max_deviation, int lane) {
    const double a0 = mo[3 * i], a1 = mo[3 * i + 1], a2 = mo[3 * i + 2];
    int32_t found = -1;
    for (int64_t j0 = i + 1; j0 < N && found < 0; j0 += 64) {
        const int64_t j = j0 + lane;
        bool sim = false;
        if (j < N) sim = fabs(a0 - mo[3 * j]) / a0 < max_deviation && fabs(a1 - mo[3 * j + 1]) / a1 < max_deviation && fabs(a2 - mo[3 * j + 2]) / a2 < max_deviation;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(sim);
        if (m) found = int32_t(j0 + (__ffsll((long long)m) - 1));
    }
    return found;
}

}  // namespace tsc
