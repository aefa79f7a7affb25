// pair_stages.hpp -- the evaluation stages of a pair that passed the screen: H = p^T q from memory (float64 or the float32 copy), the
// quartic tests on it and the explicit rotation (pair_math.hpp).  Device functions only: the pair kernels of the prune, group_filter.hpp and
// prune_batch.hpp include this.
#pragma once
#include "descriptor.hpp"
#include "pair_math.hpp"

namespace tsc {

// H = p^T q of one pair read from memory.  `lpp` consecutive lanes (a power of two) share the pair: lane `sub` takes
// atoms sub, sub + lpp, ... and the group sums H with a butterfly, so a batch of few pairs has a short critical path
// (lpp = 64 / batch size) while a full batch runs one pair per lane (lpp = 1).
__device__ inline void pair_H(const double *__restrict__ p, const double *__restrict__ q, int h, int sub, int lpp, double H[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = 0.0;
#pragma unroll 2
    for (int a = sub; a < h; a += lpp) {
        const double px = p[3 * a], py = p[3 * a + 1], pz = p[3 * a + 2];
        const double qx = q[3 * a], qy = q[3 * a + 1], qz = q[3 * a + 2];
        H[0] = fma(px, qx, H[0]), H[1] = fma(px, qy, H[1]), H[2] = fma(px, qz, H[2]);
        H[3] = fma(py, qx, H[3]), H[4] = fma(py, qy, H[4]), H[5] = fma(py, qz, H[5]);
        H[6] = fma(pz, qx, H[6]), H[7] = fma(pz, qy, H[7]), H[8] = fma(pz, qz, H[8]);
    }
    for (int off = lpp >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] += __shfl_xor(H[k], off);
    }
}

// The float32 copy of the heavy atoms that stage 1 reads first: structure i at heavy32 + i * pitch32, pitch32 = 12 * ceil(h / 4) floats
// (x y z of four atoms per three float4; zero-padded).  The gathers of the pairs that pass the screen are what the pair kernels wait
// for -- with the float64 loads issued twice a C4 step takes 18.8 instead of 12.2 ms, a C3 step 1.00 instead of 0.86 -- and the quartic
// tests on H from this copy, with the rounding bound that goes with it (pair_math.hpp: quartic_gamma32), decide all but the pairs with a
// tiny margin; those are formed again from the float64 coordinates, as is everything the explicit-rotation path needs.

// H = p^T q from the float32 copy: lane `sub` of the pair's `lpp` lanes takes the groups of four atoms sub, sub + lpp, ...; the
// products of two floats are exact in float64, the sums run there
__device__ inline void pair_H32(const float *__restrict__ p, const float *__restrict__ q, int hq, int sub, int lpp, double H[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = 0.0;
    for (int g = sub; g < hq; g += lpp) {
        const f32x4 *pv = reinterpret_cast<const f32x4 *>(p + 12 * g), *qv = reinterpret_cast<const f32x4 *>(q + 12 * g);
        const f32x4 p0 = pv[0], p1 = pv[1], p2 = pv[2], q0 = qv[0], q1 = qv[1], q2 = qv[2];
        const float pf[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        const float qf[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double px = pf[3 * a], py = pf[3 * a + 1], pz = pf[3 * a + 2];
            const double qx = qf[3 * a], qy = qf[3 * a + 1], qz = qf[3 * a + 2];
            H[0] = fma(px, qx, H[0]), H[1] = fma(px, qy, H[1]), H[2] = fma(px, qz, H[2]);
            H[3] = fma(py, qx, H[3]), H[4] = fma(py, qy, H[4]), H[5] = fma(py, qz, H[5]);
            H[6] = fma(pz, qx, H[6]), H[7] = fma(pz, qy, H[7]), H[8] = fma(pz, qz, H[8]);
        }
    }
    for (int off = lpp >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] += __shfl_xor(H[k], off);
    }
}

// Stage 1 of a pair that passed the screen: PAIR_DISSIMILAR / PAIR_SIMILAR / PAIR_UNDECIDED (pair_math.hpp).  With the float32 copy the tests
// run on H from that copy alone, with its own rounding bound; what they leave undecided goes to the explicit-rotation stage like any
// other undecided pair (it forms H from the float64 coordinates).  F32 = false: H from the float64 coordinates, as ever (a template
// parameter, not a branch: with both loops in one kernel the float64 one lost a tenth of its speed to the register allocation).
template <bool F32>
__device__ inline int pair_stage1(const double *__restrict__ heavy, const float *__restrict__ heavy32, int64_t i, int64_t j, int h, double half_sum,
                                  double half_h_thr2, double two_thr2, int sub, int lpp) {
    double H[9];
    if (F32) {
        const int pitch = heavy32_pitch(h);
        pair_H32(heavy32 + i * pitch, heavy32 + j * pitch, pitch / 12, sub, lpp, H);
        return pair_verdict_g(H, half_sum, half_h_thr2, two_thr2, quartic_gamma32(h));
    }
    pair_H(heavy + i * h * 3, heavy + j * h * 3, h, sub, lpp, H);
    return pair_verdict(H, half_sum, half_h_thr2, two_thr2, h);
}

// One pair end to end: true iff it is similar in the reference's sense (rmsd < thr and maxdev < 2 thr,
// rmsd_pruning.py:75); exact_taken tells whether the explicit-rotation path ran.
__device__ inline bool pair_is_similar(const double *__restrict__ p, const double *__restrict__ q, int h, double Gp, double Gq,
                                       double half_h_thr2, double thr, double maxdev_thr, bool &exact_taken, int sub, int lpp) {
    double H[9];
    pair_H(p, q, h, sub, lpp, H);
    exact_taken = false;
    if (certainly_dissimilar(H, 0.5 * (Gp + Gq) - half_h_thr2, 0.5 * (Gp + Gq), h)) return false;
    exact_taken = true;
    double rm, md;
    exact_rmsd_maxdev(p, q, h, H, Gp, Gq, rm, md, sub, lpp);
    return rm < thr && md < maxdev_thr;
}

}  // namespace tsc
