// tfd.hpp -- SURVEY.md 8(f) N2: torsion fingerprints and the pair search of prune_conformers_tfd.
//
// tscode/numba_functions.py:142-231.  The fingerprint of a structure is the float32 vector of its dihedral angles over a
// list of atom quadruplets (:255-264, algebra.py:24-55); two structures are similar when the wrapped absolute differences
// sum to less than `thresh` degrees (:242-253).  A pass cuts the structure list into k chunks and, inside a chunk, every
// row i looks for the first j > i that is similar (:181-199).  Rows are independent and the reference's cache only skips
// pairs already found dissimilar (it cannot change a verdict), so a pass is one launch: one wavefront per row, 64 columns
// per step, ballot for the first hit.  What happens to the matches (networkx components, "first of the cluster") stays on
// the host, with the reference's own Python objects (tscode_amd/numba_functions.py).
//
// No kernel here: the device functions.  The kernels of one ensemble and of the greedy filter are in tfd_kernels.hpp, those that take
// many ensembles per launch in tfd_batch.hpp.
#pragma once
#include "common.hpp"

namespace tsc {

// algebra.py:24-55 in fp64, result in degrees; fp contraction off: the fixture values were produced without FMA and the
// result is rounded to float32 right after
__device__ inline double dihedral_deg_dev(const double *__restrict__ p0, const double *__restrict__ p1, const double *__restrict__ p2,
                                          const double *__restrict__ p3) {
#pragma clang fp contract(off)
    double b0[3], b1[3], b2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) b0[k] = -1.0 * (p1[k] - p0[k]), b1[k] = p2[k] - p1[k], b2[k] = p3[k] - p2[k];
    const double n1 = sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) b1[k] /= n1;
    const double d0 = b0[0] * b1[0] + b0[1] * b1[1] + b0[2] * b1[2], d2 = b2[0] * b1[0] + b2[1] * b1[1] + b2[2] * b1[2];
    double v[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = b0[k] - d0 * b1[k], w[k] = b2[k] - d2 * b1[k];
    const double x = v[0] * w[0] + v[1] * w[1] + v[2] * w[2];
    const double c0 = b1[1] * v[2] - b1[2] * v[1], c1 = b1[2] * v[0] - b1[0] * v[2], c2 = b1[0] * v[1] - b1[1] * v[0];
    const double y = c0 * w[0] + c1 * w[1] + c2 * w[2];
    return atan2(y, x) * (180.0 / 3.14159265358979323846);
}

// One element of _get_tf_mat (:233-240): torsion t of the structure c[n][3].  The plain and the segmented kernel both call this, so a
// fingerprint cannot differ between the two routes.
__device__ inline float tfd_fingerprint_element(const double *__restrict__ c, const int32_t *__restrict__ quads, int t) {
    const int32_t *q = quads + 4 * t;
    return float(dihedral_deg_dev(c + 3 * q[0], c + 3 * q[1], c + 3 * q[2], c + 3 * q[3]));
}

// Row i of one pass of the pair search (:171-199), by one wavefront: the absolute index of the first similar j > i inside i's chunk,
// -1 if none or if i lies in no chunk (the last chunk ends at num_active, :175-178).  The same value in every lane.  The plain and
// the segmented kernel both call this, so a verdict cannot differ between the two routes.
__device__ inline int32_t tfd_first_similar_row(const float *__restrict__ tf, int T, int64_t i, int64_t d, int64_t k, int64_t num_active, double thresh,
                                                int lane) {
    int64_t step = i / d;
    if (step > k - 1) step = k - 1;
    const int64_t start = d * step;
    int64_t len = (step == k - 1) ? num_active - start : d;
    if (len < 0) len = 0;
    const int64_t i_rel = i - start;
    int32_t found = -1;
    if (i_rel < len) {
        const float *a = tf + i * T;
        for (int64_t j0 = i_rel + 1; j0 < len && found < 0; j0 += 64) {
            const int64_t j = j0 + lane;
            bool sim = false;
            if (j < len) {
                const float *b = tf + (start + j) * T;
                double sum = 0.0;
                for (int t = 0; t < T; ++t) {
                    const float d32 = fabsf(a[t] - b[t]);          // float32, like the reference's arrays
                    double dd = double(d32);
                    if (d32 > 180.0f) dd -= 360.0;                  // the integer term makes the rest float64
                    sum += fabs(dd);
                }
                sim = sum < thresh;
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(sim);
            if (m) found = int32_t(start + j0 + (__ffsll((long long)m) - 1));
        }
    }
    return found;
}

// ---- many ensembles per launch (tfd_batch.hpp, refine_batch.hpp): a row or element finds its segment in a table ----------------------
// the last entry q of table[0 .. count) with key(q) <= v; table[0]'s key is <= v.  Entries of equal key: the last one, which is the
// one that is not empty.
template <typename Entry, typename Key>
__device__ inline int tfd_last_not_above(const Entry *__restrict__ table, int count, int64_t v, Key key) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(table[mid]) <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// tfd_similarity (:242-253) of two fingerprints: float32 difference, float64 after the wrap, summed in order
__device__ inline bool tfd_similar_dev(const float *__restrict__ a, const float *__restrict__ b, int T, double thresh) {
    double sum = 0.0;
    for (int t = 0; t < T; ++t) {
        const float d32 = fabsf(a[t] - b[t]);
        double dd = double(d32);
        if (d32 > 180.0f) dd -= 360.0;
        sum += fabs(dd);
    }
    return sum < thresh;
}

// is_new_structure of the string embed (tscode/embeds.py:47-69) over a whole ordered list: structure s is kept iff its
// fingerprint is not tfd-similar to the fingerprint of any structure KEPT before it.  The reference's "LRU" never evicts
// (`lru_cache = lru_cache[1:]` rebinds a local name, :66-67), so every kept fingerprint is compared for ever.
// The filter is sequential by definition, but nearly all of its work is not: the list is walked in super-blocks of TG_SUPER
// candidates, and per super-block
//   k_tfd_greedy_prior   (whole GPU) marks the candidates that are similar to a structure kept in an EARLIER super-block
//                        (candidates x slices of a compact copy of the kept fingerprints; a lane stops at its first hit);
//   k_tfd_greedy_pairs   (whole GPU) every pair INSIDE the super-block, whatever the greedy order will make of it: row c of a
//                        TG_SUPER x TG_SUPER bit matrix = the earlier candidates of the super-block c is similar to;
//   k_tfd_greedy_replay  (one wavefront) the greedy order itself, which is all that is sequential: lane l holds the kept bits of
//                        candidates 64 l .. 64 l + 63; a candidate is kept iff the prior pass left it alive and its row meets no
//                        kept bit.  Per block of 64 candidates the rows are in registers (the next block's already in flight),
//                        the test against the blocks before is 64 independent ballots, and what remains serial is a scalar
//                        chain over the block's own 64 x 64 corner.
// 100 000 fingerprints with 12 000 kept: 1.07 s in a single-workgroup kernel over the whole list, 45 ms with the verdicts of a
// super-block walked by one workgroup (round 2), a few milliseconds this way.
// kept_list i32[N] (device scratch) ends up holding the kept indices in order; *n_kept their number (zeroed by the caller).
constexpr int TG_SUPER = 4096;
constexpr int TG_WORDS = TG_SUPER / 64;
constexpr int TG_REG_T = 8;         // fingerprints up to this length sit in registers and are screened in fp32 first
static_assert(TG_WORDS == 64, "k_tfd_greedy_replay: one lane per word of the kept mask");

// tfd_similar_dev with the candidate's fingerprint in registers and a float32 screen in front: min(d, |360 - d|) is the
// reference's wrapped difference (d <= 180: itself; d > 180: |d - 360|), summed in float32 it is off by at most
// T (2^-16 + 2^-23 sum) -- 2^-16 for the rounding of 360 - d, the rest for the additions -- so a sum outside [lo32, hi32] has the
// verdict of the float64 sum; inside (or NaN) the float64 sum decides.  Longer fingerprints take the float64 sum directly.
struct TfdScreen {
    float lo32, hi32;
};
__device__ inline TfdScreen tfd_screen(int T, double thresh) {
    const double abs_err = T * 3.1e-5, rel = T * 2.4e-7;
    TfdScreen sc;
    sc.lo32 = float((thresh - abs_err) * (1.0 - rel) - 1e-6 * fabs(thresh));
    sc.hi32 = float((thresh + abs_err) / (1.0 - rel) + 1e-6 * fabs(thresh));
    return sc;
}
__device__ inline void tfd_load_reg(const float *__restrict__ a, int T, float (&ar)[TG_REG_T]) {
#pragma unroll
    for (int t = 0; t < TG_REG_T; ++t) ar[t] = t < T ? a[t] : 0.0f;
}
__device__ inline bool tfd_similar_reg(const float *__restrict__ a, const float (&ar)[TG_REG_T], const float *__restrict__ b, int T, double thresh,
                                       const TfdScreen sc) {
    if (T <= TG_REG_T) {
        float s32 = 0.0f;
#pragma unroll
        for (int t = 0; t < TG_REG_T; ++t)
            if (t < T) {
                const float d = fabsf(ar[t] - b[t]);
                s32 += fminf(d, fabsf(360.0f - d));
            }
        if (s32 < sc.lo32) return true;
        if (s32 > sc.hi32) return false;
    }
    return tfd_similar_dev(a, b, T, thresh);
}

__device__ inline unsigned long long readlane64(unsigned long long v, int l) {
    const unsigned lo = __builtin_amdgcn_readlane(unsigned(v), l), hi = __builtin_amdgcn_readlane(unsigned(v >> 32), l);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

}  // namespace tsc
