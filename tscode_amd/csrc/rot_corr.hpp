// rot_corr.hpp -- the symmetry-corrected RMSD prune: tscode/torsion_module.py:953-1161 (rotationally_corrected_rmsd and
// prune_conformers_rmsd_rot_corr).
//
// A pair (i, j) compares ref = S[i] with coord = S[j]: for every dummy torsion t in order, each of its angles is tried by
// rotating S[j]'s moving atoms in place (utils.py:389-414, about the current t1 - t2 bond), taking the Kabsch RMSD of t's local
// heavy subgraph (no centring, ref rotated onto coord) and rotating back; the first angle with a strictly smaller value wins.
// Then every torsion's best angle is applied in place, in order, and the pair's value is the Kabsch RMSD over all heavy atoms.
// S[j] keeps the turns (and the round-off of every rotate / rotate-back) after the call, so rows of a chunk are sequential: the
// reference evaluates j = i+1, i+2, ... of row i on the structures as the earlier rows left them and stops at the first similar j.
//
// One workgroup owns one chunk of a pass and walks its rows in order.  A wavefront owns one j at a time: S[j] is copied into the
// wave's LDS block, turned there (lanes are atoms) and measured; the j of a row are taken nw at a time in index order, and after
// each batch the workgroup reduces to the first similar j* of the batch (LDS atomicMin).  Then the waves whose j <= j* commit --
// the turned coordinates go back to S[j], a dissimilar pair sets its cache bit -- and the row ends at j*; the turns of the
// j > j* evaluated in the same batch are dropped, as the reference never computes them.  Workgroups share nothing: chunks are
// disjoint, and the cache bits of a row sit in whole 32-bit words of that row.
//
// The Kabsch step is the exact path of pair_math.hpp (Horn's quaternion: Newton + adjugate, Jacobi when that degenerates) on the
// 3x3 correlation S = ref_sub^T coord_sub reduced across the wave; the quaternion rotation of rot_mat_from_pointer_dev
// (csearch.hpp) turns the atoms.
//
// No kernel here: arguments, device functions and the host's check of a set-up.  k_rot_corr_pass and k_rot_corr_pairs are in
// rot_corr_kernels.hpp, k_rot_corr_pass_seg (many ensembles per launch) in refine_batch.hpp.
#pragma once
#include "common.hpp"
#include "csearch.hpp"
#include "pair_math.hpp"

namespace tsc {

constexpr int RC_MAX_TORS = 16, RC_MAX_ATOMS = 512, RC_MAX_ANGLES = 6, RC_WAVES = 8;

struct RotCorrArgs {
    int n;                     // atoms per structure
    int h;                     // heavy atoms
    int n_tors;
    const int32_t *heavy;      // [h]
    const int32_t *tors;       // [n_tors][4]
    const double *angles;      // [n_tors][RC_MAX_ANGLES], degrees
    const int32_t *n_angles;   // [n_tors]
    const uint8_t *masks;      // [n_tors][n]: the atoms the torsion turns (_get_rotation_mask)
    const int32_t *sub_ptr;    // [n_tors + 1]
    const int32_t *sub_idx;    // torsion t's local heavy subgraph: sub_idx[sub_ptr[t] .. sub_ptr[t+1])
};

// LDS of one wavefront: the structure being turned (fp64) and the torsions' best angles
__host__ __device__ inline size_t rot_corr_wave_bytes(int n) { return (size_t(n) * 3 + RC_MAX_TORS) * sizeof(double); }
__host__ __device__ inline size_t rot_corr_lds_bytes(int n_tors, int n, int waves) {
    return torsion_lists_bytes(n_tors, n) + size_t(waves) * rot_corr_wave_bytes(n) + 16;
}

// kabsch_rmsd(ref[idx], c[idx]) over m atoms: lanes take atoms lane, lane + 64, ...; the sums reduce with an xor butterfly, so
// every lane holds bit-identical values and the result is wave-uniform.
__device__ inline double kabsch_rmsd_idx(const double *__restrict__ ref, const double *c, const int32_t *__restrict__ idx, int m, int lane) {
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Gp = 0.0, Gq = 0.0;
    for (int r = lane; r < m; r += 64) {
        const int a = idx[r];
        const double px = ref[3 * a], py = ref[3 * a + 1], pz = ref[3 * a + 2];
        const double qx = c[3 * a], qy = c[3 * a + 1], qz = c[3 * a + 2];
        S[0] += px * qx, S[1] += px * qy, S[2] += px * qz;
        S[3] += py * qx, S[4] += py * qy, S[5] += py * qz;
        S[6] += pz * qx, S[7] += pz * qy, S[8] += pz * qz;
        Gp += px * px + py * py + pz * pz;
        Gq += qx * qx + qy * qy + qz * qz;
    }
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int e = 0; e < 9; ++e) S[e] += __shfl_xor(S[e], off);
        Gp += __shfl_xor(Gp, off);
        Gq += __shfl_xor(Gq, off);
    }
    double e[4];
    exact_quaternion(S, Gp, Gq, e);
    const double nn = 1.0 / sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    const double w = e[0] * nn, x = e[1] * nn, y = e[2] * nn, z = e[3] * nn;
    const double R00 = w * w + x * x - y * y - z * z, R01 = 2 * (x * y - w * z), R02 = 2 * (x * z + w * y);
    const double R10 = 2 * (x * y + w * z), R11 = w * w - x * x + y * y - z * z, R12 = 2 * (y * z - w * x);
    const double R20 = 2 * (x * z - w * y), R21 = 2 * (y * z + w * x), R22 = w * w - x * x - y * y + z * z;
    double ss = 0.0;
    for (int r = lane; r < m; r += 64) {
        const int a = idx[r];
        const double px = ref[3 * a], py = ref[3 * a + 1], pz = ref[3 * a + 2];
        const double dx = R00 * px + R01 * py + R02 * pz - c[3 * a];
        const double dy = R10 * px + R11 * py + R12 * pz - c[3 * a + 1];
        const double dz = R20 * px + R21 * py + R22 * pz - c[3 * a + 2];
        ss += dx * dx + dy * dy + dz * dz;
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    return sqrt(ss / double(m));
}

// rotationally_corrected_rmsd (torsion_module.py:953-1007) on the structure c (LDS, turned in place) against ref (global).
// best: the wave's RC_MAX_TORS doubles of LDS, left holding the best angle of every torsion.  Returns the heavy-atom RMSD.
__device__ inline double rot_corr_pair(const RotCorrArgs &a, const TorsionLists &L, const double *__restrict__ ref, double *c, double *best,
                                       int lane) {
    for (int t = 0; t < a.n_tors; ++t) {
        const int i2 = a.tors[4 * t + 1], i3 = a.tors[4 * t + 2], nm = L.count[4 * t], na = a.n_angles[t];
        const uint16_t *moved = L.moved + size_t(t) * a.n;
        const int32_t *idx = a.sub_idx + a.sub_ptr[t];
        const int m = a.sub_ptr[t + 1] - a.sub_ptr[t];
        double best_rmsd = 1e10, best_angle = 0.0;          // (:981, torsion_corrections = 0)
        for (int q = 0; q < na; ++q) {                      // :984-1005
            const double ang = a.angles[RC_MAX_ANGLES * t + q];
            rotate_dihedral_lds(c, i2, i3, ang, moved, nm, lane);
            const double r = kabsch_rmsd_idx(ref, c, idx, m, lane);
            if (r < best_rmsd) best_rmsd = r, best_angle = ang;
            rotate_dihedral_lds(c, i2, i3, -ang, moved, nm, lane);
        }
        if (lane == 0) best[t] = best_angle;
    }
    __builtin_amdgcn_wave_barrier();
    for (int t = 0; t < a.n_tors; ++t)                      // :1010-1014, each about the current axis
        rotate_dihedral_lds(c, a.tors[4 * t + 1], a.tors[4 * t + 2], best[t], L.moved + size_t(t) * a.n, L.count[4 * t], lane);
    return kabsch_rmsd_idx(ref, c, a.heavy, a.h, lane);     // :1017
}

__device__ inline bool cache_bit(const uint32_t *cache, int64_t words, int64_t i, int64_t j) {
    return (cache[i * words + (j >> 5)] >> (j & 31)) & 1u;
}

// The rows of one chunk [lo, hi) of a pass (:1097-1125), in order, by one workgroup: coords, cache (rows of `words` 32-bit words) and
// first are ONE ensemble's; lds is the workgroup's dynamic LDS, laid out here from a.n_tors and a.n (rot_corr_lds_bytes of them is the
// least it may be).  first[i] = the first j of row i that is similar (rmsd < thr), or -1; *evaluated grows by the pairs evaluated.
// k_rot_corr_pass and k_rot_corr_pass_seg both call this, so a turned structure cannot differ between the two routes.
__device__ inline void rot_corr_chunk(const RotCorrArgs &a, double *__restrict__ coords, uint32_t *__restrict__ cache, int64_t words,
                                      int32_t *__restrict__ first, int64_t lo, int64_t hi, double thr, unsigned char *lds,
                                      unsigned long long *__restrict__ evaluated) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, n = a.n;
    const TorsionLists L = torsion_lists_at(lds, a.n_tors, n);
    build_torsion_lists(L, a.masks, a.tors, a.n_tors, n);
    double *c = reinterpret_cast<double *>(lds + torsion_lists_bytes(a.n_tors, n) + size_t(wid) * rot_corr_wave_bytes(n));
    double *best = c + size_t(n) * 3;
    int *s_first = reinterpret_cast<int *>(lds + torsion_lists_bytes(a.n_tors, n) + size_t(nw) * rot_corr_wave_bytes(n));
    unsigned *s_count = reinterpret_cast<unsigned *>(s_first + 1);
    if (threadIdx.x == 0) *s_count = 0;
    for (int64_t i = lo; i < hi; ++i) {
        if (threadIdx.x == 0) *s_first = INT_MAX;
        __syncthreads();
        const double *ref = coords + i * n * 3;
        int js = INT_MAX;
        for (int64_t jb = i + 1; jb < hi; jb += nw) {
            const int64_t j = jb + wid;
            const bool active = j < hi && !cache_bit(cache, words, i, j);   // :1106 cached pairs were dissimilar: skipped
            bool similar = false;
            if (active) {
                const double *src = coords + j * n * 3;
                for (int e = lane; e < n * 3; e += 64) c[e] = src[e];
                __builtin_amdgcn_wave_barrier();
                similar = rot_corr_pair(a, L, ref, c, best, lane) < thr;     // :1111-1118
                if (similar && lane == 0) atomicMin(s_first, int(j));
            }
            __syncthreads();
            js = *s_first;
            if (active && j <= js) {                        // what the reference computed before its `break` (:1119)
                double *dst = coords + j * n * 3;
                for (int e = lane; e < n * 3; e += 64) dst[e] = c[e];
                if (lane == 0) {
                    if (!similar) atomicOr(&cache[i * words + (j >> 5)], 1u << (j & 31));   // :1121-1123
                    atomicAdd(s_count, 1u);
                }
            }
            __syncthreads();                                // S[j] written before any wave reads it; the LDS blocks free again
            if (js != INT_MAX) break;
        }
        if (threadIdx.x == 0) first[i] = js == INT_MAX ? -1 : js;
    }
    __syncthreads();
    if (threadIdx.x == 0 && *s_count) atomicAdd(evaluated, (unsigned long long)*s_count);
}

// the limits of the ABI (include/tscode_hip.h), checked on the host arrays before anything touches the device (rot_corr.hip, and per
// segment in refine_batch.hip)
inline int rot_corr_check_setup(int64_t N, int n, const int32_t *heavy, int h, const int32_t *tors, int T, const double *angles, const int32_t *n_angles,
                                const uint8_t *mask, const int32_t *sub_ptr, const int32_t *sub_idx) {
    TSC_REQUIRE(heavy && (T == 0 || (tors && angles && n_angles && mask)) && sub_ptr && (T == 0 || sub_idx), "rot_corr: null argument");
    TSC_REQUIRE(N >= 0 && N < INT32_MAX, "rot_corr: %lld structures (at most %d)", (long long)N, INT32_MAX - 1);
    TSC_REQUIRE(n >= 1 && n <= RC_MAX_ATOMS, "rot_corr: %d atoms per structure (1 .. %d)", n, RC_MAX_ATOMS);
    TSC_REQUIRE(T >= 0 && T <= RC_MAX_TORS, "rot_corr: %d torsions (0 .. %d)", T, RC_MAX_TORS);
    TSC_REQUIRE(h >= 1 && h <= n, "rot_corr: %d heavy atoms of %d", h, n);
    for (int q = 0; q < h; ++q) TSC_REQUIRE(heavy[q] >= 0 && heavy[q] < n, "rot_corr: heavy atom index %d out of range", heavy[q]);
    TSC_REQUIRE(sub_ptr[0] == 0, "rot_corr: sub_ptr[0] must be 0");
    for (int t = 0; t < T; ++t) {
        for (int q = 0; q < 4; ++q) TSC_REQUIRE(tors[4 * t + q] >= 0 && tors[4 * t + q] < n, "rot_corr: torsion %d: atom index out of range", t);
        TSC_REQUIRE(n_angles[t] >= 1 && n_angles[t] <= RC_MAX_ANGLES, "rot_corr: torsion %d: %d angles (1 .. %d)", t, n_angles[t], RC_MAX_ANGLES);
        for (int q = 0; q < n_angles[t]; ++q) TSC_REQUIRE(std::isfinite(angles[RC_MAX_ANGLES * t + q]), "rot_corr: torsion %d: angle not finite", t);
        TSC_REQUIRE(sub_ptr[t + 1] > sub_ptr[t] && sub_ptr[t + 1] - sub_ptr[t] <= n, "rot_corr: torsion %d: local subgraph of %d atoms", t,
                    sub_ptr[t + 1] - sub_ptr[t]);
        for (int q = sub_ptr[t]; q < sub_ptr[t + 1]; ++q) TSC_REQUIRE(sub_idx[q] >= 0 && sub_idx[q] < n, "rot_corr: subgraph index out of range");
    }
    return 0;
}

}  // namespace tsc
