// cross.hpp -- cross-set RMSD: every query structure against every structure of a library, reduced per query row in one of three ways.
//
// A pair (query p, library q) is the reference's rmsd_and_max_numba(p, q) (tscode/rmsd_pruning.py:6-41): the optimal PROPER rotation of p
// onto q about the origin, rmsd = sqrt(sum |Rp - q|^2 / h), maxdev = max_a |Rp_a - q_a|; "similar" is rmsd < thr and maxdev < 2 thr (:75,
// :208-224).  The arithmetic is pair_math.hpp's (exact_quaternion, rmsd_and_max_pair, certainly_dissimilar); what is here is the rectangle:
//
//   k_cross_pack            (N, n, 3) structures -> the compared atoms row-major, zero-padded to the kernel's atom count (Xr), the same
//                           transposed [pitch][ld] (Xc, register path only), the squared norms G; centred on the compared atoms' mean
//                           when asked (the mean of a structure is a property of that structure alone: queries and library alike)
//   k_cross_tile<HP, EPI>   register path, h <= 32: a wavefront owns CX_ROWS query rows and one column segment of the library, a lane a
//                           library column whose HP x 3 coordinates sit in registers; H = p^T q by fma from the wavefront-uniform query row
//   k_cross_general<EPI>    any h: the same work items and epilogues, a pair per lane from the row-major packs (rmsd_and_max_pair)
//   k_cross_nearest_reduce  the `nearest` epilogue's second step (cross_reduce.hpp: only cross.hip launches it; leader.hip includes this header
//                           for the CX_FIRST rectangle alone)
//
// Epilogues:
//   CX_VALUES   every pair exactly; rmsd[q][l], maxdev[q][l] contiguous along l.  No screen.
//   CX_FIRST    certainly_dissimilar screens (a rejection is always right, pair_math.hpp), survivors take rmsd_and_max_pair; the lowest similar
//               library index of a row goes to first[q] by atomicMin (INT32_MAX: none).  A row is not visited by a segment once its
//               first lies left of that segment.  The minimum of a set does not depend on the order of the atomics.
//   CX_NEAREST  every pair exactly; per (segment, row) ONE wavefront walks the segment's columns in ascending order and writes the smallest
//               rmsd, its lowest index and the maxdev there to the partial arrays; k_cross_nearest_reduce takes the segments in ascending
//               order, a strictly smaller rmsd wins.  No floating-point atomic, nothing that depends on which wavefront arrives first:
//               two runs return identical bits.
#pragma once

#include "cross_plan.hpp"
#include "pair_math.hpp"

namespace tsc {

enum { CX_VALUES = 0, CX_FIRST = 1, CX_NEAREST = 2 };

// ---------------------------------------------------------------------------------------------------
// pack

struct CrossPackArgs {
    const double *src;      // [n][n_atoms][3]
    long long n;
    int n_atoms;
    const int32_t *idx;     // [h] compared atoms (device), or null: all atoms (h == n_atoms); an index outside 0 .. n_atoms - 1 reads as the origin
    int h, pitch;           // compared atoms; doubles per row of Xr (3 x padded atoms)
    int center;
    double *Xr;             // [n][pitch] or null (a library whose rows no epilogue reads: register path, values and nearest)
    double *Xc;             // [pitch][ld] or null
    long long ld;           // cross_ld(n)
    double *G;              // [ld]; zero behind n
};

// One workgroup = 64 structures, a wavefront takes 16 of them one after the other with its lanes on the atoms.  With Xc the rows also go
// through an LDS tile [64][pitch + 1] so that the transposed side is written 64 structures at a time (k_compact_coords' layout).
inline __global__ __launch_bounds__(256) void k_cross_pack(CrossPackArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_pack[];   // [64][pitch + 1] where a.Xc
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int lds_pitch = a.pitch + 1;
    const int h3 = 3 * a.h;
    for (long long s0 = (long long)blockIdx.x * 64; s0 < a.n; s0 += (long long)gridDim.x * 64) {
        for (int k = 0; k < 16; ++k) {
            const int rr = wid * 16 + k;
            const long long s = s0 + rr;
            if (s >= a.n) {   // (wavefront-uniform) the tail of the last tile: zeros on the transposed side and in the norms
                if (a.Xc)
                    for (int d = lane; d < a.pitch; d += 64) s_pack[rr * lds_pitch + d] = 0.0;
                if (lane == 0 && s < a.ld) a.G[s] = 0.0;
                continue;
            }
            const double *x = a.src + s * a.n_atoms * 3;
            double sx = 0.0, sy = 0.0, sz = 0.0;
            if (a.center) {
                for (int e = lane; e < a.h; e += 64) {
                    const int at = a.idx ? a.idx[e] : e;
                    if (at >= 0 && at < a.n_atoms) sx += x[3 * at], sy += x[3 * at + 1], sz += x[3 * at + 2];
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sx += __shfl_xor(sx, off), sy += __shfl_xor(sy, off), sz += __shfl_xor(sz, off);
                sx /= double(a.h), sy /= double(a.h), sz /= double(a.h);
            }
            double g = 0.0;
            for (int d = lane; d < a.pitch; d += 64) {
                double v = 0.0;
                if (d < h3) {
                    const int e = d / 3, c = d - 3 * e;
                    const int at = a.idx ? a.idx[e] : e;
                    if (at >= 0 && at < a.n_atoms) v = x[3 * at + c] - (c == 0 ? sx : (c == 1 ? sy : sz));
                }
                if (a.Xr) a.Xr[s * a.pitch + d] = v;
                if (a.Xc) s_pack[rr * lds_pitch + d] = v;
                g = fma(v, v, g);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) g += __shfl_xor(g, off);
            if (lane == 0) a.G[s] = g;
        }
        if (a.Xc) {
            __syncthreads();
            for (int e = threadIdx.x; e < 64 * a.pitch; e += 256) {
                const int d = e >> 6, rr = e & 63;
                a.Xc[(long long)d * a.ld + s0 + rr] = s_pack[rr * lds_pitch + d];   // s0 + 63 < ld: ld is a multiple of 64
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// the rectangle

struct CrossArgs {
    const double *Qr;       // [nq][pitch] query rows (this launch's first row at 0)
    const double *Qg;       // [nq]
    const double *Lr;       // [nl][pitch] library rows (general path; register path: CX_FIRST only, else null)
    const double *Lc;       // [pitch][ld] library columns (register path)
    const double *Lg;       // [ld]
    long long ld;
    long long nq, nl;       // rows of this launch, library structures
    long long n_tiles;      // ceil(nq / CX_ROWS)
    int h, pitch;
    int seg_cols;
    double thr, maxdev_thr, half_h_thr2;   // CX_FIRST
    double *rmsd, *maxdev;  // CX_VALUES: [nq][nl]; CX_NEAREST: partial [n_seg][nq]
    int32_t *idx;           // CX_FIRST: first[nq], INT32_MAX before the launch; CX_NEAREST: partial [n_seg][nq]
};

// residual_rmsd_maxdev (pair_math.hpp; rmsd_pruning.py:29-39) with the library structure in registers: the padded atoms are zero on both sides
// and add nothing to the sum or the maximum
template <int HP>
__device__ inline void cross_residual_regs(const double *__restrict__ p, const double (&q)[HP * 3], int h, const double e[4], double &rmsd, double &maxdev) {
    const double nn = 1.0 / sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    const double w = e[0] * nn, x = e[1] * nn, y = e[2] * nn, z = e[3] * nn;
    const double R00 = w * w + x * x - y * y - z * z, R01 = 2 * (x * y - w * z), R02 = 2 * (x * z + w * y);
    const double R10 = 2 * (x * y + w * z), R11 = w * w - x * x + y * y - z * z, R12 = 2 * (y * z - w * x);
    const double R20 = 2 * (x * z - w * y), R21 = 2 * (y * z + w * x), R22 = w * w - x * x - y * y + z * z;
    double ss = 0.0, mx = 0.0;
#pragma unroll
    for (int k = 0; k < HP; ++k) {
        const double px = p[3 * k], py = p[3 * k + 1], pz = p[3 * k + 2];
        const double dx = R00 * px + R01 * py + R02 * pz - q[3 * k];
        const double dy = R10 * px + R11 * py + R12 * pz - q[3 * k + 1];
        const double dz = R20 * px + R21 * py + R22 * pz - q[3 * k + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        ss += d2;
        mx = d2 > mx ? d2 : mx;
    }
    rmsd = sqrt(ss / double(h));
    maxdev = sqrt(mx);
}

// S = p^T q of rmsd_and_max_pair (rmsd_pruning.py:15) with the squared norms, for the general path's screen
__device__ inline void cross_pair_S(const double *__restrict__ p, const double *__restrict__ q, int h, double S[9], double &Gp, double &Gq) {
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
    Gp = Gq = 0.0;
    for (int a = 0; a < h; ++a) {
        const double px = p[3 * a], py = p[3 * a + 1], pz = p[3 * a + 2];
        const double qx = q[3 * a], qy = q[3 * a + 1], qz = q[3 * a + 2];
        S[0] = fma(px, qx, S[0]), S[1] = fma(px, qy, S[1]), S[2] = fma(px, qz, S[2]);
        S[3] = fma(py, qx, S[3]), S[4] = fma(py, qy, S[4]), S[5] = fma(py, qz, S[5]);
        S[6] = fma(pz, qx, S[6]), S[7] = fma(pz, qy, S[7]), S[8] = fma(pz, qz, S[8]);
        Gp += px * px + py * py + pz * pz;
        Gq += qx * qx + qy * qy + qz * qz;
    }
}

// CX_NEAREST, one row against one 64-column tile: the tile's smallest rmsd, the lowest column that has it and the maxdev there join the
// running best of the row, which lane t keeps for row t.  Lanes without a column come with rm = +inf.  Columns ascend from tile to tile, so
// only a strictly smaller rmsd replaces what the row has.
__device__ inline void cross_nearest_tile(int lane, int t, long long c0, double rm, double md, double &best_r, double &best_m, int &best_i) {
    double r = rm;
    int l = rm < INFINITY ? lane : 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ro = __shfl_xor(r, off);
        const int lo = __shfl_xor(l, off);
        const bool take = ro < r || (ro == r && lo < l);
        r = take ? ro : r, l = take ? lo : l;
    }
    const double m = __shfl(md, l & 63);
    if (lane == t && l < 64 && r < best_r) best_r = r, best_m = m, best_i = int(c0 + l);
}

// The rows of a work item that its segment still has to visit (CX_FIRST: those whose first does not lie left of the segment)
template <int EPI>
__device__ inline unsigned cross_live_rows(const CrossArgs &a, int lane, long long r0, int nrows, long long seg_lo) {
    if (EPI != CX_FIRST) return (1u << nrows) - 1u;
    int f = INT_MAX;
    if (lane < nrows) f = __hip_atomic_load(&a.idx[r0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return unsigned(__ballot(lane < nrows && (long long)f >= seg_lo));
}

// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the 3 HP doubles of the column and the explicit-rotation path together
// pass 256 VGPRs from HP = 16 on.  Held to two wavefronts per SIMD the compiler spills 76 .. 372 bytes per lane to scratch there; with one
// wavefront per SIMD it has the accumulation registers to spill to instead (18 .. 92 AGPRs, no scratch), which is what HP >= 16 is built for.
template <int HP>
constexpr int cx_waves_per_simd() { return HP <= 12 ? 2 : 1; }

template <int HP, int EPI>
inline __global__ __launch_bounds__(256, cx_waves_per_simd<HP>()) void k_cross_tile(CrossArgs a) {
    static_assert(CX_ROWS <= 16, "row liveness and the candidate bits are 32-bit masks with room to shift");
    constexpr int HP3 = HP * 3;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long seg_lo = (long long)blockIdx.y * a.seg_cols;
    const long long seg_hi = seg_lo + a.seg_cols < a.nl ? seg_lo + a.seg_cols : a.nl;
    for (long long tile = (long long)blockIdx.x * CX_WAVES + wid; tile < a.n_tiles; tile += (long long)gridDim.x * CX_WAVES) {
        const long long r0 = tile * CX_ROWS;
        const int nrows = int(a.nq - r0 < CX_ROWS ? a.nq - r0 : CX_ROWS);
        unsigned alive = cross_live_rows<EPI>(a, lane, r0, nrows, seg_lo);
        double best_r = INFINITY, best_m = INFINITY;
        int best_i = INT_MAX;
        for (long long c0 = seg_lo; c0 < seg_hi && alive; c0 += 64) {
            const long long col = c0 + lane;   // < ld: the packs are whole 64-column tiles
            const bool incol = col < a.nl;
            double q[HP3];
            {
                const double *xc = a.Lc + col;
#pragma unroll
                for (int d = 0; d < HP3; ++d, xc += a.ld) q[d] = *xc;
            }
            const double Gq = a.Lg[col];
            unsigned mycand = 0, candrows = 0;
            for (int t = 0; t < nrows; ++t) {
                if (!((alive >> t) & 1u)) continue;
                const long long r = r0 + t;
                const double *__restrict__ pr = a.Qr + r * HP3;
                double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < HP; ++k) {
                    const double px = pr[3 * k], py = pr[3 * k + 1], pz = pr[3 * k + 2];
                    H[0] = fma(px, q[3 * k], H[0]), H[1] = fma(px, q[3 * k + 1], H[1]), H[2] = fma(px, q[3 * k + 2], H[2]);
                    H[3] = fma(py, q[3 * k], H[3]), H[4] = fma(py, q[3 * k + 1], H[4]), H[5] = fma(py, q[3 * k + 2], H[5]);
                    H[6] = fma(pz, q[3 * k], H[6]), H[7] = fma(pz, q[3 * k + 1], H[7]), H[8] = fma(pz, q[3 * k + 2], H[8]);
                }
                const double Gp = a.Qg[r];
                if (EPI == CX_FIRST) {
                    const double half_sum = 0.5 * (Gp + Gq);
                    const bool cand = incol && !certainly_dissimilar(H, half_sum - a.half_h_thr2, half_sum, a.h);
                    if (__ballot(cand)) candrows |= 1u << t;
                    mycand |= cand ? (1u << t) : 0u;
                } else {
                    double rm = INFINITY, md = INFINITY;
                    if (incol) {
                        double e[4];
                        exact_quaternion(H, Gp, Gq, e);
                        cross_residual_regs<HP>(pr, q, a.h, e, rm, md);
                    }
                    if (EPI == CX_VALUES) {
                        if (incol) a.rmsd[r * a.nl + col] = rm, a.maxdev[r * a.nl + col] = md;
                    } else {
                        cross_nearest_tile(lane, t, c0, rm, md, best_r, best_m, best_i);
                    }
                }
            }
            while (candrows) {   // CX_FIRST: the survivors of this column tile take the explicit rotation
                const int t = __ffs(candrows) - 1;
                candrows &= candrows - 1;
                const long long r = r0 + t;
                bool sim = false;
                if ((mycand >> t) & 1u) {
                    double rm, md;
                    rmsd_and_max_pair(a.Qr + r * HP3, a.Lr + col * HP3, a.h, rm, md);
                    sim = rm < a.thr && md < a.maxdev_thr;   // rmsd_pruning.py:75
                }
                const unsigned long long sm = __ballot(sim);
                if (sm) {
                    if (lane == 0) atomicMin(&a.idx[r], int(c0 + __ffsll((long long)sm) - 1));
                    alive &= ~(1u << t);   // the tiles of a segment ascend: this is the segment's lowest
                }
            }
        }
        if (EPI == CX_NEAREST && lane < nrows) {
            const long long o = (long long)blockIdx.y * a.nq + r0 + lane;
            a.rmsd[o] = best_r, a.maxdev[o] = best_m, a.idx[o] = best_i;
        }
    }
}

// Any h >= 1: the same work items, a pair per lane from the row-major packs.  Every lane walks its own library row, `pitch` doubles apart
// from its neighbour's, once per query row of the item: the loads are neither coalesced nor kept -- what the register path exists to avoid.
template <int EPI>
inline __global__ __launch_bounds__(256) void k_cross_general(CrossArgs a) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long seg_lo = (long long)blockIdx.y * a.seg_cols;
    const long long seg_hi = seg_lo + a.seg_cols < a.nl ? seg_lo + a.seg_cols : a.nl;
    for (long long tile = (long long)blockIdx.x * CX_WAVES + wid; tile < a.n_tiles; tile += (long long)gridDim.x * CX_WAVES) {
        const long long r0 = tile * CX_ROWS;
        const int nrows = int(a.nq - r0 < CX_ROWS ? a.nq - r0 : CX_ROWS);
        unsigned alive = cross_live_rows<EPI>(a, lane, r0, nrows, seg_lo);
        double best_r = INFINITY, best_m = INFINITY;
        int best_i = INT_MAX;
        for (long long c0 = seg_lo; c0 < seg_hi && alive; c0 += 64) {
            const long long col = c0 + lane;
            const bool incol = col < a.nl;
            const double *__restrict__ ql = a.Lr + (incol ? col : 0) * a.pitch;
            for (int t = 0; t < nrows; ++t) {
                if (!((alive >> t) & 1u)) continue;
                const long long r = r0 + t;
                const double *__restrict__ pr = a.Qr + r * a.pitch;
                double rm = INFINITY, md = INFINITY;
                if (EPI == CX_FIRST) {
                    bool sim = false;
                    if (incol) {
                        double S[9], Gp, Gq;
                        cross_pair_S(pr, ql, a.h, S, Gp, Gq);
                        const double half_sum = 0.5 * (Gp + Gq);
                        if (!certainly_dissimilar(S, half_sum - a.half_h_thr2, half_sum, a.h)) {
                            exact_rmsd_maxdev(pr, ql, a.h, S, Gp, Gq, rm, md);
                            sim = rm < a.thr && md < a.maxdev_thr;   // rmsd_pruning.py:75
                        }
                    }
                    const unsigned long long sm = __ballot(sim);
                    if (sm) {
                        if (lane == 0) atomicMin(&a.idx[r], int(c0 + __ffsll((long long)sm) - 1));
                        alive &= ~(1u << t);
                    }
                } else {
                    if (incol) rmsd_and_max_pair(pr, ql, a.h, rm, md);
                    if (EPI == CX_VALUES) {
                        if (incol) a.rmsd[r * a.nl + col] = rm, a.maxdev[r * a.nl + col] = md;
                    } else {
                        cross_nearest_tile(lane, t, c0, rm, md, best_r, best_m, best_i);
                    }
                }
            }
        }
        if (EPI == CX_NEAREST && lane < nrows) {
            const long long o = (long long)blockIdx.y * a.nq + r0 + lane;
            a.rmsd[o] = best_r, a.maxdev[o] = best_m, a.idx[o] = best_i;
        }
    }
}

}  // namespace tsc
