// trimolecular.hpp -- the (conformers, pivots, orientation) groups of a THREE-molecule cyclical embed under RIGID, produced on the device:
// tscode/embeds.py:636-655 (the orientation loop) with _adjust_directions (:312-465) inside it.
//
// Per pivot triple the host has already taken every discrete decision (triangle test, exactly-right triangle and its nudge, obtuse-angle
// flips, which orientations the pairings leave: tscode_amd/embeds.py _trimolecular_prologue); what is left per orientation is arithmetic:
// three align_vec_pair, 21 rot_mat_from_pointer, 343 candidates of three vec_angle each and their argmin -- whose result, the new
// `directions`, is the INPUT of the next orientation (:650-655 rebinds it inside the loop).  So the eight orientations of a triple are a
// chain, and the triples are what runs side by side: one wavefront per triple, TG_WAVES of them per workgroup, grid-stride over triples.
// The wavefronts of a workgroup walk their triples in step, so the barriers between the phases are block barriers; a wavefront without
// a triple, or at an orientation its mask leaves out, idles through them (and leaves `directions` alone, as the loop's `continue` does).
//
// A NaN cost (a facing atom exactly on a triangle vertex: vec_angle of a zero vector) is outside the contract.  It never compares
// smaller, so it is never chosen; with all 343 costs NaN the group reports candidate 0 (NumPy's argmin reports the first NaN instead).
#pragma once
#include "common.hpp"
#include "csearch.hpp"

namespace tsc {

constexpr int TG_WAVES = 4;          // wavefronts (= triples in flight) per workgroup
constexpr int TG_MAX_ROWS = 8;       // rows of a molecule's reactive_cumnums table
constexpr int TG_CANDIDATES = 343;   // 7^3 turns of -30 .. 30 degrees in cartesian_product's order: the third molecule fastest, then the first (embeds.py:415-420)
constexpr int TG_RECORD = 23;        // start 0:3, end 3:6, direction 6:9, pivot 9:12, meanpoint 12:15, r0 15:18, r1 18:21, count 21, conformer 22

// What every triple shares: the three fragments inside `frags`, their reactive atoms and the (atom index, cumnum) tables.
struct TriTables {
    long long frag_off[3];  // doubles
    int n_atoms[3];
    int n_reactive[3];  // 1 or 2
    int reactive[3][2];
    int n_rows[3];
    int row_atom[3][TG_MAX_ROWS];
    long long row_cum[3][TG_MAX_ROWS];
};

// bit m of hex digit v: orientation v walks molecule m's pivot backwards (embeds.py:886-893: 000 001 010 011 100 110 101 111, molecule 0
// first) -- and, the same table, polygonize reverses the (start, end) pair of side m (utils.py:255)
constexpr unsigned TG_ORIENT = 0x75316240u;

// vec_angle (algebra.py:58-62) as _adjust_directions' cost reads it: both vectors normalised, dot, clipped, acos, degrees.  Products and
// sums are kept apart (no contraction) so that a candidate's cost is the host computation's up to the last bits of sqrt and acos.
__device__ inline double tg_vec_angle(const double u[3], const double w[3]) {
#pragma clang fp contract(off)
    const double nu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]), nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    double d = ((u[0] / nu) * (w[0] / nw) + (u[1] / nu) * (w[1] / nw)) + (u[2] / nu) * (w[2] / nw);
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);  // (a NaN stays a NaN)
    return acos(d) * (180.0 / 3.14159265358979323846);
}

struct TgWave {                 // one wavefront's LDS
    double R[3][9];             // align_vec_pair of every molecule, :368-369
    double pos[3][3];           // middle of the side - R @ meanpoint
    double p[3][3];             // end - start
    double pmean[3][3];         // (start + end) / 2
    double img[6][7][3];        // the facing point of (molecule, partner) pair k under turn j of its molecule
    int facing[3][3];           // facing[m][partner]: m's reactive atom that faces `partner` (:376-397); never set: atom 0
};

inline __global__ __launch_bounds__(64 * TG_WAVES) void k_trimolecular_groups(
    const double *__restrict__ frags, TriTables tb, const int32_t *__restrict__ conf, const double *__restrict__ pivot,
    const double *__restrict__ meanpoint, const int64_t *__restrict__ cum, const double *__restrict__ tri_poly, const double *__restrict__ tri_cost,
    const double *__restrict__ dir0, const uint8_t *__restrict__ mask, const int64_t *__restrict__ base, int64_t n_triples,
    double *__restrict__ blocks, int64_t *__restrict__ group_ids, int32_t *__restrict__ best_out) {
    __shared__ TgWave s_wave[TG_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    TgWave &S = s_wave[wid];
    for (int64_t t0 = int64_t(blockIdx.x) * TG_WAVES; t0 < n_triples; t0 += int64_t(gridDim.x) * TG_WAVES) {
        const int64_t t = t0 + wid;
        const bool have = t < n_triples;
        const unsigned bits = have ? mask[t] : 0u;
        const int m = lane < 3 ? lane : 0;  // the molecule of lanes 0 .. 2
        // lane m keeps molecule m's part of the triple, and its `directions[m]` from orientation to orientation
        double dir[3] = {0, 0, 0}, pv[3] = {0, 0, 0}, mp[3] = {0, 0, 0}, ra[3] = {0, 0, 0}, rb[3] = {0, 0, 0}, md[3] = {0, 0, 0};
        int cf = 0;
        if (have && bits && lane < 3) {
            cf = conf[3 * t + m];
            const double *c = frags + tb.frag_off[m] + int64_t(cf) * tb.n_atoms[m] * 3;
            bool zero = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                dir[i] = dir0[9 * t + 3 * m + i], pv[i] = pivot[9 * t + 3 * m + i], mp[i] = meanpoint[9 * t + 3 * m + i];
                ra[i] = c[3 * tb.reactive[m][0] + i];
                rb[i] = tb.n_reactive[m] == 2 ? c[3 * tb.reactive[m][1] + i] : ra[i];
                md[i] = mp[i] - (tb.n_reactive[m] == 2 ? (ra[i] + rb[i]) / 2.0 : ra[i]);  // meanpoint - mean(reactive atoms), conformer conf_ids[m]
                zero = zero && md[i] == 0.0;
            }
            if (zero) {
#pragma unroll
                for (int i = 0; i < 3; ++i) md[i] = mp[i];
            }
        }
        int rank = 0;
        for (int v = 0; v < 8; ++v) {
            const bool run = (bits >> v) & 1u;
            const unsigned rev = (TG_ORIENT >> (4 * v)) & 7u;
            double st[3] = {0, 0, 0}, en[3] = {0, 0, 0};
            int64_t ids[3][2] = {{0, 0}, {0, 0}, {0, 0}};
            if (run && lane < 3) {
                // the polygon side of molecule m: vertices m, m + 1, reversed where the orientation says so
                const int a = (rev >> m) & 1 ? (m + 1) % 3 : m, b = (rev >> m) & 1 ? m : (m + 1) % 3;
#pragma unroll
                for (int i = 0; i < 3; ++i) st[i] = tri_poly[9 * t + 3 * a + i], en[i] = tri_poly[9 * t + 3 * b + i];
                double p[3], pm[3], R[9];
#pragma unroll
                for (int i = 0; i < 3; ++i) p[i] = en[i] - st[i], pm[i] = (st[i] + en[i]) / 2.0;
                align_vec_pair_dev(p, dir, pv, md, R);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    S.pos[m][i] = pm[i] - (R[3 * i] * mp[0] + R[3 * i + 1] * mp[1] + R[3 * i + 2] * mp[2]);
                    S.p[m][i] = p[i], S.pmean[m][i] = pm[i];
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) S.R[m][i] = R[i];
            }
            if (run && (lane == 0 || lane == 3)) {
                // the cumnum pairs of the three contacts (:895-897) and, lane 3, who faces whom: the reference's scan, the last match wins
                int64_t c3[3][2];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int64_t c0 = cum[6 * t + 2 * q], c1 = cum[6 * t + 2 * q + 1];
                    c3[q][0] = (rev >> q) & 1 ? c1 : c0, c3[q][1] = (rev >> q) & 1 ? c0 : c1;
                }
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int64_t x = c3[q][1], y = c3[(q + 1) % 3][0];
                    ids[q][0] = x < y ? x : y, ids[q][1] = x < y ? y : x;
                }
                if (lane == 3) {
                    for (int i = 0; i < 9; ++i) S.facing[i / 3][i % 3] = 0;
                    for (int q = 0; q < 3; ++q) {
                        int m0 = 0, i0 = 0, m1 = 0, i1 = 0;
                        for (int mm = 0; mm < 3; ++mm)
                            for (int r = 0; r < tb.n_rows[mm]; ++r) {
                                if (tb.row_cum[mm][r] == ids[q][0]) m0 = mm, i0 = tb.row_atom[mm][r];
                                if (tb.row_cum[mm][r] == ids[q][1]) m1 = mm, i1 = tb.row_atom[mm][r];
                            }
                        S.facing[m0][m1] = i0;
                        S.facing[m1][m0] = i1;
                    }
                }
            }
            __syncthreads();
            if (run && lane < 42) {
                // facing point of pair k = (molecule, partner) in the order (0,1) (0,2) (1,0) (1,2) (2,0) (2,1), turned by -30 + 10 j degrees about
                // its molecule's side.  Conformer 0, as the reference (:403-411).
                const int k = lane / 7, j = lane - 7 * k;
                const int mol = k >> 1, partner = (k & 1) ? (mol == 2 ? 1 : 2) : (mol == 0 ? 1 : 0);
                const double *x = frags + tb.frag_off[mol] + 3 * int64_t(S.facing[mol][partner]);
                double at[3], ax[3], T[9];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    at[i] = S.R[mol][3 * i] * x[0] + S.R[mol][3 * i + 1] * x[1] + S.R[mol][3 * i + 2] * x[2] + S.pos[mol][i];
                    ax[i] = S.p[mol][i];
                }
                rot_mat_from_pointer_dev(ax, -30.0 + 10.0 * j, T);
#pragma unroll
                for (int i = 0; i < 3; ++i) S.img[k][j][i] = T[3 * i] * at[0] + T[3 * i + 1] * at[1] + T[3 * i + 2] * at[2];
            }
            __syncthreads();
            if (run) {
                double tv[3][3];
#pragma unroll
                for (int i = 0; i < 9; ++i) tv[i / 3][i % 3] = tri_cost[9 * t + i];
                double best_cost = INFINITY;
                int best = TG_CANDIDATES;
                for (int cand = lane; cand < TG_CANDIDATES; cand += 64) {
                    const int i1 = cand / 49, i0 = (cand / 7) % 7, i2 = cand % 7;  // (meshgrid's order: the second molecule slowest)
                    // cost = vec_angle(v0 - n02, n20 - v0) + vec_angle(v1 - n01, n10 - v1) + vec_angle(v2 - n21, n12 - v2), :441-444
                    const double *n01 = S.img[0][i0], *n02 = S.img[1][i0], *n10 = S.img[2][i1], *n12 = S.img[3][i1], *n20 = S.img[4][i2], *n21 = S.img[5][i2];
                    double u[3], w[3], cost;
#pragma unroll
                    for (int i = 0; i < 3; ++i) u[i] = tv[0][i] - n02[i], w[i] = n20[i] - tv[0][i];
                    cost = tg_vec_angle(u, w);
#pragma unroll
                    for (int i = 0; i < 3; ++i) u[i] = tv[1][i] - n01[i], w[i] = n10[i] - tv[1][i];
                    cost = cost + tg_vec_angle(u, w);
#pragma unroll
                    for (int i = 0; i < 3; ++i) u[i] = tv[2][i] - n21[i], w[i] = n12[i] - tv[2][i];
                    cost = cost + tg_vec_angle(u, w);
                    if (cost < best_cost) best_cost = cost, best = cand;  // (strict: a lane's candidates come in ascending order)
                }
                // the smallest cost of the wavefront, the lower index on equal cost: the first of the smallest
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double oc = __shfl_xor(best_cost, off, 64);
                    const int ob = __shfl_xor(best, off, 64);
                    if (oc < best_cost || (oc == best_cost && ob < best)) best_cost = oc, best = ob;
                }
                if (best >= TG_CANDIDATES) best = 0;  // every cost a NaN
                const int64_t slot = base[t] + rank;
                if (lane < 3) {
                    const int im = m == 1 ? best / 49 : (m == 0 ? (best / 7) % 7 : best % 7);
                    double *rec = blocks + (slot * 3 + m) * TG_RECORD;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        dir[i] = S.pmean[m][i] - (S.img[2 * m][im][i] + S.img[2 * m + 1][im][i]) / 2.0;
                        rec[i] = st[i], rec[3 + i] = en[i], rec[6 + i] = dir[i], rec[9 + i] = pv[i], rec[12 + i] = mp[i];
                        rec[15 + i] = ra[i], rec[18 + i] = rb[i];
                    }
                    rec[21] = double(tb.n_reactive[m]), rec[22] = double(cf);
                }
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) group_ids[slot * 6 + 2 * q] = ids[q][0], group_ids[slot * 6 + 2 * q + 1] = ids[q][1];
                    best_out[slot] = best;
                }
                ++rank;
            }
            // (no barrier here: what the next orientation's first phase writes -- R, pos, p, pmean, facing -- was last read before the
            // barrier above, and img, read just now, is written again only behind the next one)
        }
    }
}

}  // namespace tsc
