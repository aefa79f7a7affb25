// embed_transform.hpp -- K1, the batched rigid-body embedding kernel (the device functions it calls: embed_clash.hpp).
// Included only by the units that launch k_transform: embed.hip, adjacent.hip, pipeline.hip.
#pragma once
#include "embed_clash.hpp"

namespace tsc {

// K1: a workgroup embeds TR_POSES poses at a time: their rotations, translations and conformer indices go to LDS first,
// then one thread per (pose, atom); consecutive threads write consecutive 24-byte triples.
// idx (optional): only the listed poses are embedded, out row r <- pose idx[r] (used after the clash
// filter); heavy_sel/heavy_out (optional): additionally write the heavy-atom subset of each pose.
inline __global__ __launch_bounds__(256) void k_transform(const double *__restrict__ frags, FragTable ft,
                                                    const int32_t *__restrict__ conf_idx, const double *__restrict__ rot,
                                                    const double *__restrict__ pos, const int32_t *__restrict__ idx,
                                                    int64_t n_out, double *__restrict__ out,
                                                    const int32_t *__restrict__ heavy_slot, int n_heavy,
                                                    double *__restrict__ heavy_out, const int32_t *__restrict__ n_out_dev,
                                                    double *__restrict__ zero_me = nullptr, int n_zero = 0) {
    // n_out_dev (optional): the row count lives on the device (the total of the scan that made idx); the grid is then
    // sized for an upper bound and the host need not wait for the count before launching
    // zero_me (optional): n_zero doubles cleared on the way (the moment accumulators of the basis estimate that follows
    // the sample embed: a memset in that short chain is two more launches)
    extern __shared__ __attribute__((aligned(16))) double s_tr[];
    const int n = ft.n_total, nm = ft.n_mols, tid = threadIdx.x;
    for (int e = blockIdx.x * 256 + tid; e < n_zero; e += gridDim.x * 256) zero_me[e] = 0.0;
    if (n_out_dev) n_out = *n_out_dev;
    int64_t *sP = reinterpret_cast<int64_t *>(s_tr);  // pose of every local row
    double *sR = s_tr + TR_POSES, *sT = sR + TR_POSES * nm * 9;
    int *sC = reinterpret_cast<int *>(sT + TR_POSES * nm * 3);
    for (int64_t r0 = int64_t(blockIdx.x) * TR_POSES; r0 < n_out; r0 += int64_t(gridDim.x) * TR_POSES) {
        const int np = int(min<int64_t>(TR_POSES, n_out - r0));
        if (tid < np) sP[tid] = idx ? int64_t(idx[r0 + tid]) : r0 + tid;
        __syncthreads();
        for (int q = tid; q < np * nm * 9; q += 256) {
            const int row = q / (nm * 9), w = q - row * nm * 9;
            sR[q] = rot[sP[row] * nm * 9 + w];
        }
        for (int q = tid; q < np * nm * 3; q += 256) {
            const int row = q / (nm * 3), w = q - row * nm * 3;
            sT[q] = pos[sP[row] * nm * 3 + w];
        }
        for (int q = tid; q < np * nm; q += 256) {
            const int row = q / nm, w = q - row * nm;
            sC[q] = conf_idx[sP[row] * nm + w];
        }
        __syncthreads();
        for (int e = tid; e < np * n; e += 256) {
            const int row = e / n, a = e - row * n;
            const int64_t r = r0 + row;
            double v[3];
            embed_atom_staged(frags, ft, sR, sT, sC, row, a, v);
            if (out) {
                double *o = out + (r * n + a) * 3;
                o[0] = v[0];
                o[1] = v[1];
                o[2] = v[2];
            }
            if (heavy_out) {
                const int hs = heavy_slot[a];  // position of atom a among the heavy atoms, or -1
                if (hs >= 0) {
                    double *h = heavy_out + (r * n_heavy + hs) * 3;
                    h[0] = v[0];
                    h[1] = v[1];
                    h[2] = v[2];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace tsc
