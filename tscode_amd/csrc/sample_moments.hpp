// sample_moments.hpp -- k_sample_moments, the first link of the pipeline's basis chain: the sample poses embedded and their feature moments
// added up in one launch (launched by pipeline.hip alone).
#pragma once
#include "descriptor.hpp"
#include "embed_clash.hpp"

namespace tsc {

// The first link of the pipeline's basis chain on one device: the sample poses are embedded (heavy atoms, into LDS only) and the second
// moments of their features added up -- k_transform + k_feature_moments (fast form) in one launch, without the round trip of the sample's
// coordinates through memory.  grid (groups of SM_CHUNKS chunks of TR_POSES samples, NFAM); M0 / M1 are zero on entry (k_descriptor_basis clears them again).
// dynamic LDS: sample_moments_lds_bytes
constexpr int SM_CHUNKS = 1;  // chunks of TR_POSES samples per workgroup of k_sample_moments (4: 52 us instead of 26 -- a chunk is a chain of
                              // dependent loads, about 13 us beside the clash kernel, and the chains of a workgroup run one after the other)
__host__ __device__ inline size_t sample_moments_lds_bytes(int n_mols, int h) {
    return (transform_lds_bytes(n_mols) + 15) / 16 * 16 + size_t(TR_POSES) * (size_t(h) * 3 + size_t(h) + 1) * sizeof(double);
}
inline __global__ __launch_bounds__(256) void k_sample_moments(const double *__restrict__ frags, FragTable ft, const int32_t *__restrict__ conf_idx,
                                                        const double *__restrict__ rot, const double *__restrict__ pos,
                                                        const int32_t *__restrict__ sample_idx, int n_samples, const int32_t *__restrict__ heavy_slot,
                                                        int h, int nf0, int nf1, double *__restrict__ M0, double *__restrict__ M1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_sm_raw[];
    const int fam = blockIdx.y, nf = fam == 0 ? nf0 : nf1;
    if (nf == 0) return;
    const int n = ft.n_total, nm = ft.n_mols, tid = threadIdx.x, m = nf + 1;
    double *s_tr = reinterpret_cast<double *>(s_sm_raw);
    int64_t *sP = reinterpret_cast<int64_t *>(s_tr);
    double *sR = s_tr + TR_POSES, *sT = sR + TR_POSES * nm * 9;
    int *sC = reinterpret_cast<int *>(sT + TR_POSES * nm * 3);
    double *s_x = reinterpret_cast<double *>(s_sm_raw + (transform_lds_bytes(nm) + 15) / 16 * 16);   // [TR_POSES][h * 3]
    double *s_n = s_x + size_t(TR_POSES) * h * 3;                                                    // [TR_POSES][m]
    double *__restrict__ Mf = fam == 0 ? M0 : M1;
    const int n_chunks = (n_samples + TR_POSES - 1) / TR_POSES;
    // a workgroup takes SM_CHUNKS consecutive chunks and adds their products up in registers before it touches the accumulators
    constexpr int ACC = 8;
    const bool in_regs = m * m <= 256 * ACC;
    double acc[ACC];
#pragma unroll
    for (int u = 0; u < ACC; ++u) acc[u] = 0.0;
    for (int ch = blockIdx.x * SM_CHUNKS; ch < min(n_chunks, (int(blockIdx.x) + 1) * SM_CHUNKS); ++ch) {
        const int s0 = ch * TR_POSES, ns = min(TR_POSES, n_samples - s0);
        if (tid < ns) sP[tid] = int64_t(sample_idx[s0 + tid]);
        __syncthreads();
        for (int q = tid; q < ns * nm * 9; q += 256) {
            const int row = q / (nm * 9), w = q - row * nm * 9;
            sR[q] = rot[sP[row] * nm * 9 + w];
        }
        for (int q = tid; q < ns * nm * 3; q += 256) {
            const int row = q / (nm * 3), w = q - row * nm * 3;
            sT[q] = pos[sP[row] * nm * 3 + w];
        }
        for (int q = tid; q < ns * nm; q += 256) {
            const int row = q / nm, w = q - row * nm;
            sC[q] = conf_idx[sP[row] * nm + w];
        }
        __syncthreads();
        for (int e = tid; e < ns * n; e += 256) {
            const int row = e / n, a = e - row * n;
            const int hs = heavy_slot[a];
            if (hs < 0) continue;
            double v[3];
            embed_atom_staged(frags, ft, sR, sT, sC, row, a, v);
            double *o = s_x + (size_t(row) * h + hs) * 3;
            o[0] = v[0], o[1] = v[1], o[2] = v[2];
        }
        __syncthreads();
        for (int e = tid; e < ns * m; e += 256) {
            const int sm = e / m, a = e - sm * m;
            s_n[sm * m + a] = (a < nf) ? feature(s_x + size_t(sm) * h * 3, h, fam, a) : 1.0;
        }
        __syncthreads();
        if (in_regs) {
#pragma unroll
            for (int u = 0; u < ACC; ++u) {
                const int e = tid + 256 * u;
                if (e < m * m) {
                    const int a = e / m, b = e - a * m;
                    if (b >= a) {
                        double t = 0.0;
                        for (int sm = 0; sm < ns; ++sm) t += s_n[sm * m + a] * s_n[sm * m + b];
                        acc[u] += t;
                    }
                }
            }
        } else {
            for (int e = tid; e < m * m; e += 256) {
                const int a = e / m, b = e - a * m;
                if (b < a) continue;
                double t = 0.0;
                for (int sm = 0; sm < ns; ++sm) t += s_n[sm * m + a] * s_n[sm * m + b];
                atomicAdd(&Mf[e], t);
            }
        }
        __syncthreads();
    }
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < ACC; ++u) {
            const int e = tid + 256 * u;
            if (e < m * m && e % m >= e / m) atomicAdd(&Mf[e], acc[u]);
        }
    }
}

}  // namespace tsc
