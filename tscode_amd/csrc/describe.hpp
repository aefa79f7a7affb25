// describe.hpp -- the two kernels that write descriptor rows, both through describe_from_lds: k_descriptors (a prune of its own: prune.hip) and
// k_transform_describe (K1 with the descriptors fused in: pipeline.hip).  They stay in ONE header that both units include although each
// launches one of the two: compiled without the other in its unit, either kernel comes out with its address arithmetic scheduled in another
// order (same registers, same length) -- and this layout moves no instruction.
#pragma once
#include "descriptor.hpp"
#include "embed_clash.hpp"

namespace tsc {

// The descriptor rows of the ns structures staged in LDS (s_x, `pitch` doubles apart; s_q = both bases): T = 256 / S
// consecutive lanes share a structure (atoms sub, sub + T, ...) and reduce with shuffles.  Called by all 256 threads.
__device__ inline void describe_from_lds(const double *s_q, const double *s_x, int pitch, int h, int nf0, int nf1, const double *__restrict__ bias,
                                         int ns, int S, int64_t i0, float *__restrict__ D, double *__restrict__ G, unsigned *__restrict__ dmax_bits) {
    const int T = 256 / S;
    const int sidx = threadIdx.x / T, sub = threadIdx.x - sidx * T;
    const bool mine = sidx < ns;
    double d[DW], g = 0.0;
#pragma unroll
    for (int k = 0; k < DW; ++k) d[k] = 0.0;
    if (mine) {
        const double *x = s_x + sidx * pitch;
        const double *q1 = s_q + KD * nf0;
        for (int a = sub; a < h; a += T) {
            const double n2 = x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1] + x[3 * a + 2] * x[3 * a + 2];
            g += n2;
            if (a < nf0) {
                const double f = sqrt(n2);
#pragma unroll
                for (int k = 0; k < KD; ++k) d[k] = fma(s_q[k * nf0 + a], f, d[k]);
            }
            if (a < nf1) {
                const double f = feature(x, h, 1, a);
#pragma unroll
                for (int k = 0; k < KD; ++k) d[KD + k] = fma(q1[k * nf1 + a], f, d[KD + k]);
            }
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1) {  // T <= 64 consecutive lanes of one wavefront
#pragma unroll
        for (int k = 0; k < DW; ++k) d[k] += __shfl_xor(d[k], off);
        g += __shfl_xor(g, off);
    }
    float mx = 0.0f;
    if (mine && sub == 0) {
        float v[DW];
#pragma unroll
        for (int k = 0; k < DW; ++k) {
            v[(k % KD) * 2 + k / KD] = float(d[k] - bias[k]);
            mx = fmaxf(mx, fabsf(float(d[k] - bias[k])));
        }
        f32x4 *dst = reinterpret_cast<f32x4 *>(D + (i0 + sidx) * DW);
#pragma unroll
        for (int k = 0; k < DW / 4; ++k) dst[k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
        G[i0 + sidx] = g;
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    // same-address atomics serialise (about 12 ns each): only a wavefront that would raise the maximum sends one
    if ((threadIdx.x & 63) == 0 && mx > __uint_as_float(__hip_atomic_load(dmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
        atomicMax(dmax_bits, __float_as_uint(mx));
    // A structure with a NaN or infinite coordinate (its squared norm is not finite) raises the running maximum to the bit pattern of
    // a NaN: the screen's limit then drops nothing (screen_limit32*), the evaluation stages find such a structure similar to nothing
    // (every comparison with a NaN is false, rmsd_pruning.py:75), and the run reports that it saw one (tsc_pass_stats.nonfinite_input;
    // the reference's np.linalg.svd raises LinAlgError on such input, rmsd_pruning.py:19)
    if (__ballot(mine && sub == 0 && !(g < 1.7976931348623157e308)) != 0 && (threadIdx.x & 63) == 0) atomicMax(dmax_bits, NONFINITE_BITS);
}

// D[i][2k + fam] = sum_a Q_fam[k][a] * f_fam,a(x_i) - bias[fam*KD + k]   (fp32, original index space, the two families
// interleaved; the bias is the projection of the mean feature vector and cancels in every difference),
// G[i] = sum_a |x_ia|^2; *dmax_bits = max |D| over everything as the bit pattern of a non-negative float (atomicMax on the
// integer view; zero on entry) -- the pair kernel turns it into the fp32 limit of the screen (screen_limit32).
// A block stages S structures in LDS with coalesced loads (a thread-per-structure walk reads 64 lines per instruction and
// thrashes the L1); T = 256 / S consecutive lanes share a structure (atoms sub, sub + T, ...) and reduce with shuffles.
inline __global__ __launch_bounds__(256) void k_descriptors(const double *__restrict__ heavy, int64_t n, int h, int nf0, int nf1,
                                                      const double *__restrict__ Q, const double *__restrict__ bias, float *__restrict__ D,
                                                      double *__restrict__ G, unsigned *__restrict__ dmax_bits, int S) {
    extern __shared__ __attribute__((aligned(16))) double s_mem[];  // [KD][nf0], [KD][nf1], then S rows of pitch doubles
    const int h3 = h * 3, pitch = h3 | 1;
    double *s_q = s_mem, *s_x = s_mem + KD * (nf0 + nf1);
    for (int e = threadIdx.x; e < KD * (nf0 + nf1); e += 256) s_q[e] = Q[e];
    const int64_t i0 = int64_t(blockIdx.x) * S;
    const int ns = int(min<int64_t>(S, n - i0));
    const double *src = heavy + i0 * h3;
    // eight loads in flight per thread before the first LDS store (a plain copy loop waits for every load in turn)
    for (int base = threadIdx.x; base < ns * h3; base += 256 * 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (base + 256 * j < ns * h3) ? src[base + 256 * j] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = base + 256 * j;
            if (e < ns * h3) {
                const int row = e / h3;
                s_x[row * pitch + (e - row * h3)] = v[j];
            }
        }
    }
    __syncthreads();
    describe_from_lds(s_q, s_x, pitch, h, nf0, nf1, bias, ns, S, i0, D, G, dmax_bits);
}

// K1 with the descriptors of the prune fused in (tsc_pipeline_dev, when the basis is ready before the passing poses are
// embedded): k_transform's workgroup of TR_POSES poses keeps the heavy atoms it has just computed in LDS and takes their
// descriptor rows from there, so the 24 h bytes per structure are not read back by a k_descriptors launch.
// dynamic LDS: transform_lds_bytes(n_mols), then [KD][nf0 + nf1] basis doubles, then TR_POSES rows of (3 h | 1) doubles.
inline __global__ __launch_bounds__(256) void k_transform_describe(const double *__restrict__ frags, FragTable ft, const int32_t *__restrict__ conf_idx,
                                                             const double *__restrict__ rot, const double *__restrict__ pos,
                                                             const int32_t *__restrict__ idx, double *__restrict__ out,
                                                             const int32_t *__restrict__ heavy_slot, int n_heavy, double *__restrict__ heavy_out,
                                                             const int32_t *__restrict__ n_out_dev, int nf0, int nf1, const double *__restrict__ Q,
                                                             const double *__restrict__ bias, float *__restrict__ D, double *__restrict__ G,
                                                             unsigned *__restrict__ dmax_bits, float *__restrict__ heavy32_out = nullptr) {
    // heavy32_out (optional): the float32 copy of the heavy atoms that stage 1 of the pair kernels reads (pair_stage1), zero-padded rows
    extern __shared__ __attribute__((aligned(16))) double s_tr[];
    const int n = ft.n_total, nm = ft.n_mols, tid = threadIdx.x, pitch = (n_heavy * 3) | 1;
    const int pitch32 = heavy32_pitch(n_heavy), pad32 = pitch32 - 3 * n_heavy;
    const int64_t n_out = *n_out_dev;
    int64_t *sP = reinterpret_cast<int64_t *>(s_tr);
    double *sR = s_tr + TR_POSES, *sT = sR + TR_POSES * nm * 9;
    int *sC = reinterpret_cast<int *>(sT + TR_POSES * nm * 3);
    double *s_q = s_tr + (transform_lds_bytes(nm) + 15) / 16 * 2, *s_x = s_q + KD * (nf0 + nf1);
    for (int e = tid; e < KD * (nf0 + nf1); e += 256) s_q[e] = Q[e];
    for (int64_t r0 = int64_t(blockIdx.x) * TR_POSES; r0 < n_out; r0 += int64_t(gridDim.x) * TR_POSES) {
        const int np = int(min<int64_t>(TR_POSES, n_out - r0));
        if (tid < np) sP[tid] = int64_t(idx[r0 + tid]);
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
                o[0] = v[0], o[1] = v[1], o[2] = v[2];
            }
            const int hs = heavy_slot[a];
            if (hs >= 0) {
                double *hv = heavy_out + (r * n_heavy + hs) * 3, *x = s_x + row * pitch + hs * 3;
                hv[0] = x[0] = v[0], hv[1] = x[1] = v[1], hv[2] = x[2] = v[2];
                if (heavy32_out) {
                    float *hf = heavy32_out + r * pitch32 + hs * 3;
                    hf[0] = float(v[0]), hf[1] = float(v[1]), hf[2] = float(v[2]);
                }
            }
        }
        if (heavy32_out)
            for (int e = tid; e < np * pad32; e += 256) heavy32_out[(r0 + e / pad32) * pitch32 + 3 * n_heavy + e % pad32] = 0.0f;
        __syncthreads();
        describe_from_lds(s_q, s_x, pitch, n_heavy, nf0, nf1, bias, np, TR_POSES, r0, D, G, dmax_bits);
        __syncthreads();
    }
}

inline size_t transform_describe_lds_bytes(int n_mols, int h) {
    return (transform_lds_bytes(n_mols) + 15) / 16 * 16 + (size_t(KD) * (n_features(h, 0) + n_features(h, 1)) + size_t(TR_POSES) * ((h * 3) | 1)) * sizeof(double);
}

}  // namespace tsc
