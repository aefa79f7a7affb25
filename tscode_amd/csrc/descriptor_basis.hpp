// descriptor_basis.hpp -- k_descriptor_basis: the principal axes of the two feature families from their second moments, in one wavefront
// each (launched by prune.hip for a prune of its own and by pipeline.hip for the pipeline's basis chain).
#pragma once
#include "descriptor.hpp"

namespace tsc {

// Device-side descriptor basis: one wavefront per feature family.  Orthonormal rows spanning the leading principal
// axes of the feature covariance by a few steps of block power iteration (the spectrum of these features decays
// fast: one step gives the screening power of three to within 3 % of the pairs that reach H).  Rows are re-orthonormalised by
// CholeskyQR2: lane (i, j) accumulates the Gram entry <W_i, W_j>, lane 0 factors the 8x8 Gram matrix, every lane
// applies L^-1 to its columns -- no cross-lane reduction on the critical path.  Whatever the iteration produced,
// the rows are finally divided by sqrt of a Gershgorin bound of |V V^T|_2, so |V x| <= |x| holds rigorously and
// the screen can never drop a similar pair.
//   M      second moments of the family, (nf+1)^2, upper triangle filled, index nf = the constant 1
//   Qout   [KD][nf] rows of the basis;  bias[k] = V_k . mean
#ifndef TSC_BASIS_ITERS
#define TSC_BASIS_ITERS 1
#endif
constexpr int BASIS_ITERS = TSC_BASIS_ITERS;
constexpr int BASIS_LDS_C = 64;  // covariance staged in LDS up to this many features
inline __global__ __launch_bounds__(64) void k_descriptor_basis(const double *__restrict__ M0, const double *__restrict__ M1, int nf0, int nf1,
                                                          int n_samples, double *__restrict__ Q, double *__restrict__ bias,
                                                          unsigned *__restrict__ zero_word, double *__restrict__ spread_host = nullptr,
                                                          int clear_moments = 0) {
    // clear_moments: the moment matrices are accumulators that k_sample_moments adds into: this kernel, their one reader, leaves them zero
    // spread_host (optional): host-visible copy of the two spread values written at the end (pinned memory; the host pre-sets +inf
    // and looks without waiting: whatever finite values it finds are this kernel's)
    // zero_word (optional): the running max |D| of a descriptor build that follows this kernel, cleared here
    if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0u;
    __shared__ double V[KD][DESC_MAX_FEAT], Z[KD][DESC_MAX_FEAT], mu[DESC_MAX_FEAT];
    __shared__ double Cs[BASIS_LDS_C][BASIS_LDS_C + 1];
    __shared__ double Gm[KD][KD];  // Gram matrix of the rows being orthonormalised
    const int fam = blockIdx.x, lane = threadIdx.x;
    const double *M = fam == 0 ? M0 : M1;
    const int nf = fam == 0 ? nf0 : nf1, m = nf + 1;
    double *Qout = Q + (fam == 0 ? 0 : size_t(KD) * nf0);
    double *bout = bias + fam * KD;
    if (nf == 0) {
        if (lane < KD) bout[lane] = 0.0;
        if (lane == 0) {
            bias[DW + fam] = 0.0;  // (a family without features separates nothing)
            if (spread_host) spread_host[fam] = 0.0;
        }
        return;
    }
    const double inv = n_samples > 0 ? 1.0 / n_samples : 0.0;
    for (int a = lane; a < nf; a += 64) mu[a] = M[size_t(a) * m + nf] * inv;
    __builtin_amdgcn_wave_barrier();
    const bool c_in_lds = nf <= BASIS_LDS_C;
    if (c_in_lds)
        for (int e = lane; e < nf * nf; e += 64) {
            const int a = e / nf, b = e - a * nf;
            Cs[a][b] = (a <= b ? M[size_t(a) * m + b] : M[size_t(b) * m + a]) * inv - mu[a] * mu[b];
        }
    for (int k = 0; k < KD; ++k)
        for (int a = lane; a < nf; a += 64) V[k][a] = ((a % KD) == k ? 1.0 : 0.0) + 1e-3 * ((a * 7 + k * 13) % 11 - 5);
    __builtin_amdgcn_wave_barrier();

    // W <- rows of an orthonormal basis of span(W) (zero rows where the span is exhausted)
    auto cholesky_qr = [&](double (*W)[DESC_MAX_FEAT]) {
        const int gi = lane >> 3, gj = lane & 7;  // 64 lanes = the 8 x 8 Gram entries
        double g = 0.0;
#pragma unroll 4
        for (int a = 0; a < nf; ++a) g = fma(W[gi][a], W[gj][a], g);
        Gm[gi][gj] = g;
        __builtin_amdgcn_wave_barrier();
        // every lane factors the 8 x 8 Gram matrix in registers (constant indices only): G = L L^T, then Li = L^-1 -- in float32: this
        // kernel is one wavefront's instruction stream (about 40 us, on the critical path of the pipeline's front half), most of it the
        // float64 divisions and square roots of the factorisation; rows orthonormal to 1e-6 serve as well (the second pass of CholeskyQR2
        // repairs what the first leaves, and the Gershgorin scaling below makes |V x| <= |x| hold for whatever comes out)
        float L[KD][KD], Li[KD][KD];
        float tr = 0.0f;
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) L[i][j] = float(Gm[i][j]);
            tr += L[i][i];
        }
        bool dead[KD];
        float rinv[KD];  // 1 / L[i][i]
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                float sacc = L[i][j];
#pragma unroll
                for (int t = 0; t < j; ++t) sacc = fmaf(-L[i][t], L[j][t], sacc);
                if (i == j) {
                    dead[i] = !(sacc > 1e-6f * tr) || !(tr > 0.0f);
                    L[i][i] = dead[i] ? 1.0f : sqrtf(sacc);
                    rinv[i] = 1.0f / L[i][i];
                } else {
                    L[i][j] = dead[j] ? 0.0f : sacc * rinv[j];
                }
            }
            if (dead[i]) {
#pragma unroll
                for (int j = 0; j < i; ++j) L[i][j] = 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < KD; ++j) {
#pragma unroll
            for (int i = j; i < KD; ++i) {
                float sacc = (i == j) ? 1.0f : 0.0f;
#pragma unroll
                for (int t = j; t < i; ++t) sacc = fmaf(-L[i][t], Li[t][j], sacc);
                Li[i][j] = dead[i] ? 0.0f : sacc * rinv[i];
            }
        }
        for (int a = lane; a < nf; a += 64) {
            double w[KD];
#pragma unroll
            for (int k = 0; k < KD; ++k) w[k] = W[k][a];
#pragma unroll
            for (int i = 0; i < KD; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j <= i; ++j) acc = fma(double(Li[i][j]), w[j], acc);
                W[i][a] = acc;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    // (the start rows are not orthonormalised first: C V spans the same nested subspaces whether V or L^-1 V is fed in -- CholeskyQR mixes
    // row i with rows before it only -- so the rows that come out of the step are the same, and two of the four factorisations of this
    // one-wavefront kernel, which sits on the critical path of the pipeline's front half, are saved)
    for (int it = 0; it < BASIS_ITERS; ++it) {
        // Z_k = C V_k with C[a][b] = M[a][b]/ns - mu_a mu_b
        for (int a = lane; a < nf; a += 64) {
            double acc[KD];
#pragma unroll
            for (int k = 0; k < KD; ++k) acc[k] = 0.0;
#pragma unroll 4
            for (int b = 0; b < nf; ++b) {
                const double cab = c_in_lds ? Cs[a][b] : ((a <= b ? M[size_t(a) * m + b] : M[size_t(b) * m + a]) * inv - mu[a] * mu[b]);
#pragma unroll
                for (int k = 0; k < KD; ++k) acc[k] = fma(cab, V[k][b], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < KD; ++k) Z[k][a] = acc[k];
        }
        __builtin_amdgcn_wave_barrier();
        cholesky_qr(Z);
        cholesky_qr(Z);
        // a direction that C annihilated comes back as a zero row: keep the previous row there if it is still
        // orthogonal to the new ones?  Not needed for validity -- a zero row only weakens the screen.
        for (int k = 0; k < KD; ++k)
            for (int a = lane; a < nf; a += 64) V[k][a] = Z[k][a];
        __builtin_amdgcn_wave_barrier();
    }
    // Gershgorin bound of the largest eigenvalue of V V^T (= |V|_2^2): max_i sum_j |<V_i, V_j>|
    {
        const int gi = lane >> 3, gj = lane & 7;
        double g = 0.0;
        for (int a = 0; a < nf; ++a) g = fma(V[gi][a], V[gj][a], g);
        Gm[gi][gj] = fabs(g);
        __builtin_amdgcn_wave_barrier();
    }
    double gmax = 0.0;
    for (int i = 0; i < KD; ++i) {
        double row = 0.0;
        for (int j = 0; j < KD; ++j) row += Gm[i][j];
        gmax = fmax(gmax, row);
    }
    const double sc = gmax > 0.0 ? 1.0 / sqrt(gmax * (1.0 + 1e-12)) : 0.0;
    for (int a = lane; a < nf; a += 64)
        for (int k = 0; k < KD; ++k) {
            const double v = V[k][a] * sc;
            V[k][a] = v;
            Qout[size_t(k) * nf + a] = v;
        }
    __builtin_amdgcn_wave_barrier();
    if (lane < KD) {
        double b = 0.0;
        for (int a = 0; a < nf; ++a) b = fma(V[lane][a], mu[a], b);
        bout[lane] = b;
    }
    // How far apart two structures of the sample lie in this family's descriptor, on average: E |V (f(p) - f(q))|^2 = 2 sum_k V_k^T C V_k.
    // The host compares it with the screen's limit h thr^2: where both families stay below it the screen can separate (almost)
    // nothing -- every pair would reach H anyway -- and an all-pairs kernel without a screen is the faster route (prune_api.hpp,
    // screen_is_useless).  Only worked out where that kernel exists (up to 32 heavy atoms); +inf otherwise.
    double spread = __builtin_inf();
    if (nf <= 32) {  // (c_in_lds) lane = (row k of V, an eighth of the features a): 64 lanes share the nf^2 KD products
        static_assert(KD == 8 && BASIS_LDS_C >= 32, "lane layout of the spread estimate");
        const int k = lane & 7;
        double lam = 0.0;
        for (int a = lane >> 3; a < nf; a += 8) {
            double z = 0.0;
            for (int b = 0; b < nf; ++b) z = fma(Cs[a][b], V[k][b], z);
            lam = fma(V[k][a], z, lam);
        }
        for (int off = 32; off > 0; off >>= 1) lam += __shfl_xor(lam, off);
        spread = 2.0 * lam;
    }
    if (lane == 0) {
        bias[DW + fam] = spread;
        if (spread_host) {
            spread_host[fam] = spread;
            __threadfence_system();
        }
    }
    if (clear_moments) {
        double *Mw = const_cast<double *>(M);
        for (int e = lane; e < m * m; e += 64) Mw[e] = 0.0;
    }
}

}  // namespace tsc
