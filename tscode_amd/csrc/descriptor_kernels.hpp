// descriptor_kernels.hpp -- what a prune run builds its descriptors with, launched by prune.hip alone: the feature moments of a sample,
// the trivial basis, the descriptors of every structure and the float32 copy of the heavy atoms.
#pragma once
#include "descriptor.hpp"

namespace tsc {

// Second-moment matrix of the sampled feature vectors of one family, with a constant 1 appended:
// M[a][b] = sum_s f_a(s) f_b(s), a, b in [0, nf]  (index nf = the constant) -> mean and covariance on the host.
// blockIdx.y = family: both moment matrices come out of one launch.
// DETERMINISTIC: the sums are taken in a fixed order -- workgroup b of the MOM_BLOCKS of a family adds the chunks b, b + MOM_BLOCKS,
// ... into a partial matrix of its own (Mfam + b * m * m: every entry has one owner thread, no atomics) and the workgroup that
// finishes last adds the partials in index order.  The basis, the descriptors and with them the Morton order of a culled pass
// (cull.hpp) then come out bit for bit the same on every rank of a sharded run that feeds them the same sample: the ranks deal
// the tiles of that order among themselves, and orders that differed in one structure would let pairs go unvisited.
inline __global__ __launch_bounds__(256) void k_feature_moments(const double *__restrict__ heavy, int h, int nf0, int nf1, int64_t stride_structs,
                                                          int n_samples, double *__restrict__ M0, double *__restrict__ M1, unsigned *__restrict__ tickets) {
    // tickets == null: the fast form -- one workgroup per chunk of 32 samples, atomicAdd into the (zeroed) first partial matrix of the
    // family: the order of the additions, and with it the last bits of the basis, differ from run to run.  Any basis gives the same
    // verdicts; only a SHARDED run needs the same bits on every rank (option "deterministic_basis").
    // tickets[fam] (zero on entry): the workgroup of a family that finishes LAST adds the partial matrices up, in index order, into the first
    extern __shared__ __attribute__((aligned(16))) double s_n[];  // [chunk][nf + 1]
    __shared__ int s_last;
    const int fam = blockIdx.y, nf = fam == 0 ? nf0 : nf1;
    if (nf == 0) return;
    const int m = nf + 1;
    double *__restrict__ Mf = fam == 0 ? M0 : M1;
    constexpr int CHUNK = 32;
    const int n_chunks = (n_samples + CHUNK - 1) / CHUNK;
    if (!tickets) {
        for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
            const int s0 = ch * CHUNK, ns = min(CHUNK, n_samples - s0);
            for (int e = threadIdx.x; e < ns * m; e += blockDim.x) {
                int s = e / m, a = e - s * m;
                s_n[s * m + a] = (a < nf) ? feature(heavy + int64_t(s0 + s) * stride_structs * h * 3, h, fam, a) : 1.0;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
                int a = e / m, b = e - a * m;
                if (b < a) continue;
                double acc = 0.0;
                for (int s = 0; s < ns; ++s) acc += s_n[s * m + a] * s_n[s * m + b];
                atomicAdd(&Mf[e], acc);
            }
            __syncthreads();
        }
        return;
    }
    double *__restrict__ M = Mf + size_t(blockIdx.x) * m * m;
    bool first = true;
    for (int ch = blockIdx.x; ch < n_chunks || first; ch += gridDim.x) {
        const int s0 = ch * CHUNK, ns = ch < n_chunks ? min(CHUNK, n_samples - s0) : 0;   // (a workgroup without a chunk still writes zeros)
        for (int e = threadIdx.x; e < ns * m; e += blockDim.x) {
            int s = e / m, a = e - s * m;
            s_n[s * m + a] = (a < nf) ? feature(heavy + int64_t(s0 + s) * stride_structs * h * 3, h, fam, a) : 1.0;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
            int a = e / m, b = e - a * m;
            if (b < a) continue;
            double acc = first ? 0.0 : M[e];
            for (int s = 0; s < ns; ++s) acc += s_n[s * m + a] * s_n[s * m + b];
            M[e] = acc;
        }
        __syncthreads();
        first = false;
    }
    // Hand-off of the partial matrices to the workgroup that finishes last, in the form MI355X_MICROARCH.md lists as valid (inter-workgroup
    // visibility): every storing wavefront drains its stores, the workgroup meets, ONE lane releases at agent scope (write-back of the XCD's
    // L2) and -- behind an explicit wait the compiler cannot drop: its pass removes the one after buffer_wbl2 when it believes the scoreboard
    // empty, and the ticket could then overtake the write-back -- takes the ticket; the last workgroup acquires before it loads.  (Rounds
    // 2 - 3 had __threadfence() on both sides and no explicit wait; no wrong basis was ever traced to it.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = (atomicAdd(&tickets[fam], 1u) == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
        int a = e / m, b = e - a * m;
        if (b < a) continue;
        // (this workgroup has not touched the other workgroups' partials before: the loads miss its CU's cache and come from the L2,
        // where the writers' stores are since their fences; all of an entry's partials in flight at once, added in index order)
        double v[MOM_BLOCKS], acc = 0.0;
#pragma unroll
        for (int u = 0; u < MOM_BLOCKS; ++u) v[u] = __builtin_nontemporal_load(&Mf[size_t(u) * m * m + e]);   // one round trip
#pragma unroll
        for (int u = 0; u < MOM_BLOCKS; ++u) acc += v[u];
        Mf[e] = acc;   // (entry e of partial 0 is read by this thread alone)
    }
}

// The trivial basis for small ensembles: component k of a family = its feature k (rows of the identity: |Q x| <= |x|), no
// centring.  Any basis gives the same verdicts; with a few thousand structures the screen has little to do, and estimating
// principal axes (a memset, a moments launch and the one-wavefront basis kernel: about 45 us of latency) costs more than it saves.
inline __global__ void k_identity_basis(int nf0, int nf1, double *__restrict__ Q, double *__restrict__ bias) {
    const int total = KD * (nf0 + nf1);
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int fam = e < KD * nf0 ? 0 : 1, r = fam == 0 ? e : e - KD * nf0, nf = fam == 0 ? nf0 : nf1;
        Q[e] = (r / nf == r % nf) ? 1.0 : 0.0;
    }
    for (int e = threadIdx.x; e < DW; e += blockDim.x) bias[e] = 0.0;
    if (threadIdx.x < NFAM) bias[DW + threadIdx.x] = __builtin_inf();  // (no estimate of the descriptors' spread: k_descriptor_basis)
}

// The float32 copy of the heavy atoms that stage 1 of the pair kernels reads first (pair_stages.hpp: pair_H32)
inline __global__ __launch_bounds__(256) void k_heavy32(const double *__restrict__ heavy, int64_t n, int h, float *__restrict__ out) {
    const int h3 = h * 3, pitch = heavy32_pitch(h);
    const int64_t total = n * pitch;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t i = e / pitch;
        const int w = int(e - i * pitch);
        out[e] = w < h3 ? float(heavy[i * h3 + w]) : 0.0f;
    }
}

}  // namespace tsc
