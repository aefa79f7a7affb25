// leader.hpp -- the energy-ordered RMSD prune: walk the rows in a given order and keep a row iff no row KEPT before it is similar to it
// (the greedy filter of tscode/embeds.py:715, :843, for a whole ensemble).  A removed row never covers anything, so the rule is sequential
// by definition; what is parallel is the pair work, and it is stated in blocks of LEADER_BLOCK rows of the order (leader_plan.hpp):
//
//   (a) the block against everything kept so far -- the caller's library and the kept rows of the earlier blocks, one growing pack in the
//       cross layout -- with the CX_FIRST rectangle of cross.hpp: first[s] = the lowest similar pack index.  A covered row is decided.
//   k_leader_bits    (b) for the rows (a) left open, the bits similar(s -> j) for every open j < s of the block: a wavefront owns LD_ROWS
//                    rows and one 64-column tile, a lane an earlier row; row s is turned onto row j (rmsd_pruning.py:6-41, the later onto
//                    the earlier) by the verdict functions of the general cross path (cross_pair_S, certainly_dissimilar,
//                    exact_rmsd_maxdev) and a ballot writes the word.  Every word the replay reads is written, nothing is accumulated.
//   k_leader_replay  (c) ONE wavefront replays the order on the bits, 64 rows at a time: a row falls to the lowest accepted j < s that has
//                    its bit, else it is accepted.  Against the accepted rows of earlier 64-row groups every lane tests its own row at
//                    once; inside a group the 64 rows are resolved one after the other on a 64-bit word.  It writes mask / rep / lib_rep
//                    through the order, the block's accepted rows and the call's kept count.
//   k_leader_append  (d) the accepted rows join the pack: rows of Xr, columns of Xc, G.
//
// The kept count goes back to the host once per block (4 bytes) and sizes the next block's library walk; no kernel waits for another
// workgroup and no grid is sized from device memory (k_leader_append is launched for the block's row count and reads how many rows there are).
#pragma once

#include "cross.hpp"
#include "leader_plan.hpp"

namespace tsc {

struct LeaderBitsArgs {
    const double *Xr;           // [nb][pitch] the block's rows, in order (this block's first row at 0)
    const int32_t *first;       // [nb] the library walk's verdict: INT32_MAX = open
    int nb;                     // rows of the block
    int h, pitch;
    double thr, maxdev_thr, half_h_thr2;
    unsigned long long *bits;   // [nb][LEADER_WORDS]; word w of row s is written for every w <= s / 64, bit j - 64 w: similar(s -> j), j < s, both open
};

inline __global__ __launch_bounds__(64 * LD_WAVES) void k_leader_bits(LeaderBitsArgs a) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = (int(blockIdx.x) * LD_WAVES + wid) * LD_ROWS;
    const int c0 = int(blockIdx.y) * 64;
    if (r0 >= a.nb || c0 > r0) return;   // (wavefront-uniform) no row, or every column at or behind the rows
    const int nrows = a.nb - r0 < LD_ROWS ? a.nb - r0 : LD_ROWS;
    const int j = c0 + lane;             // < nb: c0 <= r0 < nb covers lane 0 only, the others are checked
    const bool col_open = j < a.nb && a.first[j] == INT_MAX;
    const double *__restrict__ ql = a.Xr + (long long)(j < a.nb ? j : 0) * a.pitch;
    for (int t = 0; t < nrows; ++t) {
        const int s = r0 + t;
        unsigned long long word = 0;
        if (a.first[s] == INT_MAX) {     // (uniform)
            const double *__restrict__ pr = a.Xr + (long long)s * a.pitch;
            bool sim = false;
            if (col_open && j < s) {
                double S[9], Gp, Gq, rm, md;
                cross_pair_S(pr, ql, a.h, S, Gp, Gq);
                const double half_sum = 0.5 * (Gp + Gq);
                if (!certainly_dissimilar(S, half_sum - a.half_h_thr2, half_sum, a.h)) {
                    exact_rmsd_maxdev(pr, ql, a.h, S, Gp, Gq, rm, md);
                    sim = rm < a.thr && md < a.maxdev_thr;   // rmsd_pruning.py:75
                }
            }
            word = __ballot(sim);
        }
        if (lane == 0) a.bits[(long long)s * LEADER_WORDS + blockIdx.y] = word;
    }
}

struct LeaderReplayArgs {
    const unsigned long long *bits;   // [nb][LEADER_WORDS]
    const int32_t *first;             // [nb] this block's slice
    const int32_t *order;             // [n] or null: the identity
    long long n;                      // rows of the call
    long long b0;                     // position of the block's first row in the order
    int nb;
    int n_library;                    // pack indices below it are the caller's library rows
    int kept_before;                  // rows of this call kept by the earlier blocks: pack index n_library + k is kept_src[k]
    int32_t *kept_src;                // [n] the caller's row of every kept row, in the order they were kept
    int32_t *acc_pos;                 // [nb] out: the block rows accepted, ascending
    int32_t *count;                   // out: kept_before + the block's accepted rows
    uint8_t *mask;                    // [n], through the order
    int32_t *rep, *lib_rep;           // [n], through the order
};

inline __global__ __launch_bounds__(64) void k_leader_replay(LeaderReplayArgs a) {
    __shared__ unsigned long long s_acc[LEADER_WORDS];   // the accepted rows of the groups done
    const int lane = threadIdx.x;
    int kept_run = 0;
    for (int g = 0; g * 64 < a.nb; ++g) {
        const int s = g * 64 + lane;
        const bool in = s < a.nb;
        const int f = in ? a.first[s] : 0;
        const bool open = in && f == INT_MAX;
        const unsigned long long *row = a.bits + (long long)(in ? s : 0) * LEADER_WORDS;
        int hit = -1;
        if (open)
            for (int w = 0; w < g; ++w) {
                const unsigned long long m = row[w] & s_acc[w];
                if (m) {
                    hit = w * 64 + __ffsll((long long)m) - 1;
                    break;
                }
            }
        const bool cand = open && hit < 0;
        const unsigned long long wg = cand ? row[g] : 0ull;
        unsigned long long todo = __ballot(cand), accg = 0;
        while (todo) {   // (uniform) the group's candidates in order: accepted iff no accepted row before it has its bit
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned long long bi = (unsigned long long)__shfl((long long)wg, i);
            if (!(bi & accg)) accg |= 1ull << i;
        }
        if (lane == 0) s_acc[g] = accg;
        __syncthreads();
        const bool kept = cand && ((accg >> lane) & 1ull);
        if (cand && !kept) hit = g * 64 + __ffsll((long long)(wg & accg)) - 1;
        if (in) {
            const long long pos = a.b0 + s;
            const int orig = a.order ? a.order[pos] : int(pos);
            int r = orig, lr = -1;
            if (!open) {
                if (f < a.n_library) r = -1, lr = f;
                else r = a.kept_src[f - a.n_library];
            } else if (!kept) {
                r = a.order ? a.order[a.b0 + hit] : int(a.b0 + hit);
            } else {
                const int k = kept_run + __popcll(accg & ((1ull << lane) - 1ull));
                a.acc_pos[k] = s;
                a.kept_src[a.kept_before + k] = orig;
            }
            if (orig >= 0 && orig < a.n) {   // (an order that is no permutation -- the _dev form does not check it -- writes nowhere)
                a.mask[orig] = kept ? 1 : 0;
                a.rep[orig] = r;
                a.lib_rep[orig] = lr;
            }
        }
        kept_run += __popcll(accg);
    }
    if (lane == 0) *a.count = a.kept_before + kept_run;
}

struct LeaderAppendArgs {
    const double *Er;         // [nb][pitch] the block's rows (this block's first row at 0)
    const double *Eg;         // [nb]
    const int32_t *acc_pos;   // [nb] the accepted block rows, ascending
    const int32_t *count;     // kept rows of this call, this block's included
    int kept_before;
    long long nl;             // pack rows in front of this block's: n_library + kept_before
    long long capacity;       // rows the pack has room for
    int pitch;
    double *Lr;               // [capacity][pitch]
    double *Lc;               // [pitch][ld] or null (general path)
    double *Lg;               // [ld]
    long long ld;
};

// A workgroup per accepted row (striding), its threads on the row's doubles
inline __global__ __launch_bounds__(128) void k_leader_append(LeaderAppendArgs a) {
    const int n_acc = *a.count - a.kept_before;
    for (int k = blockIdx.x; k < n_acc; k += gridDim.x) {
        const long long dst = a.nl + k;
        if (dst >= a.capacity) return;   // (cannot happen: a call keeps at most its own rows)
        const double *__restrict__ src = a.Er + (long long)a.acc_pos[k] * a.pitch;
        for (int d = threadIdx.x; d < a.pitch; d += blockDim.x) {
            const double v = src[d];
            a.Lr[dst * a.pitch + d] = v;
            if (a.Lc) a.Lc[(long long)d * a.ld + dst] = v;
        }
        if (threadIdx.x == 0) a.Lg[dst] = a.Eg[a.acc_pos[k]];
    }
}

}  // namespace tsc
