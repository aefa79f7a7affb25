// torsions.hpp -- what the set-up of a conformational search asks of every pose, one wavefront per structure (or per chunk of the
// candidate torsions of one topology class).
//
// What the reference does per TS candidate in Python loops (tscode/torsion_module.py:559-615): _get_hydrogen_bonds (:233-299, a
// double loop over the N / O pairs), the connected-components verdict of csearch (:581-604), and per candidate torsion three graph
// searches with the central bond taken out: Torsion.in_cycle (:54-61, nx.has_path), Torsion.sort_torsion (:120-132, one nx.has_path
// per constrained atom) and _get_rotation_mask (:301-325, nx.shortest_path).
//
// Shape of both kernels: the structure's graph is staged in LDS as a SYMMETRIC bit matrix, word w of atom j at adj[w * 64 W + j]
// (consecutive lanes read consecutive words: no bank conflict), built from the strict upper triangle the bond kernel writes with
// one ds_or per word and per set bit.  Lane l owns atoms l, l + 64, ...
//
// The search is a pull-style bit-set frontier: the reached set R is W wave-uniform words; in one sweep every lane asks, for each
// of its atoms not yet in R, whether its row meets R (W and-s), and one __ballot per 64 atoms gives the atoms that join.  A sweep
// that adds nothing ends the search, every other sweep adds at least one atom: at most n sweeps of W * W LDS reads per lane, and
// as many sweeps as the graph's eccentricity from the source in practice (words are updated in place, so a sweep also uses what
// it has just found in lower tiles).  The cut edge i2 - i3 of a torsion is taken out of the two rows it touches as they are read.
//
// LDS per wavefront and the block shape per W = ceil(n / 64):
//   adjacency 512 W^2 bytes (W = 4: 8 KiB, W = 8: 32 KiB); k_hbonds adds the pose (24 n bytes) and a component label per atom (2 n).
//   W <= 4: four wavefronts per block (256 threads; k_torsion_reach <= 32 KiB, k_hbonds <= 60 KiB per block);
//   W >= 5: one wavefront per block (64 threads; <= 32 KiB resp. <= 45 KiB), so that three to five blocks share a CU's 160 KiB
//           where four such wavefronts in one block (128 KiB and more) would leave it to a single block.
// No launch asks for more than 64 KiB.
#pragma once

#include "common.hpp"

namespace tsc {

constexpr int TOR_MAX_ATOMS = 512;
constexpr int TOR_MAX_W = TOR_MAX_ATOMS / 64;
constexpr int TOR_MAX_EXTRA = 64;   // constraint pairs per structure (one bit each in a wave-uniform word)
constexpr int TOR_CHUNK = 8;        // candidate torsions one wavefront takes after staging a class graph
constexpr int TOR_MODE_ALL = 0, TOR_MODE_LINK = 1;

__host__ __device__ inline int tor_waves_per_block(int W) { return W <= 4 ? 4 : 1; }
__host__ __device__ inline size_t tor_adj_bytes(int W) { return size_t(512) * W * W; }
__host__ __device__ inline size_t hbonds_wave_bytes(int n, int W) { return tor_adj_bytes(W) + size_t(24) * n + ((size_t(2) * n + 15) & ~size_t(15)); }

struct HbArgs {
    int64_t n_structs;
    int n;
    int n_extra;   // constraint pairs per structure
    int mode;      // TOR_MODE_ALL: every hetero pair; TOR_MODE_LINK: only when segmented, only pairs across components
    int max_hb;    // slots per structure of the pair list
    double lo_sq;  // d_min < sqrt(d2)  <=>  d2 > lo_sq
    double hi_sq;  // sqrt(d2) < d_max  <=>  d2 < hi_sq
    double max_angle;                  // degrees
    uint64_t het[TOR_MAX_W];           // N / O atoms, one bit each
    uint64_t hyd[TOR_MAX_W];           // H atoms
};

// ---- the symmetric bit matrix of one wavefront ------------------------------------------------------------------------------------
template <int W>
__device__ inline void adj_set_edge(unsigned long long *adj, int a, int b) {   // (every lane writes the same two words)
    constexpr int NP = 64 * W;
    adj[(b >> 6) * NP + a] |= 1ull << (b & 63);
    adj[(a >> 6) * NP + b] |= 1ull << (a & 63);
}

// adj <- the symmetric closure of upper u64[n][W]; bits at or left of the diagonal and behind atom n - 1 are ignored
template <int W>
__device__ inline void adj_stage(unsigned long long *adj, const uint64_t *__restrict__ upper, int n, int lane) {
    constexpr int NP = 64 * W;
    for (int e = lane; e < W * NP; e += 64) adj[e] = 0ull;
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < n * W; e += 64) {
        const int i = e / W, w = e - i * W;
        unsigned long long bits = upper[e];
        const int lo = i + 1 - 64 * w, hi = n - 64 * w;   // columns lo .. hi - 1 of this word are real
        if (lo >= 64 || hi <= 0) continue;
        if (lo > 0) bits &= ~0ull << lo;
        if (hi < 64) bits &= ~(~0ull << hi);
        if (!bits) continue;
        atomicOr(&adj[w * NP + i], bits);
        while (bits) {
            const int j = 64 * w + __builtin_ctzll(bits);
            bits &= bits - 1;
            atomicOr(&adj[(i >> 6) * NP + j], 1ull << (i & 63));
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// rows that hold one-directional bits (bit k of row j without bit j of row k) made symmetric
template <int W>
__device__ inline void adj_symmetrise(unsigned long long *adj, int n, int lane) {
    constexpr int NP = 64 * W;
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < n * W; e += 64) {
        const int j = e / W, w = e - j * W;
        unsigned long long bits = adj[w * NP + j];
        while (bits) {
            const int k = 64 * w + __builtin_ctzll(bits);
            bits &= bits - 1;
            if (k < n) atomicOr(&adj[(j >> 6) * NP + k], 1ull << (j & 63));
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// R <- the atoms reachable from src with the edge cut_a - cut_b taken out (-1, -1: no cut).  Wave-uniform in and out.
template <int W>
__device__ inline void adj_reach(const unsigned long long *adj, int n, int lane, int src, int cut_a, int cut_b, uint64_t (&R)[W]) {
    constexpr int NP = 64 * W;
#pragma unroll
    for (int t = 0; t < W; ++t) R[t] = (src >> 6) == t ? 1ull << (src & 63) : 0ull;
    for (int sweep = 0; sweep < n; ++sweep) {   // (a sweep that adds nothing ends the search; each other one adds an atom)
        bool grew = false;
#pragma unroll
        for (int t = 0; t < W; ++t) {
            const int j = lane + 64 * t;
            bool hit = false;
            if (j < n && !((R[t] >> lane) & 1ull)) {
                const int other = j == cut_a ? cut_b : (j == cut_b ? cut_a : -1);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    unsigned long long row = adj[w * NP + j];
                    if (other >= 0 && (other >> 6) == w) row &= ~(1ull << (other & 63));
                    hit = hit || (row & R[w]) != 0ull;
                }
            }
            const uint64_t joined = __ballot(hit);
            R[t] |= joined;
            grew = grew || joined != 0ull;
        }
        if (!grew) break;
    }
}

// the number of connected components; comp (optional, LDS u16[n]) receives the component of every atom
template <int W>
__device__ inline int adj_components(const unsigned long long *adj, int n, int lane, unsigned short *comp) {
    uint64_t seen[W];
#pragma unroll
    for (int t = 0; t < W; ++t) seen[t] = 0ull;
    int n_comp = 0;
    for (;;) {
        int src = -1;
#pragma unroll
        for (int t = W - 1; t >= 0; --t) {
            const int rest = n - 64 * t;   // atoms of this word
            const uint64_t open = ~seen[t] & (rest >= 64 ? ~0ull : (rest <= 0 ? 0ull : ~(~0ull << rest)));
            if (open) src = 64 * t + __builtin_ctzll(open);   // (the lowest atom not yet in a component)
        }
        if (src < 0) break;
        uint64_t R[W];
        adj_reach<W>(adj, n, lane, src, -1, -1, R);
#pragma unroll
        for (int t = 0; t < W; ++t) {
            if (comp && ((R[t] >> lane) & 1ull)) comp[lane + 64 * t] = (unsigned short)n_comp;
            seen[t] |= R[t];
        }
        ++n_comp;
    }
    __builtin_amdgcn_wave_barrier();
    return n_comp;
}

// ---- hydrogen bonds and the search graph -----------------------------------------------------------------------------------------
// tscode/torsion_module.py:233-299 and :559-606; the semantics are spelled out at tsc_hbonds in include/tscode_hip.h.
// bonds u64[S][n][W] strict upper triangle; extra (optional) i32[S][n_extra][2], a pair with an index outside 0 .. n-1 or with two
// equal indices is an unused slot; hb (optional when max_hb == 0) i32[S][max_hb][2]; n_hb i32[S]; status u8[S]; n_before
// (optional) i32[S]; graph (optional) u64[S][n][W].
template <int W, int WPB>
inline __global__ __launch_bounds__(64 * WPB) void k_hbonds(HbArgs a, const double *__restrict__ coords, const uint64_t *__restrict__ bonds,
                                                            const int32_t *__restrict__ extra, int32_t *__restrict__ hb,
                                                            int32_t *__restrict__ n_hb, uint8_t *__restrict__ status,
                                                            int32_t *__restrict__ n_before, uint64_t *__restrict__ graph) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    constexpr int NP = 64 * W;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = a.n;
    unsigned char *base = s_raw + size_t(wid) * hbonds_wave_bytes(n, W);
    unsigned long long *adj = reinterpret_cast<unsigned long long *>(base);
    double *xyz = reinterpret_cast<double *>(base + tor_adj_bytes(W));
    unsigned short *comp = reinterpret_cast<unsigned short *>(base + tor_adj_bytes(W) + size_t(24) * n);
    const int64_t waves_total = int64_t(gridDim.x) * WPB;
    for (int64_t s = int64_t(blockIdx.x) * WPB + wid; s < a.n_structs; s += waves_total) {
        const double *src = coords + s * n * 3;
        for (int e = lane; e < 3 * n; e += 64) xyz[e] = src[e];
        adj_stage<W>(adj, bonds + size_t(s) * n * W, n, lane);
        // the constraint pairs, in the caller's order; bit q of fresh: pair q was not an edge yet (it then follows the bonded
        // atoms in the neighbour lists of its two atoms)
        const int32_t *ex = extra ? extra + s * a.n_extra * 2 : nullptr;
        uint64_t fresh = 0ull;
        for (int q = 0; q < a.n_extra; ++q) {
            const int ea = __builtin_amdgcn_readfirstlane(ex[2 * q]), eb = __builtin_amdgcn_readfirstlane(ex[2 * q + 1]);
            if (ea < 0 || eb < 0 || ea >= n || eb >= n || ea == eb) continue;
            if (!((adj[(eb >> 6) * NP + ea] >> (eb & 63)) & 1ull)) {
                fresh |= 1ull << q;
                adj_set_edge<W>(adj, ea, eb);
            }
        }
        __builtin_amdgcn_wave_barrier();
        const int n_comp0 = adj_components<W>(adj, n, lane, comp);
        const bool search = a.mode == TOR_MODE_ALL || n_comp0 > 1;
        const bool across = a.mode != TOR_MODE_ALL;
        int found = 0;
        if (search) {
            double x[W], y[W], z[W];
#pragma unroll
            for (int t = 0; t < W; ++t) {
                const int j = lane + 64 * t;
                const bool in = j < n;
                x[t] = in ? xyz[3 * j] : 0.0, y[t] = in ? xyz[3 * j + 1] : 0.0, z[t] = in ? xyz[3 * j + 2] : 0.0;
            }
            for (int t1 = 0; t1 < W; ++t1) {
                for (uint64_t het1 = a.het[t1]; het1; het1 &= het1 - 1) {
                    const int i1 = 64 * t1 + __builtin_ctzll(het1);
                    if (i1 >= n) break;
                    const double x1 = xyz[3 * i1], y1 = xyz[3 * i1 + 1], z1 = xyz[3 * i1 + 2];
                    const int c1 = comp[i1];
#pragma unroll
                    for (int tc = 0; tc < W; ++tc) {
                        if (tc < t1) continue;
                        const int j = lane + 64 * tc;
                        double d2;
                        {
#pragma clang fp contract(off)
                            const double dx = x1 - x[tc], dy = y1 - y[tc], dz = z1 - z[tc];
                            d2 = dx * dx + dy * dy + dz * dz;
                        }
                        bool q = j < n && j > i1 && ((a.het[tc] >> lane) & 1ull) && d2 > a.lo_sq && d2 < a.hi_sq;
                        if (q && across) q = comp[j] != c1;
                        for (uint64_t cand = __ballot(q); cand; cand &= cand - 1) {
                            const int i2 = 64 * tc + __builtin_ctzll(cand);
                            // ---- one hetero pair in range: its candidate hydrogens in list order, the first that passes decides
                            const double x2 = xyz[3 * i2], y2 = xyz[3 * i2 + 1], z2 = xyz[3 * i2 + 2];
                            double ux, uy, uz;
                            {
#pragma clang fp contract(off)
                                const double dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
                                const double len = sqrt(dx * dx + dy * dy + dz * dz);
                                ux = dx / len, uy = dy / len, uz = dz / len;
                            }
                            int hit_h = -1, hit_x = -1;
                            for (int side = 0; side < 2 && hit_h < 0; ++side) {
                                const int xa = side == 0 ? i1 : i2;
                                // walk 0 .. W-1: the bonded hydrogens of xa in ascending order (the row without its fresh constraint
                                // partners); walk W: those partners in the caller's order
                                uint64_t not_bonded[W];
#pragma unroll
                                for (int w = 0; w < W; ++w) not_bonded[w] = 0ull;
                                for (uint64_t f = fresh; f; f &= f - 1) {
                                    const int q2 = __builtin_ctzll(f);
                                    const int ea = __builtin_amdgcn_readfirstlane(ex[2 * q2]), eb = __builtin_amdgcn_readfirstlane(ex[2 * q2 + 1]);
                                    const int p = ea == xa ? eb : (eb == xa ? ea : -1);
#pragma unroll
                                    for (int w = 0; w < W; ++w)
                                        if (p >= 0 && (p >> 6) == w) not_bonded[w] |= 1ull << (p & 63);
                                }
                                uint64_t f = fresh;
                                int w = 0;
                                uint64_t hs = 0ull;
                                bool have_row = false;
                                for (;;) {
                                    int iH = -1;
                                    if (w < W) {
                                        if (!have_row) {
                                            uint64_t nb = 0ull, hy = 0ull;
#pragma unroll
                                            for (int ww = 0; ww < W; ++ww)
                                                if (ww == w) nb = not_bonded[ww], hy = a.hyd[ww];
                                            hs = adj[w * NP + xa] & ~nb & hy;
                                            have_row = true;
                                        }
                                        if (!hs) {
                                            ++w, have_row = false;
                                            continue;
                                        }
                                        iH = 64 * w + __builtin_ctzll(hs);
                                        hs &= hs - 1;
                                        if (iH >= n) continue;
                                    } else {
                                        if (!f) break;
                                        const int q2 = __builtin_ctzll(f);
                                        f &= f - 1;
                                        const int ea = __builtin_amdgcn_readfirstlane(ex[2 * q2]), eb = __builtin_amdgcn_readfirstlane(ex[2 * q2 + 1]);
                                        const int p = ea == xa ? eb : (eb == xa ? ea : -1);
                                        if (p < 0) continue;
                                        bool is_h = false;
#pragma unroll
                                        for (int ww = 0; ww < W; ++ww)
                                            if ((p >> 6) == ww) is_h = (a.hyd[ww] >> (p & 63)) & 1ull;
                                        if (!is_h) continue;
                                        iH = p;
                                    }
                                    // :273-297
                                    const double hx = xyz[3 * iH], hy_ = xyz[3 * iH + 1], hz = xyz[3 * iH + 2];
                                    double alfa, d1, d2h;
                                    {
#pragma clang fp contract(off)
                                        const double v1x = hx - x1, v1y = hy_ - y1, v1z = hz - z1;
                                        const double v2x = hx - x2, v2y = hy_ - y2, v2z = hz - z2;
                                        d1 = sqrt(v1x * v1x + v1y * v1y + v1z * v1z);
                                        d2h = sqrt(v2x * v2x + v2y * v2y + v2z * v2z);
                                        const double l1 = v1x * ux + v1y * uy + v1z * uz;
                                        const double l2 = v2x * -ux + v2y * -uy + v2z * -uz;
                                        const bool first = l1 < l2;
                                        const double ax = first ? v1x : v2x, ay = first ? v1y : v2y, az = first ? v1z : v2z, al = first ? d1 : d2h;
                                        const double bx = first ? ux : -ux, by = first ? uy : -uy, bz = first ? uz : -uz;
                                        const double bl = sqrt(bx * bx + by * by + bz * bz);   // (vec_angle normalises the versor again)
                                        double c = (ax / al) * (bx / bl) + (ay / al) * (by / bl) + (az / al) * (bz / bl);
                                        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
                                        alfa = acos(c) * 180.0 / 3.141592653589793;
                                    }
                                    if (alfa < a.max_angle) {
                                        hit_h = iH, hit_x = d1 < d2h ? i2 : i1;
                                        break;
                                    }
                                }
                            }
                            if (hit_h >= 0) {
                                if (found < a.max_hb && lane == 0) {
                                    int32_t *dst = hb + (s * a.max_hb + found) * 2;
                                    dst[0] = min(hit_h, hit_x), dst[1] = max(hit_h, hit_x);
                                }
                                ++found;
                                // kept one-directional, in the hydrogen's row, until the search is over: the rows of the hetero atoms
                                // are what the neighbour lists above are read from, and the reference adds its pairs afterwards
                                adj[(hit_x >> 6) * NP + hit_h] |= 1ull << (hit_x & 63);
                            }
                        }
                    }
                }
            }
        }
        int n_comp1 = n_comp0;
        if (found) {
            adj_symmetrise<W>(adj, n, lane);
            n_comp1 = adj_components<W>(adj, n, lane, nullptr);
        }
        if (graph) {
#pragma unroll
            for (int t = 0; t < W; ++t) {
                const int i = lane + 64 * t;
                if (i >= n) continue;
                uint64_t *dst = graph + (size_t(s) * n + i) * W;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    unsigned long long bits = adj[w * NP + i];
                    const int lo = i + 1 - 64 * w, hi = n - 64 * w;
                    if (lo >= 64 || hi <= 0) bits = 0ull;
                    else {
                        if (lo > 0) bits &= ~0ull << lo;
                        if (hi < 64) bits &= ~(~0ull << hi);
                    }
                    dst[w] = bits;
                }
            }
        }
        if (lane == 0) {
            n_hb[s] = found;
            status[s] = uint8_t(n_comp1 > 1 ? 1 : 0);   // (segmented before and nothing found: n_comp1 == n_comp0 > 1)
            if (n_before) n_before[s] = n_comp0;
        }
        __builtin_amdgcn_wave_barrier();   // the next structure overwrites this wavefront's LDS
    }
}

// ---- reachability per (class graph, candidate torsion) ------------------------------------------------------------------------------
// tscode/torsion_module.py:54-61, :120-132, :301-325.  graph u64[G][n][W]; torsions i32[T][4]; items i32[n_items][3] = (class,
// first torsion, torsions) with at most TOR_CHUNK torsions each; constrained (optional) i32[G][n_con], an entry outside 0 .. n-1
// is an unused slot; flags u8[T]: bit 0 in_cycle, bit 1 reversed; masks u8[T][n].  A torsion with an index outside 0 .. n-1 or
// with i2 == i3 (only the _dev form can meet one: the host-array form refuses it) gets flags 0x80 and a zero mask.
template <int W, int WPB>
inline __global__ __launch_bounds__(64 * WPB) void k_torsion_reach(int n, int64_t n_items, const int32_t *__restrict__ items,
                                                                   const uint64_t *__restrict__ graph, const int32_t *__restrict__ torsions,
                                                                   const int32_t *__restrict__ constrained, int n_con,
                                                                   uint8_t *__restrict__ flags, uint8_t *__restrict__ masks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long *adj = reinterpret_cast<unsigned long long *>(s_raw + size_t(wid) * tor_adj_bytes(W));
    const int64_t waves_total = int64_t(gridDim.x) * WPB;
    int staged = -1;
    for (int64_t it = int64_t(blockIdx.x) * WPB + wid; it < n_items; it += waves_total) {
        const int g = __builtin_amdgcn_readfirstlane(items[3 * it]), t0 = __builtin_amdgcn_readfirstlane(items[3 * it + 1]),
                  nt = __builtin_amdgcn_readfirstlane(items[3 * it + 2]);
        if (g != staged) {
            __builtin_amdgcn_wave_barrier();
            adj_stage<W>(adj, graph + size_t(g) * n * W, n, lane);
            staged = g;
        }
        for (int k = 0; k < nt; ++k) {
            const int64_t t = int64_t(t0) + k;
            const int i1 = __builtin_amdgcn_readfirstlane(torsions[4 * t]), i2 = __builtin_amdgcn_readfirstlane(torsions[4 * t + 1]),
                      i3 = __builtin_amdgcn_readfirstlane(torsions[4 * t + 2]), i4 = __builtin_amdgcn_readfirstlane(torsions[4 * t + 3]);
            uint8_t *mrow = masks + t * n;
            if (i1 < 0 || i2 < 0 || i3 < 0 || i4 < 0 || i1 >= n || i2 >= n || i3 >= n || i4 >= n || i2 == i3) {
                for (int j = lane; j < n; j += 64) mrow[j] = 0;
                if (lane == 0) flags[t] = 0x80;
                continue;
            }
            uint64_t R1[W], R2[W], RM[W];
            adj_reach<W>(adj, n, lane, i1, i2, i3, R1);
            auto holds = [](const uint64_t(&R)[W], int atom) {
                bool in = false;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if ((atom >> 6) == w) in = (R[w] >> (atom & 63)) & 1ull;
                return in;
            };
            const bool in_cycle = holds(R1, i4);
            if (holds(R1, i2)) {
#pragma unroll
                for (int w = 0; w < W; ++w) R2[w] = R1[w];
            } else {
                adj_reach<W>(adj, n, lane, i2, i2, i3, R2);
            }
            int n_reached = 0;   // entries of the constrained list reachable from i2, duplicates counted: one flip each
            for (int q = 0; q < n_con; ++q) {
                const int d = __builtin_amdgcn_readfirstlane(constrained[size_t(g) * n_con + q]);
                if (d >= 0 && d < n && holds(R2, d)) ++n_reached;
            }
            const bool reversed = n_reached & 1;
            const int from = reversed ? i4 : i1, axis = reversed ? i3 : i2;
            if (!reversed || holds(R1, i4)) {
#pragma unroll
                for (int w = 0; w < W; ++w) RM[w] = R1[w];
            } else if (holds(R2, i4)) {
#pragma unroll
                for (int w = 0; w < W; ++w) RM[w] = R2[w];
            } else {
                adj_reach<W>(adj, n, lane, from, i2, i3, RM);
            }
            int moved = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) moved += __popcll(RM[w]);
            const bool invert = moved > n / 2;
#pragma unroll
            for (int tt = 0; tt < W; ++tt) {
                const int j = lane + 64 * tt;
                if (j >= n) continue;
                bool m = (RM[tt] >> lane) & 1ull;
                if (invert) m = !m;
                if (j == axis || in_cycle) m = false;
                mrow[j] = uint8_t(m ? 1 : 0);
            }
            if (lane == 0) flags[t] = uint8_t((in_cycle ? 1 : 0) | (reversed ? 2 : 0));
        }
    }
}

// ---- which torsions turn together ------------------------------------------------------------------------------------------------
// tscode/torsion_module.py:373-397 (_group_torsions_dbscan) and the T < 9 branch of :689; the semantics are spelled out at
// tsc_torsion_groups in include/tscode_hip.h.  One wavefront per structure, one wavefront per block; lane l owns torsions l, l + 64, ...
// (K = ceil(T_max / 64) of them, centres and labels in registers).  LDS: the centres as three f64[T_max] and label, count and position
// as three i32[T_max] -- 36 T_max bytes, 18 KiB at 512 torsions.
//
// The clusters of one level are the connected components of "centres at most eps apart".  Every torsion starts as its own label; a
// sweep gives it the smallest label among the torsions it is linked to (every lane walks all T centres, which all lanes read at the
// same address: a broadcast), then follows the labels down to one that points at itself.  A label is always the index of a member of
// the torsion's own component and never grows, so the sweeps end -- when one changes nothing -- with every torsion carrying the
// smallest index of its component.  Thanks to the second step a line of T centres closes in a few sweeps, not in T.
constexpr int GRP_MAX_TORSIONS = 512;
constexpr int GRP_LEVELS = 17;   // 10.0, 9.5, ..., 2.0 (np.arange(10, 1.5, -0.5))

__host__ __device__ inline size_t groups_lds_bytes(int t_max) { return size_t(36) * t_max; }

template <int K>
inline __global__ __launch_bounds__(64) void k_torsion_groups(int n_structs, int n, int t_max, const double *__restrict__ coords,
                                                              const int32_t *__restrict__ torsions, const int32_t *__restrict__ set_off,
                                                              int max_size, int min_torsions, int32_t *__restrict__ group_of,
                                                              int32_t *__restrict__ n_groups, int32_t *__restrict__ eps_index,
                                                              uint8_t *__restrict__ oversize) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double *cx = reinterpret_cast<double *>(s_raw), *cy = cx + t_max, *cz = cy + t_max;
    int *label = reinterpret_cast<int *>(cz + t_max), *count = label + t_max, *pos = count + t_max;
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < n_structs; s += gridDim.x) {
        const int t0 = __builtin_amdgcn_readfirstlane(set_off[s]);
        const int T = min(__builtin_amdgcn_readfirstlane(set_off[s + 1]) - t0, 64 * K);   // (the host refused more than t_max)
        if (T < min_torsions || T <= 0) {
            for (int t = lane; t < T; t += 64) group_of[t0 + t] = 0;
            if (lane == 0) n_groups[s] = T > 0 ? 1 : 0, eps_index[s] = -1, oversize[s] = 0;
            continue;
        }
        // ---- centres (:379); a torsion with an atom outside 0 .. n-1 (only the _dev form can meet one) gets NaN: linked to nothing
        const double *xyz = coords + size_t(s) * n * 3;
        double x[K], y[K], z[K];
        int my[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = lane + 64 * k;
            x[k] = y[k] = z[k] = __builtin_nan("");
            if (t < T) {
                const int i2 = torsions[4 * size_t(t0 + t) + 1], i3 = torsions[4 * size_t(t0 + t) + 2];
                if (i2 >= 0 && i2 < n && i3 >= 0 && i3 < n) {
                    x[k] = (xyz[3 * i2] + xyz[3 * i3]) / 2.0, y[k] = (xyz[3 * i2 + 1] + xyz[3 * i3 + 1]) / 2.0;
                    z[k] = (xyz[3 * i2 + 2] + xyz[3 * i3 + 2]) / 2.0;
                }
                cx[t] = x[k], cy[t] = y[k], cz[t] = z[k];
            }
        }
        int level = 0, biggest = 0;
        for (;; ++level) {
            const double eps = 10.0 - 0.5 * level, eps_sq = eps * eps;   // (a multiple of 0.5: the square is exact)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                my[k] = lane + 64 * k;
                if (my[k] < T) label[my[k]] = my[k];
            }
            __builtin_amdgcn_wave_barrier();
            for (;;) {
                bool changed = false;
                for (int u = 0; u < T; ++u) {
                    const double ux = cx[u], uy = cy[u], uz = cz[u];
                    const int lu = label[u];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
#pragma clang fp contract(off)
                        const double dx = x[k] - ux, dy = y[k] - uy, dz = z[k] - uz;
                        if (dx * dx + dy * dy + dz * dz <= eps_sq && lu < my[k]) my[k] = lu, changed = true;   // (NaN: never)
                    }
                }
                if (!__ballot(changed)) break;
                // the sweep read the labels of the sweep before; now they move, and then every torsion follows them down
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (lane + 64 * k < T) label[lane + 64 * k] = my[k];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (lane + 64 * k < T) {
                        int l = my[k];
                        for (int up = label[l]; up < l; up = label[l]) l = up;
                        my[k] = l;
                    }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (lane + 64 * k < T) label[lane + 64 * k] = my[k];
                __builtin_amdgcn_wave_barrier();
            }
            // ---- members per cluster, kept at the cluster's smallest member, and the largest cluster (:385)
            for (int t = lane; t < T; t += 64) count[t] = 0;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (lane + 64 * k < T) atomicAdd(&count[my[k]], 1);
            __builtin_amdgcn_wave_barrier();
            biggest = 0;
            for (int t = lane; t < T; t += 64) biggest = max(biggest, count[t]);
            for (int off = 32; off > 0; off >>= 1) biggest = max(biggest, __shfl_xor(biggest, off));
            if (biggest <= max_size || level == GRP_LEVELS - 1) break;   // (:387; no level qualifies: the last one stands)
        }
        // ---- sorted(output, key=len) (:394): a cluster's place is the number of clusters that are smaller, or as large with a smaller
        // first member -- dbscan numbers its clusters by first member, and the sort is stable
        int n_clusters = 0;
        for (int t = lane; t < T; t += 64) {
            if (label[t] != t) continue;
            const int mine = count[t];
            int before = 0;
            for (int u = 0; u < T; ++u)
                if (label[u] == u && (count[u] < mine || (count[u] == mine && u < t))) ++before;
            pos[t] = before;
            ++n_clusters;
        }
        for (int off = 32; off > 0; off >>= 1) n_clusters += __shfl_xor(n_clusters, off);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (lane + 64 * k < T) group_of[t0 + lane + 64 * k] = pos[my[k]];
        if (lane == 0) n_groups[s] = n_clusters, eps_index[s] = level, oversize[s] = uint8_t(biggest > max_size ? 1 : 0);
        __builtin_amdgcn_wave_barrier();   // the next structure overwrites this wavefront's LDS
    }
}

}  // namespace tsc
