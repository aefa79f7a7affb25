// nci.hpp -- non-covalent interactions of a whole ensemble, one wavefront per structure: what tscode/nci.py computes per structure in
// Python loops (get_nci :28-52; _get_nci_atomic_pairs :54-89; _get_nci_aromatic_rings :91-139; _get_aromatic_centers :141-181, which
// calls is_phenyl, tscode/graph_manipulations.py:152-174, on every combination of 6 of a molecule's C/N atoms).
//
// The ring search is a different algorithm, not a port.  A 6-subset passes is_phenyl's distance test iff it is a 6-clique of the graph
// "distance not above 3 A" on the molecule's candidates; at most 64 candidates per molecule, so a row of that graph is one 64-bit word
// and a clique a < b < c < d < e < f is found by intersecting rows.  is_phenyl's flatness test reads the four LOWEST atoms only, so it
// is asked once per (a, b, c, d) that has a completion.
//
// Per structure (the structure staged in LDS by coalesced loads, lane l keeps atoms l, l + 64, ... in registers):
//   A  pairs.   Row atom i broadcast from LDS, lanes on the columns of LATER molecules (the atoms of a molecule are contiguous), d2 formed
//               with the reference's roundings (three products, two sums, no fused multiply-add: norm_of, tscode/algebra.py:90-96) and
//               compared with the squared bound of the class pair (clash_sq_bound: the verdict of sqrt-then-compare; 0 = never); rows
//               and columns of constrained atoms masked; one __ballot per 64 columns.
//   B  rings.   Per molecule with at least 6 candidates: lane k holds candidate k; near[k] by one ballot per candidate, kept in LDS.
//               Lane a enumerates the cliques whose lowest vertex is a, in nested ascending loops -- that IS the reference's order
//               (itertools.combinations is lexicographic in the atom index, the molecules are visited in order), so a count pass, an
//               exclusive scan of the counts over the lanes and a second pass that writes each ring to its slot give the list in
//               reference order with no sort and no atomic.  The count is exact whatever it is; slots exist for the first 64.
//               Flat iff 1 - |cos(dihedral)| < 1 - cos(10 deg) with |cos(atan2(y, x))| = |x| / sqrt(x x + y y) (x, y formed as
//               tscode/algebra.py:24-56 forms them); x = y = 0 is flat (atan2(0, 0) = 0), a NaN is not.  The two forms of the flatness
//               value differ by rounding only (1e-15); the fixtures keep 1e-9 clear of the bound.
//               Centre = (((((r0 + r1) + r2) + r3) + r4) + r5) / 6 per component, as np.mean(axis = 0) sums.
//   C  rings against atoms (one ballot per ring and 64 atoms, bound by the atom's class, the owner rule) and against later rings (lane s
//               holds ring s).  Constrained atoms are NOT masked here, as in the reference.
// A non-finite coordinate makes every d2 it enters NaN or +inf, which fails every `<` and `<=`: such an atom is in no pair and no ring.
//
// What bounds the kernel.  LDS: 2272 B of tables per block and 24 n + 2880 B per wavefront (the structure, near[64], 64 ring slots:
// centres, atoms, owners), 62 944 B at n = 512 -- under the 64 KiB a block gets without asking for more; everything is carved from the
// dynamic region at multiples of 16 B.  Time: phase A is n (W - w0) ballots of fp64 work like k_bond_delta; phase B costs 64 ballots per
// molecule plus the clique walk, which is lane-divergent integer work proportional to the number of 4-cliques with a completion -- a
// few hundred per aromatic molecule, but C(64, 6) = 7.5e7 if 64 candidates were put within 3 A of one another, which no molecule does
// (the call still ends, and the count is still exact: it fits 31 bits).  Registers: 3 W doubles per lane for the structure.
#pragma once

#include "common.hpp"

namespace tsc {

constexpr int NC_MAX_ATOMS = 512;
constexpr int NC_MAX_W = NC_MAX_ATOMS / 64;
constexpr int NC_MAX_CLASSES = 8;
constexpr int NC_TABLE = NC_MAX_CLASSES + 1;  // + the class of the lanes behind the last atom
constexpr int NC_MAX_MOLS = 8;
constexpr int NC_MAX_CAND = 64;               // ring candidates per molecule: one bit each
constexpr int NC_MAX_CON = 16;
constexpr int NC_MAX_RINGS = 64;              // ring slots per structure
constexpr double NC_RING_DIST = 3.0;          // is_phenyl: "if any atomic couple is more than 3 A away from each other, this is not a Ph"
constexpr double NC_FLAT_DEGREES = 10.0;      // is_phenyl: threshold_delta = 1 - cos(10 deg)

struct NciArgs {
    int64_t n_structs;
    int n;           // atoms per structure
    int n_tab;       // classes, the padding one (n_tab - 1) included
    int n_mols;
    int n_con;       // slots per structure of the per-structure constrained list (0: none)
    int owner_rule;  // 0: a ring meets every atom unless the ring's molecule is molecule 0 (tscode/nci.py:100-105 as written);
                     // 1: a ring meets the atoms of the other molecules (what the comment at :105-106 intends)
    double rr_bound, near_bound, flat_bound;
    uint64_t con_words[NC_MAX_W];        // atoms constrained in every structure, one bit each
    double bound[NC_TABLE * NC_TABLE];   // squared pair bounds by class pair
    double ring_bound[NC_TABLE];         // squared ring-centre-to-atom bounds by class
    int mol_end[NC_MAX_MOLS];            // one past the last atom of molecule m
    int cand_off[NC_MAX_MOLS + 1];       // the candidates of molecule m are cand[cand_off[m] .. cand_off[m + 1])
    uint8_t meta[NC_MAX_ATOMS];          // class | molecule << 4
    uint16_t cand[NC_MAX_ATOMS];         // ring candidates, ascending
};
static_assert(sizeof(NciArgs) <= 4096, "kernel arguments");

constexpr int NC_LDS_BOUND = 0, NC_LDS_RBOUND = 656, NC_LDS_META = 736, NC_LDS_CAND = 1248, NC_LDS_WAVES = 2272;
constexpr int NC_WAVE_NEAR = 0, NC_WAVE_CTR = 512, NC_WAVE_RATOMS = 2048, NC_WAVE_ROWNER = 2816, NC_WAVE_FIXED = 2880;

__host__ __device__ constexpr size_t nci_wave_coord_bytes(int n) { return (size_t(24) * n + 15) & ~size_t(15); }
__host__ __device__ constexpr size_t nci_lds_bytes(int n) { return NC_LDS_WAVES + 4 * (nci_wave_coord_bytes(n) + NC_WAVE_FIXED); }

__device__ inline uint64_t nci_above(int k) { return k >= 63 ? 0ull : ~0ull << (k + 1); }

// is_phenyl's flatness test on atoms p0 < p1 < p2 < p3 of the staged structure (dihedral, tscode/algebra.py:24-56)
__device__ inline bool nci_flat(const double *w, int p0, int p1, int p2, int p3, double flat_bound) {
#pragma clang fp contract(off)
    const double b0x = -1.0 * (w[3 * p1] - w[3 * p0]), b0y = -1.0 * (w[3 * p1 + 1] - w[3 * p0 + 1]), b0z = -1.0 * (w[3 * p1 + 2] - w[3 * p0 + 2]);
    double b1x = w[3 * p2] - w[3 * p1], b1y = w[3 * p2 + 1] - w[3 * p1 + 1], b1z = w[3 * p2 + 2] - w[3 * p1 + 2];
    const double b2x = w[3 * p3] - w[3 * p2], b2y = w[3 * p3 + 1] - w[3 * p2 + 1], b2z = w[3 * p3 + 2] - w[3 * p2 + 2];
    const double nb = sqrt(b1x * b1x + b1y * b1y + b1z * b1z);
    b1x /= nb, b1y /= nb, b1z /= nb;
    const double p = b0x * b1x + b0y * b1y + b0z * b1z;
    const double vx = b0x - p * b1x, vy = b0y - p * b1y, vz = b0z - p * b1z;
    const double q = b2x * b1x + b2y * b1y + b2z * b1z;
    const double ux = b2x - q * b1x, uy = b2y - q * b1y, uz = b2z - q * b1z;
    const double x = vx * ux + vy * uy + vz * uz;
    const double y = (b1y * vz - b1z * vy) * ux + (b1z * vx - b1x * vz) * uy + (b1x * vy - b1y * vx) * uz;
    if (x == 0.0 && y == 0.0) return true;
    return 1.0 - fabs(x) / sqrt(x * x + y * y) < flat_bound;  // (false for NaN)
}

// The rings (flat 6-cliques of near[]) whose lowest vertex is a, in lexicographic order.  EMIT false: their number.  EMIT true: they are
// written to slots base, base + 1, ... while a slot is left; the return value is again their number.
template <bool EMIT>
__device__ inline int nci_rings_of(int a, const uint64_t *near, const double *w, const uint16_t *cand, double flat_bound, int base, int owner,
                                   uint16_t *ratoms, uint8_t *rowner) {
    int cnt = 0;
    const uint64_t na = near[a] & nci_above(a);
    if (__popcll(na) < 5) return 0;
    for (uint64_t ib = na; ib; ib &= ib - 1) {
        const int b = __builtin_ctzll(ib);
        const uint64_t nab = na & near[b] & nci_above(b);
        if (__popcll(nab) < 4) continue;
        for (uint64_t ic = nab; ic; ic &= ic - 1) {
            const int c = __builtin_ctzll(ic);
            const uint64_t nabc = nab & near[c] & nci_above(c);
            if (__popcll(nabc) < 3) continue;
            for (uint64_t id = nabc; id; id &= id - 1) {
                const int d = __builtin_ctzll(id);
                const uint64_t nabcd = nabc & near[d] & nci_above(d);
                if (__popcll(nabcd) < 2) continue;
                int completions = 0;
                for (uint64_t ie = nabcd; ie; ie &= ie - 1) completions += __popcll(nabcd & near[__builtin_ctzll(ie)] & nci_above(__builtin_ctzll(ie)));
                if (completions == 0) continue;
                if (!nci_flat(w, cand[a], cand[b], cand[c], cand[d], flat_bound)) continue;
                if (!EMIT) {
                    cnt += completions;
                    continue;
                }
                for (uint64_t ie = nabcd; ie; ie &= ie - 1) {
                    const int e = __builtin_ctzll(ie);
                    for (uint64_t jf = nabcd & near[e] & nci_above(e); jf; jf &= jf - 1) {
                        const int slot = base + cnt;
                        ++cnt;
                        if (slot >= NC_MAX_RINGS) continue;
                        uint16_t *dst = ratoms + 6 * slot;
                        dst[0] = cand[a], dst[1] = cand[b], dst[2] = cand[c], dst[3] = cand[d], dst[4] = cand[e], dst[5] = cand[__builtin_ctzll(jf)];
                        rowner[slot] = uint8_t(owner);
                    }
                }
            }
        }
    }
    return cnt;
}

// W = ceil(n / 64).  con (optional) i32[n_structs][n_con]: atoms constrained in that structure only (anything outside 0 .. n-1: an
// unused slot).  counts i32[n_structs][4]: pairs, rings, ring-atom, ring-ring; overflow u8[n_structs]: more than 64 rings (the count is
// exact, the lists and the two ring counts cover the first 64).  Optional: pair_bits u64[n_structs][n][W], ring_atoms
// u16[n_structs][64][6], ring_owner u8[n_structs][64], ring_center f64[n_structs][64][3], ring_atom_bits u64[n_structs][64][W],
// ring_ring_bits u64[n_structs][64]; slots behind the last ring are written as zeros.
template <int W>
inline __global__ __launch_bounds__(256) void k_nci(NciArgs a, const double *__restrict__ coords, const int32_t *__restrict__ con,
                                              int32_t *__restrict__ counts, uint8_t *__restrict__ overflow, uint64_t *__restrict__ pair_bits,
                                              uint16_t *__restrict__ ring_atoms, uint8_t *__restrict__ ring_owner,
                                              double *__restrict__ ring_center, uint64_t *__restrict__ ring_atom_bits,
                                              uint64_t *__restrict__ ring_ring_bits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_nci[];
    double *s_bound = reinterpret_cast<double *>(s_nci + NC_LDS_BOUND);
    double *s_rbound = reinterpret_cast<double *>(s_nci + NC_LDS_RBOUND);
    uint8_t *s_meta = s_nci + NC_LDS_META;
    uint16_t *s_cand = reinterpret_cast<uint16_t *>(s_nci + NC_LDS_CAND);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = a.n, T = a.n_tab;
    for (int e = threadIdx.x; e < T * T; e += 256) s_bound[e] = a.bound[e];
    for (int e = threadIdx.x; e < T; e += 256) s_rbound[e] = a.ring_bound[e];
    for (int e = threadIdx.x; e < NC_MAX_ATOMS; e += 256) {
        s_meta[e] = e < n ? a.meta[e] : uint8_t(T - 1);
        s_cand[e] = a.cand[e];
    }
    __syncthreads();
    unsigned char *mine_lds = s_nci + NC_LDS_WAVES + size_t(wid) * (nci_wave_coord_bytes(n) + NC_WAVE_FIXED);
    double *w = reinterpret_cast<double *>(mine_lds);
    unsigned char *fixed = mine_lds + nci_wave_coord_bytes(n);
    uint64_t *s_near = reinterpret_cast<uint64_t *>(fixed + NC_WAVE_NEAR);
    double *s_ctr = reinterpret_cast<double *>(fixed + NC_WAVE_CTR);
    uint16_t *s_ratoms = reinterpret_cast<uint16_t *>(fixed + NC_WAVE_RATOMS);
    uint8_t *s_rowner = fixed + NC_WAVE_ROWNER;
    int cl[W], ml[W];
#pragma unroll
    for (int t = 0; t < W; ++t) cl[t] = s_meta[lane + 64 * t] & 15, ml[t] = s_meta[lane + 64 * t] >> 4;
    const int64_t waves_total = int64_t(gridDim.x) * 4;
    for (int64_t s = int64_t(blockIdx.x) * 4 + wid; s < a.n_structs; s += waves_total) {
        const double *src = coords + s * n * 3;
        for (int e = lane; e < 3 * n; e += 64) w[e] = src[e];
        for (int e = lane; e < 6 * NC_MAX_RINGS; e += 64) s_ratoms[e] = 0;
        for (int e = lane; e < 3 * NC_MAX_RINGS; e += 64) s_ctr[e] = 0.0;
        s_rowner[lane] = 0;
        // the constrained atoms of this structure as one bit each (wave-uniform)
        uint64_t exc[W];
#pragma unroll
        for (int t = 0; t < W; ++t) exc[t] = a.con_words[t];
        if (con) {
            for (int q = 0; q < a.n_con; ++q) {
                const int e = __builtin_amdgcn_readfirstlane(con[s * a.n_con + q]);  // (the same address in every lane)
#pragma unroll
                for (int t = 0; t < W; ++t)
                    if (e >= 64 * t && e < 64 * t + 64 && e < n) exc[t] |= 1ull << (e & 63);
            }
        }
        __builtin_amdgcn_wave_barrier();
        double x[W], y[W], z[W];
#pragma unroll
        for (int t = 0; t < W; ++t) {
            const int j = lane + 64 * t;
            const bool in = j < n;
            x[t] = in ? w[3 * j] : 0.0, y[t] = in ? w[3 * j + 1] : 0.0, z[t] = in ? w[3 * j + 2] : 0.0;
        }

        // ---- A: atomic pairs
        int n_pairs = 0;
#pragma unroll
        for (int tr = 0; tr < W; ++tr) {
            const int rows = min(64, n - 64 * tr);
            uint64_t mine[W];  // row 64 tr + lane, gathered for one store per row tile
#pragma unroll
            for (int t = 0; t < W; ++t) mine[t] = 0;
            for (int r = 0; r < rows; ++r) {
                const int i = 64 * tr + r;
                const int meta_i = __builtin_amdgcn_readfirstlane(int(s_meta[i]));
                const int start = a.mol_end[meta_i >> 4];  // the first atom of the next molecule
                if (start >= n || ((exc[tr] >> r) & 1ull)) continue;
                const double xi = w[3 * i], yi = w[3 * i + 1], zi = w[3 * i + 2];
                const double *brow = s_bound + (meta_i & 15) * T;
#pragma unroll
                for (int tc = 0; tc < W; ++tc) {
                    if (64 * tc + 64 <= start) continue;
                    double d2;
                    {
#pragma clang fp contract(off)
                        const double dx = xi - x[tc], dy = yi - y[tc], dz = zi - z[tc];
                        d2 = dx * dx + dy * dy + dz * dz;
                    }
                    uint64_t bits = __ballot(d2 < brow[cl[tc]]) & ~exc[tc];
                    if (start > 64 * tc) bits &= ~0ull << (start - 64 * tc);
                    n_pairs += __popcll(bits);
                    if (pair_bits && lane == r) mine[tc] = bits;
                }
            }
            if (pair_bits && lane < rows) {
                uint64_t *dst = pair_bits + (size_t(s) * n + 64 * tr + lane) * W;
#pragma unroll
                for (int t = 0; t < W; ++t) dst[t] = mine[t];
            }
        }

        // ---- B: rings
        int n_rings = 0;
        for (int m = 0; m < a.n_mols; ++m) {
            const int c0 = a.cand_off[m], nc = a.cand_off[m + 1] - c0;
            if (nc < 6) continue;
            const bool has = lane < nc;
            const int my_atom = has ? int(s_cand[c0 + lane]) : 0;
            const double cx = w[3 * my_atom], cy = w[3 * my_atom + 1], cz = w[3 * my_atom + 2];
            uint64_t my_near = 0;
            for (int q = 0; q < nc; ++q) {
                const int at = s_cand[c0 + q];
                double d2;
                {
#pragma clang fp contract(off)
                    const double dx = w[3 * at] - cx, dy = w[3 * at + 1] - cy, dz = w[3 * at + 2] - cz;
                    d2 = dx * dx + dy * dy + dz * dz;
                }
                const uint64_t word = __ballot(has && d2 <= a.near_bound);
                if (lane == q) my_near = word;
            }
            s_near[lane] = my_near;
            __builtin_amdgcn_wave_barrier();
            const int cnt = has ? nci_rings_of<false>(lane, s_near, w, s_cand + c0, a.flat_bound, 0, m, s_ratoms, s_rowner) : 0;
            int scan = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(scan, d);
                if (lane >= d) scan += up;
            }
            const int total = __shfl(scan, 63);
            const int base = n_rings + scan - cnt;
            if (cnt > 0 && base < NC_MAX_RINGS) nci_rings_of<true>(lane, s_near, w, s_cand + c0, a.flat_bound, base, m, s_ratoms, s_rowner);
            n_rings += total;
            __builtin_amdgcn_wave_barrier();  // the next molecule overwrites near[]
        }
        const int n_slots = min(n_rings, NC_MAX_RINGS);
        if (lane < n_slots) {
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int k = 0; k < 6; ++k) {
                const int at = s_ratoms[6 * lane + k];
                sx += w[3 * at], sy += w[3 * at + 1], sz += w[3 * at + 2];
            }
            s_ctr[3 * lane] = sx / 6.0, s_ctr[3 * lane + 1] = sy / 6.0, s_ctr[3 * lane + 2] = sz / 6.0;
        }
        __builtin_amdgcn_wave_barrier();

        // ---- C: rings against atoms, rings against later rings
        int n_ring_atom = 0, n_ring_ring = 0;
        const double lx = s_ctr[3 * lane], ly = s_ctr[3 * lane + 1], lz = s_ctr[3 * lane + 2];
        const int lown = s_rowner[lane];
        uint64_t my_rr = 0;
        for (int r = 0; r < n_slots; ++r) {
            const int own = __builtin_amdgcn_readfirstlane(int(s_rowner[r]));
            const double rx = s_ctr[3 * r], ry = s_ctr[3 * r + 1], rz = s_ctr[3 * r + 2];
            const bool open = a.owner_rule != 0 || own != 0;
            uint64_t my_word = 0;
#pragma unroll
            for (int t = 0; t < W; ++t) {
                double d2;
                {
#pragma clang fp contract(off)
                    const double dx = rx - x[t], dy = ry - y[t], dz = rz - z[t];
                    d2 = dx * dx + dy * dy + dz * dz;
                }
                const uint64_t bits = __ballot(open && d2 < s_rbound[cl[t]] && (a.owner_rule == 0 || ml[t] != own));
                n_ring_atom += __popcll(bits);
                if (lane == t) my_word = bits;
            }
            if (ring_atom_bits && lane < W) ring_atom_bits[(size_t(s) * NC_MAX_RINGS + r) * W + lane] = my_word;
            double d2;
            {
#pragma clang fp contract(off)
                const double dx = rx - lx, dy = ry - ly, dz = rz - lz;
                d2 = dx * dx + dy * dy + dz * dz;
            }
            const uint64_t rr = __ballot(lane > r && lane < n_slots && lown != own && d2 < a.rr_bound);
            n_ring_ring += __popcll(rr);
            if (lane == r) my_rr = rr;
        }
        if (ring_atom_bits)
            for (int e = n_slots * W + lane; e < NC_MAX_RINGS * W; e += 64) ring_atom_bits[size_t(s) * NC_MAX_RINGS * W + e] = 0;
        if (ring_ring_bits) ring_ring_bits[size_t(s) * NC_MAX_RINGS + lane] = my_rr;
        if (ring_atoms)
            for (int e = lane; e < 6 * NC_MAX_RINGS; e += 64) ring_atoms[size_t(s) * 6 * NC_MAX_RINGS + e] = s_ratoms[e];
        if (ring_owner) ring_owner[size_t(s) * NC_MAX_RINGS + lane] = uint8_t(lown);
        if (ring_center)
            for (int e = lane; e < 3 * NC_MAX_RINGS; e += 64) ring_center[size_t(s) * 3 * NC_MAX_RINGS + e] = s_ctr[e];
        if (lane == 0) {
            counts[4 * s] = n_pairs, counts[4 * s + 1] = n_rings, counts[4 * s + 2] = n_ring_atom, counts[4 * s + 3] = n_ring_ring;
            overflow[s] = uint8_t(n_rings > NC_MAX_RINGS ? 1 : 0);
        }
        __builtin_amdgcn_wave_barrier();  // the next structure overwrites this wavefront's LDS
    }
}

}  // namespace tsc
