// orbitals.hpp -- reactive-atom orbitals and pivots of every conformer of a molecule (include/tscode_hip.h: tsc_orbitals), one lane per
// conformer.  What the reference does per conformer and per reactive atom in Python -- Hypermolecule.compute_orbitals
// (tscode/hypermolecule_class.py:195-217), the init(update=True) of the eight classes of tscode/reactive_atoms_classes.py,
// is_sigmatropic's distance test (tscode/graph_manipulations.py:256) and Embedder._get_pivots / _set_pivots (tscode/embedder.py:542-621)
// -- is fp64 vector algebra on at most a dozen gathered atoms.  Everything that needs the bond graph is in the recipe the host built from
// conformer 0 (tscode_amd/reactive_atoms.py); the class of a recipe is the same for every lane, so a wavefront diverges only where
// conformers decide differently: sp against bent carbene, sigmatropic or not, how many pivots survive.
// No LDS; a lane writes its lobes as it forms them and reads those of the first two reactive atoms back from its own rows for the pivots.
#pragma once

#include "common.hpp"

namespace tsc {

constexpr int OB_MAX_REACTIVE = TSC_ORB_MAX_REACTIVE;
constexpr int OB_LOBES = TSC_ORB_MAX_LOBES;
constexpr int OB_PIVOTS = TSC_ORB_MAX_PIVOTS;
constexpr int OB_ANGLES = 8;   // the rotation angles the classes use, in degrees: 0 60 90 120 180 240 270 300
enum { OB_A0 = 0, OB_A60, OB_A90, OB_A120, OB_A180, OB_A240, OB_A270, OB_A300 };

using OrbRecipe = tsc_orbital_recipe;   // (include/tscode_hip.h, field by field)

struct OrbArgs {
    int64_t n_conf;
    int32_t n_atoms, n_reactive;
    int32_t sigma_mode;     // 0 never sigmatropic, 1 where the two reactive atoms are closer than 3 A, 2 always
    int32_t suprafacial, sigmastar, want_pivots;
    double half_sin[OB_ANGLES], half_cos[OB_ANGLES];   // sin / cos of half of each angle of OB_A*, formed on the host as the reference forms them
    OrbRecipe rec[OB_MAX_REACTIVE];
};

struct V3 {
    double x, y, z;
};
struct M3 {
    double m[3][3];
};

__host__ __device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__host__ __device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__host__ __device__ __forceinline__ V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__host__ __device__ __forceinline__ V3 operator/(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__host__ __device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ __forceinline__ double norm_of(V3 a) { return sqrt(dot(a, a)); }       // tscode/algebra.py:90-96
__host__ __device__ __forceinline__ V3 unit(V3 a) { return a / sqrt(dot(a, a)); }           // tscode/algebra.py:81-87 (norm)
__host__ __device__ __forceinline__ V3 reject(V3 v, V3 axis) { return v - axis * dot(v, axis); }   // v - v @ axis * axis

__host__ __device__ __forceinline__ V3 apply(const M3 &r, V3 v) {
    return {r.m[0][0] * v.x + r.m[0][1] * v.y + r.m[0][2] * v.z, r.m[1][0] * v.x + r.m[1][1] * v.y + r.m[1][2] * v.z,
            r.m[2][0] * v.x + r.m[2][1] * v.y + r.m[2][2] * v.z};
}

__host__ __device__ __forceinline__ M3 matmul(const M3 &a, const M3 &b) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return c;
}

// rot_mat_from_pointer (tscode/algebra.py:326-344) with quaternion_to_rotation_matrix (:285-323): s, c = sin, cos of half the angle
__host__ __device__ __forceinline__ M3 rot_about(V3 pointer, double s, double c) {
    const V3 p = unit(pointer);
    const double q0 = c, q1 = s * p.x, q2 = s * p.y, q3 = s * p.z;
    M3 r;
    r.m[0][0] = 2 * (q0 * q0 + q1 * q1) - 1, r.m[0][1] = 2 * (q1 * q2 - q0 * q3), r.m[0][2] = 2 * (q1 * q3 + q0 * q2);
    r.m[1][0] = 2 * (q1 * q2 + q0 * q3), r.m[1][1] = 2 * (q0 * q0 + q2 * q2) - 1, r.m[1][2] = 2 * (q2 * q3 - q0 * q1);
    r.m[2][0] = 2 * (q1 * q3 - q0 * q2), r.m[2][1] = 2 * (q2 * q3 + q0 * q1), r.m[2][2] = 2 * (q0 * q0 + q3 * q3) - 1;
    return r;
}

__host__ __device__ __forceinline__ void store3(double *__restrict__ p, V3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

// One reactive atom of one conformer: its lobes go straight to their rows pc (centres) and pv (orbital vectors), f64[4][3] each, unused lobes
// zero; returns the number of lobes and sets *kind.  x = the conformer's atoms; every index was checked on the host and is clamped here all the same.
__host__ __device__ __forceinline__ int orb_lobes(const OrbArgs &a, const OrbRecipe &rc, const double *__restrict__ x, bool sigmatropic,
                                                  double *pc, double *pv, int *kind) {
    const int last = a.n_atoms - 1;
    auto at = [&](int idx) -> V3 {
        const double *p = x + 3 * size_t(idx < 0 ? 0 : (idx > last ? last : idx));
        return {p[0], p[1], p[2]};
    };
    auto rot = [&](V3 pointer, int which) { return rot_about(pointer, a.half_sin[which], a.half_cos[which]); };
    auto put = [&](int k, V3 center, V3 vec) {
        store3(pc + 3 * k, center);
        store3(pv + 3 * k, vec);
    };
    const V3 coord = at(rc.atom);
    const bool sigmastar = rc.flags & TSC_ORB_F_SIGMASTAR;
    double orb_dim = rc.orb_dim;
    int n = 0;
    switch (rc.cls) {
        case TSC_ORB_SINGLE:   // reactive_atoms_classes.py:29-80
        case TSC_ORB_SP3: {    // :122-207
            const bool single = rc.cls == TSC_ORB_SINGLE;
            *kind = single ? TSC_ORB_KIND_SINGLE : TSC_ORB_KIND_SP3;
            if (!sigmastar) {
                n = 1;
                if (single) {
                    const V3 d = coord - at(rc.nb[0]);
                    if (rc.flags & TSC_ORB_F_BOND_LENGTH) orb_dim = norm_of(d);   // :77
                    const V3 v = unit(d);
                    put(0, v * orb_dim + coord, v);
                } else {
                    const V3 v = coord - at(rc.ex[0]);   // (not normalised, :172)
                    put(0, unit(v) * orb_dim + coord, v);
                }
            } else {
                const V3 partner = at(rc.ex[0]);
                const V3 pivot = unit(partner - coord);
                V3 v = unit(at(rc.ex[1]) - (single ? partner : coord));   // :62 / :189
                v = reject(v, pivot);
                if (single && (rc.flags & TSC_ORB_F_BOND_LENGTH)) orb_dim = norm_of(coord - at(rc.nb[0]));
                n = 3;
                for (int k = 0; k < 3; ++k) {   // angle + 60 for angle in 0, 120, 240
                    const V3 w = apply(rot(pivot, k == 0 ? OB_A60 : (k == 1 ? OB_A180 : OB_A300)), v);
                    put(k, (single ? w : unit(w)) * orb_dim + coord, w);   // :80 / :207
                }
            }
        } break;
        case TSC_ORB_SP2: {   // :83-119
            const V3 n0 = unit(at(rc.nb[0]) - coord), n1 = unit(at(rc.nb[1]) - coord), n2 = unit(at(rc.nb[2]) - coord);
            const V3 v = unit((cross(n0, n1) + cross(n1, n2) + cross(n2, n0)) / 3.0);
            *kind = TSC_ORB_KIND_SP2, n = 2;
            put(0, v * orb_dim + coord, v);
            put(1, (-v) * orb_dim + coord, -v);
        } break;
        case TSC_ORB_ETHER: {   // :248-284
            const V3 v0 = unit(at(rc.nb[0]) - coord) * orb_dim, v1 = unit(at(rc.nb[1]) - coord) * orb_dim;
            const M3 m = matmul(rot((v0 + v1) / 2.0, OB_A90), rot(cross(v0, v1), OB_A180));
            *kind = TSC_ORB_KIND_ETHER, n = 2;
            const V3 w0 = apply(m, v0), w1 = apply(m, v1);
            put(0, w0 + coord, w0);
            put(1, w1 + coord, w1);
        } break;
        case TSC_ORB_KETONE: {   // :288-375: the centres first, orb_vecs = norm(centre) (:371), then centres += coord
            const V3 vector = unit(at(rc.nb[0]) - coord) * orb_dim;
            const int subtype = rc.flags & TSC_ORB_F_KETONE_MASK;
            if (subtype == TSC_ORB_F_KETONE_KETENE) {
                const V3 v = at(rc.ex[1]) - at(rc.ex[0]);
                const V3 pointer = unit(v - vector * dot(v, unit(vector))) * orb_dim;   // :335-336
                *kind = TSC_ORB_KIND_KETONE_PP, n = 4;
                for (int k = 0; k < 4; ++k) {
                    const V3 w = apply(rot(vector, k == 0 ? OB_A0 : (k == 1 ? OB_A90 : (k == 2 ? OB_A180 : OB_A270))), pointer);
                    put(k, w + coord, unit(w));
                }
            } else if (subtype == TSC_ORB_F_KETONE_TWO) {
                const V3 pivot = unit(cross(at(rc.ex[0]) - coord, at(rc.ex[1]) - coord));
                n = 2;
                V3 w0, w1;
                if (sigmatropic) {   // :350-353
                    *kind = TSC_ORB_KIND_KETONE_P;
                    w0 = pivot * orb_dim, w1 = -pivot * orb_dim;
                } else {
                    *kind = TSC_ORB_KIND_KETONE_SP2;
                    w0 = apply(rot(pivot, OB_A120), vector), w1 = apply(rot(pivot, OB_A240), vector);
                }
                put(0, w0 + coord, unit(w0));
                put(1, w1 + coord, unit(w1));
            } else {
                const V3 v1 = unit(at(rc.ex[0]) - coord) * orb_dim;
                const M3 m = rot(unit(cross(vector, v1)), OB_A180);
                *kind = TSC_ORB_KIND_KETONE_TRILOBE, n = 3;
                for (int k = 0; k < 3; ++k) {
                    const V3 w = apply(m, k == 0 ? v1 : unit(at(rc.ex[k]) - coord) * orb_dim);
                    put(k, w + coord, unit(w));
                }
            }
        } break;
        case TSC_ORB_IMINE: {   // :378-416
            const V3 v0 = at(rc.nb[0]) - coord, v1 = at(rc.nb[1]) - coord;
            *kind = TSC_ORB_KIND_IMINE;
            if (sigmatropic) {
                const V3 p = unit(cross(v0, v1)) * orb_dim;
                n = 2;
                put(0, p + coord, p);
                put(1, (-p) + coord, -p);
            } else {
                const V3 w = -unit((unit(v0) + unit(v1)) / 2.0) * orb_dim;
                n = 1;
                put(0, w + coord, w);
            }
        } break;
        case TSC_ORB_SP_OR_CARBENE: {   // :420-538
            const V3 o0 = at(rc.nb[0]), o1 = at(rc.nb[1]);
            const V3 v0 = o0 - coord, v1 = o1 - coord;
            const V3 n0 = unit(v0), n1 = unit(v1);
            const double c = dot(unit(n0), unit(n1));   // vec_angle normalises what it is given once more (algebra.py:58-62)
            const double angle = acos(c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c)) * 180 / M_PI;
            if (fabs(angle - 180) < 5) {   // :442
                V3 pivot1;
                if (rc.flags & (TSC_ORB_F_ALLENE | TSC_ORB_F_KETENE)) {
                    const V3 axis = unit(o0 - o1);
                    const V3 ref = at(rc.ex[0]) - at(rc.ex[1]);
                    pivot1 = reject(ref, axis);   // :512
                } else {
                    const V3 v = {rc.seed[0], rc.seed[1], rc.seed[2]};
                    pivot1 = v - v0 * dot(v, n0);   // :496
                }
                const M3 r2 = rot(unit(cross(pivot1, v0)), OB_A90);
                *kind = TSC_ORB_KIND_SP, n = 4;
                for (int k = 0; k < 4; ++k) {
                    const M3 r1 = rot(pivot1, k == 0 ? OB_A0 : (k == 1 ? OB_A90 : (k == 2 ? OB_A180 : OB_A270)));
                    const V3 w = apply(matmul(r2, r1), n0) * orb_dim;   // :518-520
                    put(k, w + coord, w);
                }
            } else {
                orb_dim = rc.orb_dim_bent;
                const V3 p = unit(cross(n0, n1));
                const V3 w = -unit((n0 + n1) / 2.0) * orb_dim;   // :529-534
                *kind = TSC_ORB_KIND_BENT_CARBENE, n = 3;
                put(0, w + coord, w);
                put(1, p * orb_dim + coord, p * orb_dim);
                put(2, (-p) * orb_dim + coord, (-p) * orb_dim);
            }
        } break;
        default: {   // TSC_ORB_METAL, :541-576
            const V3 v1 = at(rc.nb[0]) - coord, v2 = at(rc.ex[0]) - coord;
            const V3 v = unit(apply(rot(cross(v1, v2), OB_A120), v1));
            *kind = TSC_ORB_KIND_METAL, n = 4;
            for (int k = 0; k < 4; ++k) {
                const V3 w = apply(rot(v1, k == 0 ? OB_A0 : (k == 1 ? OB_A90 : (k == 2 ? OB_A180 : OB_A270))), v);
                put(k, w * orb_dim + coord, w);
            }
        } break;
    }
    for (int k = n; k < OB_LOBES; ++k) put(k, V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 0.0});
    return n;
}

// One conformer: every output row c.  (Host-callable as well: tools/probe/orbitals_host_check.cpp runs this code on the CPU under sanitizers.)
__host__ __device__ inline void orb_conformer(const OrbArgs &a, int64_t c, const double *__restrict__ coords, double *__restrict__ centers,
                                              double *__restrict__ orb_vecs, uint8_t *__restrict__ n_lobes, uint8_t *__restrict__ kind,
                                              uint8_t *__restrict__ sigmatropic, double *__restrict__ pivot, double *__restrict__ meanpoint,
                                              int8_t *__restrict__ lobe_index, uint8_t *__restrict__ n_pivots) {
    const int R = a.n_reactive;
    const double *x = coords + size_t(c) * a.n_atoms * 3;
    bool sig = a.sigma_mode == 2;
    if (a.sigma_mode == 1) {   // tscode/graph_manipulations.py:256
        const double *p = x + 3 * size_t(a.rec[0].atom), *q = x + 3 * size_t(a.rec[1].atom);
        const V3 d = V3{p[0], p[1], p[2]} - V3{q[0], q[1], q[2]};
        sig = norm_of(d) < 3;
    }
    sigmatropic[c] = sig;
    int n1 = 0, n2 = 0;
    for (int r = 0; r < R; ++r) {
        int k = 0;
        const int n = orb_lobes(a, a.rec[r], x, sig, centers + (size_t(c) * R + r) * OB_LOBES * 3, orb_vecs + (size_t(c) * R + r) * OB_LOBES * 3, &k);
        n_lobes[size_t(c) * R + r] = uint8_t(n);
        kind[size_t(c) * R + r] = uint8_t(k);
        if (r == 0) n1 = n2 = n;
        if (r == 1) n2 = n;
    }
    if (!a.want_pivots) return;
    // the lobes of the first two reactive atoms, read back from this lane's own rows (of the same atom twice when there is one)
    V3 c1[OB_LOBES], c2[OB_LOBES];
    {
        const double *p1 = centers + size_t(c) * R * OB_LOBES * 3, *p2 = p1 + (R >= 2 ? OB_LOBES * 3 : 0);
#pragma unroll
        for (int k = 0; k < OB_LOBES; ++k) c1[k] = V3{p1[3 * k], p1[3 * k + 1], p1[3 * k + 2]}, c2[k] = V3{p2[3 * k], p2[3 * k + 1], p2[3 * k + 2]};
    }
    // ---- tscode/embedder.py:575-621: slot t = i + 4 j is the pivot from lobe i of the first atom to lobe j of the second (of the same atom
    // when there is one, i < j), walked with i fastest: the order of cartesian_product
    unsigned valid = 0;
    double len[OB_PIVOTS];
#pragma unroll
    for (int t = 0; t < OB_PIVOTS; ++t) {
        const int i = t & 3, j = t >> 2;
        const bool ok = R == 2 ? (i < n1 && j < n2) : (R == 1 && i < j && j < n1);   // (:589, :604: one or two reactive atoms)
        const V3 d = c2[j] - c1[i];
        len[t] = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
        valid |= unsigned(ok) << t;
    }
    unsigned keep = valid;
    if (a.suprafacial && __builtin_popcount(valid) == 4) {   // :552-563
        double four[4] = {0.0, 0.0, 0.0, 0.0};
        int k = 0;
#pragma unroll
        for (int t = 0; t < OB_PIVOTS; ++t) {
            if (valid >> t & 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) four[q] = k == q ? len[t] : four[q];
                ++k;
            }
        }
        bool found = false;
        double bound = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int not_above = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) not_above += four[s] >= four[q];
            if (!found && not_above == 2) found = true, bound = four[s];
        }
        if (found) {
#pragma unroll
            for (int t = 0; t < OB_PIVOTS; ++t)
                if (!(len[t] <= bound)) keep &= ~(1u << t);
        }
    }
    if (a.sigmastar && keep) {   // :569-573
        double shortest = INFINITY;
#pragma unroll
        for (int t = 0; t < OB_PIVOTS; ++t)
            if (keep >> t & 1) shortest = fmin(shortest, len[t]);
#pragma unroll
        for (int t = 0; t < OB_PIVOTS; ++t)
            if (!(len[t] - shortest < 1e-5)) keep &= ~(1u << t);
    }
    double *pp = pivot + size_t(c) * OB_PIVOTS * 3, *pm = meanpoint + size_t(c) * OB_PIVOTS * 3;
    int8_t *pl = lobe_index + size_t(c) * OB_PIVOTS * 2;
    int count = 0;
    const double *p1 = centers + size_t(c) * R * OB_LOBES * 3, *p2 = p1 + (R >= 2 ? OB_LOBES * 3 : 0);
#pragma unroll 1
    for (int t = 0; t < OB_PIVOTS; ++t) {   // (one slot at a time, the two centres from this lane's own rows: the 16 slots unrolled cost 190 registers)
        if (keep >> t & 1) {
            const int i = t & 3, j = t >> 2;
            const V3 from = {p1[3 * i], p1[3 * i + 1], p1[3 * i + 2]}, to = {p2[3 * j], p2[3 * j + 1], p2[3 * j + 2]};
            store3(pp + 3 * count, to - from);                 // hypermolecule_class.py:400
            store3(pm + 3 * count, (from + to) / 2.0);         // :401
            pl[2 * count] = int8_t(i), pl[2 * count + 1] = int8_t(j);
            ++count;
        }
    }
    for (int t = count; t < OB_PIVOTS; ++t) {
        store3(pp + 3 * t, V3{0.0, 0.0, 0.0});
        store3(pm + 3 * t, V3{0.0, 0.0, 0.0});
        pl[2 * t] = pl[2 * t + 1] = -1;
    }
    n_pivots[c] = uint8_t(count);
}

__global__ void __launch_bounds__(256) k_orbitals(const OrbArgs a, const double *__restrict__ coords, double *__restrict__ centers,
                                                  double *__restrict__ orb_vecs, uint8_t *__restrict__ n_lobes, uint8_t *__restrict__ kind,
                                                  uint8_t *__restrict__ sigmatropic, double *__restrict__ pivot, double *__restrict__ meanpoint,
                                                  int8_t *__restrict__ lobe_index, uint8_t *__restrict__ n_pivots) {
    for (int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; c < a.n_conf; c += int64_t(gridDim.x) * blockDim.x)
        orb_conformer(a, c, coords, centers, orb_vecs, n_lobes, kind, sigmatropic, pivot, meanpoint, lobe_index, n_pivots);
}

}  // namespace tsc
