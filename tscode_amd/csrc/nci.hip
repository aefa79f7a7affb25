// nci.hip -- launches and C ABI of the batched non-covalent-interaction finder (nci.hpp; tscode/nci.py:28-181 with is_phenyl,
// tscode/graph_manipulations.py:152-174).  gfx950 only.  There is deliberately no CPU implementation behind these entry points.
#include "host.hpp"
#include "call.hpp"
#include "nci.hpp"

namespace {

using namespace tsc;

// HIP-event time of the kernel of the calling thread's latest tsc_nci / tsc_nci_dev, taken only under the context option
// "pass_timing" >= 1 (tools/nci_profile.py); -1 otherwise
thread_local float g_kernel_ms = -1.f;

struct Outputs {
    int32_t *counts;
    uint8_t *overflow;
    uint64_t *pair_bits;
    uint16_t *ring_atoms;
    uint8_t *ring_owner;
    double *ring_center;
    uint64_t *ring_atom_bits, *ring_ring_bits;
};

// Largest double whose square root is not above t: (sqrt(d2) > t) == (d2 > x) for every d2, IEEE sqrt being correctly rounded and monotone
double sq_bound_not_above(double t) {
    double x = t * t;
    while (std::sqrt(x) > t) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= t) x = std::nextafter(x, INFINITY);
    return x;
}

// Everything that can be refused is refused here, before anything touches the device.
int make_args(const char *who, int64_t n_structs, int n_atoms, const uint8_t *atom_class, const double *thr, int n_classes,
              const uint8_t *atom_mol, int n_mols, const uint8_t *ring_candidate, const double *ring_thr, double ring_ring_thr,
              const int32_t *constrained, int n_con, int con_per_struct, bool constrained_on_host, int owner_rule, NciArgs *out) {
    TSC_REQUIRE(atom_class && thr && atom_mol && ring_candidate && ring_thr, "%s: null argument", who);
    TSC_REQUIRE(n_structs >= 0, "%s: %lld structures", who, (long long)n_structs);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= NC_MAX_ATOMS, "%s: %d atoms per structure (1 .. %d)", who, n_atoms, NC_MAX_ATOMS);
    TSC_REQUIRE(n_classes >= 1 && n_classes <= NC_MAX_CLASSES, "%s: %d element classes (1 .. %d)", who, n_classes, NC_MAX_CLASSES);
    TSC_REQUIRE(n_mols >= 1 && n_mols <= NC_MAX_MOLS, "%s: %d molecules (1 .. %d)", who, n_mols, NC_MAX_MOLS);
    TSC_REQUIRE(n_con >= 0 && n_con <= NC_MAX_CON, "%s: %d constrained atoms per structure (0 .. %d)", who, n_con, NC_MAX_CON);
    TSC_REQUIRE(n_con == 0 || constrained, "%s: %d constrained atoms without an array", who, n_con);
    TSC_REQUIRE(owner_rule == 0 || owner_rule == 1, "%s: owner rule %d (0: as the reference, 1: intermolecular)", who, owner_rule);
    TSC_REQUIRE(std::isfinite(ring_ring_thr) && ring_ring_thr >= 0.0, "%s: ring-ring threshold %g is negative or not finite", who, ring_ring_thr);
    const int T = n_classes + 1;
    NciArgs &a = *out;
    memset(&a, 0, sizeof(a));
    a.n_structs = n_structs, a.n = n_atoms, a.n_tab = T, a.n_mols = n_mols, a.owner_rule = owner_rule;
    a.rr_bound = clash_sq_bound(ring_ring_thr);
    a.near_bound = sq_bound_not_above(NC_RING_DIST);
    a.flat_bound = 1.0 - std::cos(NC_FLAT_DEGREES * M_PI / 180.0);
    // the atoms of a molecule are contiguous and the molecules come in order, every one with an atom: what np.cumsum(ids) describes
    TSC_REQUIRE(atom_mol[0] == 0 && atom_mol[n_atoms - 1] == n_mols - 1, "%s: the atoms run from molecule %d to %d with %d molecules", who,
                int(atom_mol[0]), int(atom_mol[n_atoms - 1]), n_mols);
    TSC_TRY(check_class_table(who, atom_class, n_atoms, thr, n_classes, a.bound, T));  // (a bound of 0: never)
    int n_cand = 0;
    for (int i = 0; i < n_atoms; ++i) {
        const int m = atom_mol[i];
        TSC_REQUIRE(i == 0 || m == atom_mol[i - 1] || m == atom_mol[i - 1] + 1, "%s: atom %d of molecule %d follows one of molecule %d", who, i, m,
                    int(atom_mol[i - 1]));
        a.meta[i] = uint8_t(atom_class[i] | m << 4);
        a.mol_end[m] = i + 1;
        if (i == 0 || m != atom_mol[i - 1]) a.cand_off[m] = n_cand;
        if (ring_candidate[i]) {
            TSC_REQUIRE(n_cand - a.cand_off[m] < NC_MAX_CAND, "%s: molecule %d has more than %d ring candidates", who, m, NC_MAX_CAND);
            a.cand[n_cand++] = uint16_t(i);
        }
    }
    a.cand_off[n_mols] = n_cand;
    for (int p = 0; p < n_classes; ++p) {
        TSC_REQUIRE(std::isfinite(ring_thr[p]) && ring_thr[p] >= 0.0, "%s: ring_thr[%d] = %g is negative or not finite", who, p, ring_thr[p]);
        a.ring_bound[p] = clash_sq_bound(ring_thr[p]);
    }
    return check_index_list(who, "constrained", constrained, n_con, con_per_struct, constrained_on_host, n_structs, n_atoms, a.con_words, &a.n_con);
}

// device pointers throughout, except the tables
int run_dev(tsc_ctx *c, const NciArgs &a, const double *coords, const int32_t *con_dev, const Outputs &o) {
    static_assert(nci_lds_bytes(NC_MAX_ATOMS) <= 65536, "LDS of a block");
    StageTimer tm(c);
    tm.begin();
    with_words(a.n, [&](auto w) {
        // (a grid-stride loop from 8192 structures on: eight blocks per CU is what the LDS of a small structure admits)
        hipLaunchKernelGGL(k_nci<decltype(w)::value>, dim3(grid_for(a.n_structs, 4, 2048)), dim3(256), nci_lds_bytes(a.n), c->stream, a, coords, con_dev,
                           o.counts, o.overflow, o.pair_bits, o.ring_atoms, o.ring_owner, o.ring_center, o.ring_atom_bits, o.ring_ring_bits);
    });
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_kernel_ms);
    TSC_HIP(launched);
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_nci_timings(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "tsc_nci_timings: null argument");
    *ms = g_kernel_ms;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_nci_dev(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                                  const uint8_t *atom_class, const double *thr, int n_classes,
                                                                  const uint8_t *atom_mol, int n_mols, const uint8_t *ring_candidate,
                                                                  const double *ring_thr, double ring_ring_thr, const int32_t *constrained,
                                                                  int n_con, int con_per_struct, int owner_rule, int32_t *counts,
                                                                  uint8_t *overflow, uint64_t *pair_bits, uint16_t *ring_atoms,
                                                                  uint8_t *ring_owner, double *ring_center, uint64_t *ring_atom_bits,
                                                                  uint64_t *ring_ring_bits) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && counts && overflow, "tsc_nci_dev: null argument");
    NciArgs a;
    TSC_TRY(make_args("tsc_nci_dev", n_structs, n_atoms, atom_class, thr, n_classes, atom_mol, n_mols, ring_candidate, ring_thr, ring_ring_thr,
                      constrained, n_con, con_per_struct, false, owner_rule, &a));
    g_kernel_ms = -1.f;
    if (n_structs == 0) return 0;
    DeviceGuard guard(c->device);
    const Outputs o{counts, overflow, pair_bits, ring_atoms, ring_owner, ring_center, ring_atom_bits, ring_ring_bits};
    return run_dev(c, a, coords, a.n_con ? constrained : nullptr, o);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_nci(tsc_ctx *c, const double *coords, int64_t n_structs, int n_atoms,
                                                              const uint8_t *atom_class, const double *thr, int n_classes,
                                                              const uint8_t *atom_mol, int n_mols, const uint8_t *ring_candidate,
                                                              const double *ring_thr, double ring_ring_thr, const int32_t *constrained, int n_con,
                                                              int con_per_struct, int owner_rule, int32_t *counts, uint8_t *overflow,
                                                              uint64_t *pair_bits, uint16_t *ring_atoms, uint8_t *ring_owner, double *ring_center,
                                                              uint64_t *ring_atom_bits, uint64_t *ring_ring_bits) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords && counts && overflow, "tsc_nci: null argument");
    NciArgs a;
    TSC_TRY(make_args("tsc_nci", n_structs, n_atoms, atom_class, thr, n_classes, atom_mol, n_mols, ring_candidate, ring_thr, ring_ring_thr,
                      constrained, n_con, con_per_struct, true, owner_rule, &a));
    g_kernel_ms = -1.f;
    if (n_structs == 0) return 0;
    HostCall h(c);
    const size_t N = size_t(n_structs), W = size_t(ceil_div(n_atoms, 64)), R = NC_MAX_RINGS;
    double *d_coords;
    int32_t *d_con = nullptr;
    Outputs o{};
    TSC_TRY(h.in(coords, N * n_atoms * 3, &d_coords));
    if (a.n_con) TSC_TRY(h.in(constrained, N * n_con, &d_con));
    TSC_TRY(h.out(counts, N * 4, &o.counts));
    TSC_TRY(h.out(overflow, N, &o.overflow));
    TSC_TRY(h.out(pair_bits, N * n_atoms * W, &o.pair_bits));
    TSC_TRY(h.out(ring_atoms, N * R * 6, &o.ring_atoms));
    TSC_TRY(h.out(ring_owner, N * R, &o.ring_owner));
    TSC_TRY(h.out(ring_center, N * R * 3, &o.ring_center));
    TSC_TRY(h.out(ring_atom_bits, N * R * W, &o.ring_atom_bits));
    TSC_TRY(h.out(ring_ring_bits, N * R, &o.ring_ring_bits));
    TSC_TRY(run_dev(c, a, d_coords, d_con, o));
    return h.finish();
    TSC_API_GUARD_END
}
