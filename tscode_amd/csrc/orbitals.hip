// orbitals.hip -- launch and C ABI of the reactive-atom orbitals and pivots of a conformer ensemble (orbitals.hpp;
// tscode/hypermolecule_class.py:195-217, tscode/reactive_atoms_classes.py, tscode/embedder.py:542-621).  gfx950 only.  No entry point
// has a CPU path; the per-conformer code of orbitals.hpp is host-callable only so that tools/probe/orbitals_host_check.cpp can run it under sanitizers.
#include "host.hpp"
#include "call.hpp"
#include "orbitals.hpp"

namespace {

using namespace tsc;

static_assert(sizeof(tsc_orbital_recipe) == 88, "tsc_orbital_recipe is 12 int32 and 5 doubles, no padding");

// HIP-event time of the kernel of the calling thread's latest tsc_orbitals / tsc_orbitals_dev, taken only under the context option
// "pass_timing" >= 1 (tools/orbitals_profile.py); -1 otherwise
thread_local float g_kernel_ms = -1.f;

struct Outputs {
    double *centers, *orb_vecs;
    uint8_t *n_lobes, *kind, *sigmatropic;
    double *pivot, *meanpoint;
    int8_t *lobe_index;
    uint8_t *n_pivots;
};

// Everything that can be refused is refused here, before anything touches the device: the kernel gathers atoms by the indices of the recipes.
int make_args(const char *who, int64_t n_conf, int n_atoms, const tsc_orbital_recipe *recipes, int n_reactive, int sigmatropic_mode,
              int suprafacial, const Outputs &o, OrbArgs *out) {
    TSC_REQUIRE(recipes && o.centers && o.orb_vecs && o.n_lobes && o.kind && o.sigmatropic, "%s: null argument", who);
    const int n_piv = (o.pivot != nullptr) + (o.meanpoint != nullptr) + (o.lobe_index != nullptr) + (o.n_pivots != nullptr);
    TSC_REQUIRE(n_piv == 0 || n_piv == 4, "%s: pivot, meanpoint, lobe_index and n_pivots are given together or not at all", who);
    TSC_REQUIRE(n_conf >= 0, "%s: %lld conformers", who, (long long)n_conf);
    TSC_REQUIRE(n_atoms >= 1 && n_atoms <= TSC_ORB_MAX_ATOMS, "%s: %d atoms per conformer (1 .. %d)", who, n_atoms, TSC_ORB_MAX_ATOMS);
    TSC_REQUIRE(n_reactive >= 1 && n_reactive <= OB_MAX_REACTIVE, "%s: %d reactive atoms (1 .. %d)", who, n_reactive, OB_MAX_REACTIVE);
    TSC_REQUIRE(sigmatropic_mode >= 0 && sigmatropic_mode <= 2, "%s: sigmatropic mode %d (0 never, 1 by distance, 2 always)", who, sigmatropic_mode);
    TSC_REQUIRE(n_piv == 0 || n_reactive <= 2, "%s: pivots are defined for one or two reactive atoms, not %d: pass no pivot arrays", who, n_reactive);
    TSC_REQUIRE(sigmatropic_mode != 1 || n_reactive == 2, "%s: sigmatropic by distance takes two reactive atoms, not %d", who, n_reactive);
    OrbArgs &a = *out;
    memset(&a, 0, sizeof(a));
    a.n_conf = n_conf, a.n_atoms = n_atoms, a.n_reactive = n_reactive, a.sigma_mode = sigmatropic_mode, a.suprafacial = suprafacial != 0;
    a.want_pivots = n_piv == 4;
    const double degrees[OB_ANGLES] = {0, 60, 90, 120, 180, 240, 270, 300};
    for (int q = 0; q < OB_ANGLES; ++q) {   // tscode/algebra.py:337-341: angle *= pi / 180, then sin and cos of angle / 2
        const double angle = degrees[q] * (M_PI / 180);
        a.half_sin[q] = std::sin(angle / 2), a.half_cos[q] = std::cos(angle / 2);
    }
    for (int r = 0; r < n_reactive; ++r) {
        const tsc_orbital_recipe &rc = recipes[r];
        const bool sigmastar = rc.flags & TSC_ORB_F_SIGMASTAR;
        int n_nb = 0, n_ex = 0;
        switch (rc.cls) {
            case TSC_ORB_SINGLE: n_nb = 1, n_ex = sigmastar ? 2 : 0; break;
            case TSC_ORB_SP3: n_ex = sigmastar ? 2 : 1; break;
            case TSC_ORB_SP2: n_nb = 3; break;
            case TSC_ORB_ETHER:
            case TSC_ORB_IMINE: n_nb = 2; break;
            case TSC_ORB_KETONE: {
                const int subtype = rc.flags & TSC_ORB_F_KETONE_MASK;
                TSC_REQUIRE(subtype != 0, "%s: recipe %d is a Ketone without a subtype flag", who, r);
                n_nb = 1, n_ex = subtype == TSC_ORB_F_KETONE_TRILOBE ? 3 : 2;
            } break;
            case TSC_ORB_SP_OR_CARBENE: n_nb = 2, n_ex = (rc.flags & (TSC_ORB_F_ALLENE | TSC_ORB_F_KETENE)) ? 2 : 0; break;
            case TSC_ORB_METAL: n_nb = 1, n_ex = 1; break;
            default: TSC_REQUIRE(false, "%s: recipe %d has class %d (0 .. 7)", who, r, rc.cls);
        }
        TSC_REQUIRE((rc.flags & ~TSC_ORB_F_ALL) == 0, "%s: recipe %d has unknown flag bits %#x", who, r, rc.flags);
        TSC_REQUIRE(rc.atom >= 0 && rc.atom < n_atoms, "%s: recipe %d: atom %d with %d atoms", who, r, rc.atom, n_atoms);
        for (int q = 0; q < n_nb; ++q)
            TSC_REQUIRE(rc.nb[q] >= 0 && rc.nb[q] < n_atoms, "%s: recipe %d: neighbour slot %d = %d with %d atoms", who, r, q, rc.nb[q], n_atoms);
        for (int q = 0; q < n_ex; ++q)
            TSC_REQUIRE(rc.ex[q] >= 0 && rc.ex[q] < n_atoms, "%s: recipe %d: extra slot %d = %d with %d atoms", who, r, q, rc.ex[q], n_atoms);
        TSC_REQUIRE(std::isfinite(rc.orb_dim) && std::isfinite(rc.orb_dim_bent), "%s: recipe %d: orb_dim is not finite", who, r);
        TSC_REQUIRE(std::isfinite(rc.seed[0]) && std::isfinite(rc.seed[1]) && std::isfinite(rc.seed[2]), "%s: recipe %d: seed is not finite", who, r);
        TSC_REQUIRE(sigmastar == bool(recipes[0].flags & TSC_ORB_F_SIGMASTAR), "%s: the recipes disagree on sp3_sigmastar", who);
        a.rec[r] = rc;
    }
    a.sigmastar = (recipes[0].flags & TSC_ORB_F_SIGMASTAR) != 0;
    return 0;
}

// device pointers throughout
int run_dev(tsc_ctx *c, const OrbArgs &a, const double *coords, const Outputs &o) {
    StageTimer tm(c);
    tm.begin();
    // (a grid-stride loop from a million conformers on)
    hipLaunchKernelGGL(k_orbitals, dim3(grid_for(a.n_conf, 256)), dim3(256), 0, c->stream, a, coords, o.centers, o.orb_vecs, o.n_lobes, o.kind,
                       o.sigmatropic, o.pivot, o.meanpoint, o.lobe_index, o.n_pivots);
    const hipError_t launched = hipGetLastError();
    if (launched == hipSuccess) tm.end(&g_kernel_ms);
    TSC_HIP(launched);
    return 0;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int tsc_orbitals_timings(tsc_ctx *c, float *ms) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && ms, "tsc_orbitals_timings: null argument");
    *ms = g_kernel_ms;
    return 0;
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_orbitals_dev(tsc_ctx *c, const double *coords, int64_t n_conf, int n_atoms,
                                                                       const tsc_orbital_recipe *recipes, int n_reactive, int sigmatropic_mode,
                                                                       int suprafacial, double *centers, double *orb_vecs, uint8_t *n_lobes,
                                                                       uint8_t *kind, uint8_t *sigmatropic, double *pivot, double *meanpoint,
                                                                       int8_t *lobe_index, uint8_t *n_pivots) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords, "tsc_orbitals_dev: null argument");
    const Outputs o{centers, orb_vecs, n_lobes, kind, sigmatropic, pivot, meanpoint, lobe_index, n_pivots};
    OrbArgs a;
    TSC_TRY(make_args("tsc_orbitals_dev", n_conf, n_atoms, recipes, n_reactive, sigmatropic_mode, suprafacial, o, &a));
    g_kernel_ms = -1.f;
    if (n_conf == 0) return 0;
    DeviceGuard guard(c->device);
    return run_dev(c, a, coords, o);
    TSC_API_GUARD_END
}

extern "C" __attribute__((visibility("default"))) int tsc_orbitals(tsc_ctx *c, const double *coords, int64_t n_conf, int n_atoms,
                                                                   const tsc_orbital_recipe *recipes, int n_reactive, int sigmatropic_mode,
                                                                   int suprafacial, double *centers, double *orb_vecs, uint8_t *n_lobes, uint8_t *kind,
                                                                   uint8_t *sigmatropic, double *pivot, double *meanpoint, int8_t *lobe_index,
                                                                   uint8_t *n_pivots) {
    TSC_API_GUARD_BEGIN
    TSC_REQUIRE(c && coords, "tsc_orbitals: null argument");
    const Outputs h{centers, orb_vecs, n_lobes, kind, sigmatropic, pivot, meanpoint, lobe_index, n_pivots};
    OrbArgs a;
    TSC_TRY(make_args("tsc_orbitals", n_conf, n_atoms, recipes, n_reactive, sigmatropic_mode, suprafacial, h, &a));
    g_kernel_ms = -1.f;
    if (n_conf == 0) return 0;
    HostCall hc(c);
    const size_t C = size_t(n_conf), R = size_t(n_reactive), L = OB_LOBES, P = OB_PIVOTS;
    double *d_coords;
    Outputs o{};
    TSC_TRY(hc.in(coords, C * n_atoms * 3, &d_coords));
    TSC_TRY(hc.out(centers, C * R * L * 3, &o.centers));
    TSC_TRY(hc.out(orb_vecs, C * R * L * 3, &o.orb_vecs));
    TSC_TRY(hc.out(n_lobes, C * R, &o.n_lobes));
    TSC_TRY(hc.out(kind, C * R, &o.kind));
    TSC_TRY(hc.out(sigmatropic, C, &o.sigmatropic));
    TSC_TRY(hc.out(pivot, C * P * 3, &o.pivot));   // (the four pivot arrays together or none of them: make_args)
    TSC_TRY(hc.out(meanpoint, C * P * 3, &o.meanpoint));
    TSC_TRY(hc.out(lobe_index, C * P * 2, &o.lobe_index));
    TSC_TRY(hc.out(n_pivots, C, &o.n_pivots));
    TSC_TRY(run_dev(c, a, d_coords, o));
    return hc.finish();
    TSC_API_GUARD_END
}
