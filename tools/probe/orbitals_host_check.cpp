// orbitals_host_check.cpp -- the per-conformer code of csrc/orbitals.hpp (orb_conformer, behind the argument checks of orbitals.hip's make_args)
// run on the CPU by a stand-alone program, so that it can be built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the
// library; tools/orbitals_host_check.py builds it, feeds it the fixtures' cases and compares what it writes.
//
//   orbitals_host_check IN OUT
//   IN : int64 n_conf, int32 n_atoms, int32 n_reactive, int32 sigmatropic_mode, int32 suprafacial, tsc_orbital_recipe[n_reactive],
//        f64 coords[n_conf][n_atoms][3]
//   OUT: centers, orb_vecs, n_lobes, kind, sigmatropic, then (one or two reactive atoms) pivot, meanpoint, lobe_index, n_pivots, laid out as
//        include/tscode_hip.h says, each in a heap block of exactly its documented size: a write past any end is seen by the sanitizer.
#include <cstdio>
#include <vector>

#include "../../tscode_amd/csrc/orbitals.hip"

template <typename T>
static bool put(FILE *f, const std::vector<T> &v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    int64_t C;
    int32_t h[4];
    if (!f || fread(&C, 8, 1, f) != 1 || fread(h, 4, 4, f) != 4 || C < 0 || h[0] < 1 || h[1] < 1 || h[1] > TSC_ORB_MAX_REACTIVE) return 2;
    const int n = h[0], R = h[1];
    std::vector<tsc_orbital_recipe> rec(R);
    std::vector<double> x(size_t(C) * n * 3);
    if (fread(rec.data(), sizeof(tsc_orbital_recipe), R, f) != size_t(R) || fread(x.data(), 8, x.size(), f) != x.size()) return 2;
    fclose(f);
    const bool piv = R <= 2;
    std::vector<double> centers(size_t(C) * R * 12), orb_vecs(size_t(C) * R * 12), pivot(piv ? size_t(C) * 48 : 0), meanpoint(piv ? size_t(C) * 48 : 0);
    std::vector<uint8_t> n_lobes(size_t(C) * R), kind(size_t(C) * R), sig(C), n_pivots(piv ? C : 0);
    std::vector<int8_t> lobe_index(piv ? size_t(C) * 32 : 0);
    const Outputs o{centers.data(), orb_vecs.data(), n_lobes.data(), kind.data(), sig.data(), piv ? pivot.data() : nullptr,
                    piv ? meanpoint.data() : nullptr, piv ? lobe_index.data() : nullptr, piv ? n_pivots.data() : nullptr};
    OrbArgs a;
    if (make_args("orbitals_host_check", C, n, rec.data(), R, h[2], h[3], o, &a) != 0) return fprintf(stderr, "%s\n", tsc::g_err), 3;
    for (int64_t c = 0; c < C; ++c)
        orb_conformer(a, c, x.data(), o.centers, o.orb_vecs, o.n_lobes, o.kind, o.sigmatropic, o.pivot, o.meanpoint, o.lobe_index, o.n_pivots);
    f = fopen(argv[2], "wb");
    const bool ok = f && put(f, centers) && put(f, orb_vecs) && put(f, n_lobes) && put(f, kind) && put(f, sig) && put(f, pivot) && put(f, meanpoint) &&
                    put(f, lobe_index) && put(f, n_pivots);
    return (f && fclose(f) == 0 && ok) ? 0 : 4;
}
