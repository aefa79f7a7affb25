// call_host_check.cpp -- the host-only parts of csrc/call.hpp (check_class_table, check_index_list, with_words) run by a stand-alone
// program on hand-made cases, so that they can be built with AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library;
// tools/call_host_check.py builds and runs it.  Every array a check reads or writes lives in a heap block of exactly its documented
// size: a step past any end is seen by the sanitizer.  No HIP runtime call is made: the program needs no GPU.
//
//   call_host_check        (exit status 0 and a line "call_host_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../tscode_amd/csrc/call.hpp"

using namespace tsc;

static int g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_err); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

template <typename T>
static std::unique_ptr<T[]> block(size_t count, T fill) {
    std::unique_ptr<T[]> p(new T[count]);
    for (size_t q = 0; q < count; ++q) p[q] = fill;
    return p;
}

// x is the squared bound of threshold t: (sqrt(d2) < t) == (d2 < x) for every d2
static bool is_bound_of(double x, double t) {
    if (t == 0.0) return x == 0.0;
    return std::sqrt(x) >= t && std::sqrt(std::nextafter(x, 0.0)) < t;
}

static bool refused(int rc, const char *text) { return rc == TSC_ERR_INVALID && std::string(g_err) == text; }

static int class_tables() {
    const double SENTINEL = -7.0;
    for (int n_classes : {1, 16}) {   // (16: the most classes an entry point takes)
        const int T = n_classes + 1, n_atoms = 40;
        auto cls = block<uint8_t>(n_atoms, 0);
        for (int i = 0; i < n_atoms; ++i) cls[i] = uint8_t(i % n_classes);
        auto thr = block<double>(size_t(n_classes) * n_classes, 0.0);
        for (int p = 0; p < n_classes; ++p)
            for (int q = 0; q < n_classes; ++q) thr[p * n_classes + q] = (p + q) % 5 == 4 ? 0.0 : 0.9 + 0.173 * p + 0.0611 * q;
        auto table = block<double>(size_t(T) * T, SENTINEL);
        CHECK(check_class_table("probe", cls.get(), n_atoms, thr.get(), n_classes, table.get(), T) == 0);
        for (int p = 0; p < T; ++p)
            for (int q = 0; q < T; ++q) {
                if (p < n_classes && q < n_classes)
                    CHECK(is_bound_of(table[p * T + q], thr[p * n_classes + q]));
                else
                    CHECK(table[p * T + q] == SENTINEL);   // the row and column of the extra class are the caller's
            }
    }
    // the refusals, message for message
    auto cls = block<uint8_t>(4, 0);
    auto thr = block<double>(9, 1.5);
    auto table = block<double>(16, 0.0);
    cls[2] = 3;
    CHECK(refused(check_class_table("tsc_bond_delta", cls.get(), 4, thr.get(), 3, table.get(), 4), "tsc_bond_delta: class 3 of atom 2 with 3 classes"));
    cls[2] = 2;
    CHECK(check_class_table("tsc_bond_delta", cls.get(), 4, thr.get(), 3, table.get(), 4) == 0);
    thr[3] = -1.0;
    CHECK(refused(check_class_table("tsc_nci", cls.get(), 4, thr.get(), 3, table.get(), 4), "tsc_nci: thr[1][0] = -1 is negative or not finite"));
    thr[3] = 1.5, thr[1] = INFINITY;
    CHECK(refused(check_class_table("tsc_nci_dev", cls.get(), 4, thr.get(), 3, table.get(), 4), "tsc_nci_dev: thr[0][1] = inf is negative or not finite"));
    thr[1] = 1.5, thr[8] = NAN;
    CHECK(refused(check_class_table("tsc_bond_delta_dev", cls.get(), 4, thr.get(), 3, table.get(), 4),
                  "tsc_bond_delta_dev: thr[2][2] = nan is negative or not finite"));
    return 0;
}

static int index_lists() {
    int per = -1;
    {   // a shared list on 512 atoms: the padding, the first and the last atom
        auto idx = block<int32_t>(3, 0);
        idx[0] = -1, idx[1] = 0, idx[2] = 511;
        auto words = block<uint64_t>(8, 0);
        CHECK(check_index_list("probe", "excluded", idx.get(), 3, 0, true, 1000, 512, words.get(), &per) == 0);
        CHECK(per == 0 && words[0] == 1ull && words[7] == 1ull << 63);
        for (int w = 1; w < 7; ++w) CHECK(words[w] == 0);
        // ... the same list handed in from the device side of an entry point: a shared list is a host array there too
        auto again = block<uint64_t>(8, 0);
        CHECK(check_index_list("probe", "excluded", idx.get(), 3, 0, false, 1000, 512, again.get(), &per) == 0);
        CHECK(per == 0 && memcmp(again.get(), words.get(), 8 * sizeof(uint64_t)) == 0);
    }
    {   // 65 atoms are two words
        auto idx = block<int32_t>(2, 0);
        idx[0] = 64, idx[1] = 63;
        auto words = block<uint64_t>(2, 0);
        CHECK(check_index_list("probe", "constrained", idx.get(), 2, 0, true, 5, 65, words.get(), &per) == 0);
        CHECK(per == 0 && words[0] == 1ull << 63 && words[1] == 1ull);
    }
    {   // a list per structure on the host: checked, no bits, the slot count for the kernel
        auto idx = block<int32_t>(6, -1);
        idx[1] = 0, idx[2] = 511, idx[4] = 5, idx[5] = 5;
        auto words = block<uint64_t>(8, 0);
        CHECK(check_index_list("probe", "constrained", idx.get(), 2, 1, true, 3, 512, words.get(), &per) == 0);
        CHECK(per == 2);
        for (int w = 0; w < 8; ++w) CHECK(words[w] == 0);
        idx[5] = 512;   // the last slot of the last row
        CHECK(refused(check_index_list("tsc_nci", "constrained", idx.get(), 2, 1, true, 3, 512, words.get(), &per), "tsc_nci: constrained atom 512 with 512 atoms"));
        idx[5] = -2;
        CHECK(refused(check_index_list("tsc_nci", "constrained", idx.get(), 2, 1, true, 3, 512, words.get(), &per), "tsc_nci: constrained atom -2 with 512 atoms"));
    }
    {   // a list per structure on the device is not the host's to read: a block of no elements stands in for it
        auto idx = block<int32_t>(0, 0);
        auto words = block<uint64_t>(8, 0);
        CHECK(check_index_list("probe", "excluded", idx.get(), 4, 1, false, 3, 512, words.get(), &per) == 0);
        CHECK(per == 4);
        for (int w = 0; w < 8; ++w) CHECK(words[w] == 0);
        per = -1;   // no list at all
        CHECK(check_index_list("probe", "excluded", nullptr, 0, 1, true, 3, 512, words.get(), &per) == 0 && per == 0);
    }
    {   // the refusals of a shared list
        auto idx = block<int32_t>(2, 0);
        auto words = block<uint64_t>(8, 0);
        idx[1] = 512;
        CHECK(refused(check_index_list("tsc_bond_delta", "excluded", idx.get(), 2, 0, true, 3, 512, words.get(), &per),
                      "tsc_bond_delta: excluded atom 512 with 512 atoms"));
        idx[1] = -2;
        CHECK(refused(check_index_list("tsc_bond_delta_dev", "excluded", idx.get(), 2, 0, false, 3, 512, words.get(), &per),
                      "tsc_bond_delta_dev: excluded atom -2 with 512 atoms"));
        idx[1] = 4;
        CHECK(refused(check_index_list("tsc_bond_delta", "excluded", idx.get(), 2, 0, true, 3, 4, words.get(), &per), "tsc_bond_delta: excluded atom 4 with 4 atoms"));
    }
    return 0;
}

static int widths() {
    const int atoms[] = {1, 64, 65, 128, 129, 448, 449, 512}, want[] = {1, 1, 2, 2, 3, 7, 8, 8};
    for (int q = 0; q < 8; ++q) {
        int got = 0, calls = 0;
        with_words(atoms[q], [&](auto w) { got = decltype(w)::value, ++calls; });
        CHECK(got == want[q] && calls == 1);
    }
    for (int w = 1; w <= 8; ++w) {
        int got = 0;
        with_width(w, [&](auto v) { got = decltype(v)::value; });
        CHECK(got == w);
    }
    int got = 0;
    with_width(9, [&](auto v) { got = decltype(v)::value; });   // (the widest instantiation for anything beyond it, as the launches had it)
    CHECK(got == 8);
    return 0;
}

int main() {
    if (class_tables() || index_lists() || widths()) return 1;
    printf("call_host_check: %d checks passed\n", g_checks);
    return 0;
}
