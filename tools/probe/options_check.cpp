// options_check.cpp -- the option table of csrc/options.hpp (every tunable's name, default and rule; what tsc_ctx_set_option,
// tsc_ctx_get_option and tsc_option_info run) walked by a stand-alone program, so that it can be checked without a GPU and built with
// AddressSanitizer and UndefinedBehaviorSanitizer.  Not part of the library; tools/options_check.py builds and runs it.  Includes
// options.hpp only; no HIP runtime call is made.  The values tried for a row come from the row's own rule and numbers: the program
// holds no second list of the options.
//
//   options_check          (exit status 0 and a line "options_check: N checks passed", or the first failed check and status 1)
//   options_check --list   (one line "name default" per option, in the table's order)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <set>
#include <string>
#include <vector>

#include "../../tscode_amd/csrc/options.hpp"

using namespace tsc;

static int g_checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++g_checks;                                              \
        if (!(cond)) {                                           \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_what); \
            return 1;                                            \
        }                                                        \
    } while (0)

static const char *g_what = "";
static char g_msg[512];

static int set(tsc_options &o, const char *name, double v) { return option_set(o, name, v, g_msg, sizeof(g_msg)); }
static double get(const tsc_options &o, const char *name) {
    double v = NAN;
    return option_get(o, name, &v, g_msg, sizeof(g_msg)) == 0 ? v : NAN;
}

// one value the row accepts that is not `def`, and the values just outside its rule
static double other_value(const OptionRow &r, double def) {
    switch (r.rule) {
    case OPT_ONE_OF: return r.a != def ? r.a : r.b;
    case OPT_RANGE:
    case OPT_WHOLE:
    case OPT_ZERO_OR_MULTIPLE: return r.a != def ? r.a : r.b;
    case OPT_AT_LEAST: return r.a + 1 != def ? r.a + 1 : r.a + 2;
    case OPT_FLAG: return 1 - def;
    default: return def + 1;
    }
}
static std::vector<double> refused_values(const OptionRow &r) {
    switch (r.rule) {
    case OPT_ONE_OF: return {std::fmin(r.a, std::fmin(r.b, r.m)) - 1, std::fmax(r.a, std::fmax(r.b, r.m)) + 1, r.a + 0.5, NAN};
    case OPT_RANGE: return {r.a - 1, r.b + 1, NAN};
    case OPT_ZERO_OR_MULTIPLE: return {r.a - 1, r.b + 1, r.a + r.m / 2, -r.m, NAN};
    case OPT_WHOLE: return {r.a - 1, r.b + 1, r.a + 0.5, NAN};
    case OPT_AT_LEAST: return {r.a - 1, r.a - 0.5, NAN};
    default: return {};
    }
}

static int rows() {
    for (const OptionRow &r : OPTION_TABLE) {
        g_what = r.name;
        tsc_options o;
        const double def = r.get(tsc_options());
        // the default is a value the row takes, and comes back
        CHECK(get(o, r.name) == def);
        CHECK(set(o, r.name, def) == 0 && get(o, r.name) == def);
        // one other accepted value is stored -- in this option only
        const double v = other_value(r, def);
        CHECK(v != def && set(o, r.name, v) == 0 && get(o, r.name) == v);
        for (const OptionRow &q : OPTION_TABLE) CHECK(&q == &r || q.get(o) == q.get(tsc_options()));
        // just outside the rule: refused, with the option's name and the value in the message, and the stored value stays
        for (double bad : refused_values(r)) {
            g_msg[0] = 0;
            CHECK(set(o, r.name, bad) == TSC_ERR_INVALID);
            CHECK(strstr(g_msg, r.name) == g_msg && strstr(g_msg, "must be") && strstr(g_msg, "(got "));
            CHECK(get(o, r.name) == v);
        }
        CHECK(set(o, r.name, def) == 0 && get(o, r.name) == def);
    }
    g_what = "";
    return 0;
}

static int unknown_names() {
    tsc_options o;
    double v = 7;
    for (const char *name : {"no_such_option", "", "cull_", "Cull", "prune_algo ", "dbg_stamp_"}) {
        g_what = name;
        const std::string want = std::string("unknown option '") + name + "'";
        CHECK(set(o, name, 1) == TSC_ERR_INVALID && want == g_msg);
        g_msg[0] = 0;
        CHECK(option_get(o, name, &v, g_msg, sizeof(g_msg)) == TSC_ERR_INVALID && want == g_msg && v == 7);
    }
    g_what = "";
    return 0;
}

static int info_walk() {
    std::set<std::string> seen;
    int n = 0;
    const char *name = nullptr;
    double def = NAN;
    while (option_info(n, &name, &def) == 0) {
        g_what = name;
        CHECK(name == OPTION_TABLE[n].name && seen.insert(name).second);   // (every name once)
        CHECK(def == get(tsc_options(), name));                            // (the default is what a fresh context holds)
        ++n;
        CHECK(n <= 1000);
    }
    g_what = "";
    CHECK(n == int(sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0])) && n >= 28);
    CHECK(option_info(-1, &name, &def) == TSC_ERR_INVALID && option_info(n + 1, &name, &def) == TSC_ERR_INVALID);
    CHECK(option_info(0, nullptr, nullptr) == 0);
    return 0;
}

// what the rules leave as it always was
static int oddities() {
    tsc_options o;
    // fractions are cut off, also where the rule looks at the whole part only; a double member keeps them
    g_what = "truncation";
    CHECK(set(o, "drain_min", 7.9) == 0 && o.drain_min == 7 && get(o, "drain_min") == 7);
    CHECK(set(o, "drain_min", 64.5) == TSC_ERR_INVALID && o.drain_min == 7);
    CHECK(set(o, "mm_min_n", 1234.9) == 0 && o.mm_min_n == 1234);
    CHECK(set(o, "seg_cols", 512.7) == 0 && o.seg_cols == 512 && set(o, "mm_seg_cols", 64.5) == 0 && o.mm_seg_cols == 64);
    CHECK(set(o, "prune_batch_max_n", 100.5) == TSC_ERR_INVALID && o.prune_batch_max_n == 2048 && set(o, "prune_batch_max_n", 100) == 0 && o.prune_batch_max_n == 100);
    CHECK(set(o, "cull_grid", 100.9) == 0 && o.cull_grid == 100);
    CHECK(set(o, "cull_min_pairs", 0.5) == 0 && o.cull_min_pairs == 0.5 && get(o, "cull_min_pairs") == 0.5);
    // "open_lds_blocks" stores 2^30 for anything above
    g_what = "clamp";
    CHECK(set(o, "open_lds_blocks", 4e9) == 0 && o.open_lds_blocks == (1 << 30) && set(o, "open_lds_blocks", INFINITY) == 0 && o.open_lds_blocks == (1 << 30));
    CHECK(set(o, "open_lds_blocks", 1073741823.0) == 0 && o.open_lds_blocks == (1 << 30) - 1 && set(o, "open_lds_blocks", 0) == 0 && o.open_lds_blocks == 0);
    // non-zero means 1
    g_what = "flag";
    for (const char *name : {"deterministic_basis", "cull_xcd"}) {
        for (double v : {5.0, -3.0, 0.25, 1.0}) CHECK(set(o, name, 0) == 0 && get(o, name) == 0 && set(o, name, v) == 0 && get(o, name) == 1);
    }
    // unchecked
    g_what = "unchecked";
    for (double v : {7.0, -1.0, 0.0, 2.0}) CHECK(set(o, "stage1_f32", v) == 0 && o.stage1_f32 == int(v));
    CHECK(set(o, "stage1_f32", 2.9) == 0 && o.stage1_f32 == 2);
    CHECK(want_heavy32(o, 1.0) && set(o, "stage1_f32", 7) == 0 && !want_heavy32(o, 1e12));   // (2: always; any other value but 1: never)
#ifdef TSC_DBG_STAMPS
    CHECK(get(o, "dbg_stamp_k") == -1 && set(o, "dbg_stamp_k", -12345678901.0) == 0 && o.dbg_stamp_k == -12345678901LL);
#else
    CHECK(set(o, "dbg_stamp_k", 1) == TSC_ERR_INVALID);
#endif
    g_what = "";
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "--list") == 0) {
        const char *name;
        double def;
        for (int i = 0; option_info(i, &name, &def) == 0; ++i) printf("%s %.17g\n", name, def);
        return 0;
    }
    if (rows() || unknown_names() || info_walk() || oddities()) return 1;
    printf("options_check: %d checks passed\n", g_checks);
    return 0;
}
