// owned_check.cpp -- the ownership rule of csrc/owned.hpp (the base of the objects created from a context, and the list the context keeps
// of them) run by a stand-alone program on a context that never saw a device, so that it can be built with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Not part of the library; tools/owned_check.py builds and runs it.  The objects' destructors record
// themselves; their "device blocks" are addresses inside a host array that the context's cache is told about and nobody dereferences.
// No HIP runtime call is made: the program needs no GPU.
//
//   owned_check        (exit status 0 and a line "owned_check: N checks passed", or the first failed check and status 1)
#include <cstdio>
#include <thread>
#include <vector>

#include "../../tscode_amd/csrc/common.hpp"

using namespace tsc;

static int g_checks = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        ++g_checks;                                                    \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static std::vector<int> g_destroyed, g_unlisted;

struct Probe : Owned {
    int id;
    bool disowns_itself;   // as an entry point's destroy does before it deletes -- here from the destructor, the latest it can be
    Probe(tsc_ctx *c, int i, bool self = false) : Owned(c), id(i), disowns_itself(self) {}
    ~Probe() override {
        if (disowns_itself) ctx->owned.disown(this);
        g_destroyed.push_back(id);
    }
    void unlisted() override { g_unlisted.push_back(id); }
};

static void reset() { g_destroyed.clear(), g_unlisted.clear(); }

static int order_and_once() {
    tsc_ctx c;
    // an empty list: the context whose creation failed before anything was made from it
    CHECK(c.owned.empty());
    c.owned.destroy_all();
    CHECK(c.owned.empty() && g_destroyed.empty());
    // five listed, destroyed with the context: each once, newest first, each told that it left the list
    reset();
    for (int i = 0; i < 5; ++i) c.owned.adopt(new Probe(&c, i));
    CHECK(!c.owned.empty());
    c.owned.destroy_all();
    CHECK((g_destroyed == std::vector<int>{4, 3, 2, 1, 0}) && g_unlisted == g_destroyed && c.owned.empty());
    c.owned.destroy_all();   // (again: nothing is left)
    CHECK(g_destroyed.size() == 5);
    // one destroyed by hand beforehand -- disown, then delete, the steps of destroy_owned -- is not touched again
    reset();
    Probe *p[4];
    for (int i = 0; i < 4; ++i) c.owned.adopt(p[i] = new Probe(&c, i));
    c.owned.disown(p[2]);
    CHECK(g_unlisted == std::vector<int>{2});
    delete p[2];
    CHECK(g_destroyed == std::vector<int>{2});
    c.owned.destroy_all();
    CHECK((g_destroyed == std::vector<int>{2, 3, 1, 0}) && (g_unlisted == std::vector<int>{2, 3, 1, 0}));
    return 0;
}

static int unknown_and_self() {
    tsc_ctx c;
    // a pointer the list does not hold (an object that failed before it was listed; one already disowned): nothing happens
    reset();
    Probe stranger(&c, 100), *listed = new Probe(&c, 7);
    c.owned.disown(&stranger);
    c.owned.disown(nullptr);
    c.owned.adopt(listed);
    c.owned.disown(&stranger);
    CHECK(g_unlisted.empty() && !c.owned.empty());
    c.owned.disown(listed);
    c.owned.disown(listed);
    CHECK(g_unlisted == std::vector<int>{7} && c.owned.empty());
    delete listed;
    // every object disowns itself while destroy-all runs: it is off the list by then and the mutex is free
    reset();
    for (int i = 0; i < 6; ++i) c.owned.adopt(new Probe(&c, i, true));
    c.owned.destroy_all();
    CHECK((g_destroyed == std::vector<int>{5, 4, 3, 2, 1, 0}) && g_unlisted == g_destroyed && c.owned.empty());
    reset();   // (`stranger` goes with the scope: never listed, never told)
    return 0;
}

// The blocks of an object are the context's: out of its cache while the object lives, back in it when it dies.
static int blocks_go_back() {
    static char arena[8 * 256];
    tsc_ctx c;
    for (int i = 0; i < 8; ++i) c.cache.emplace(256, arena + 256 * i);   // (what earlier calls left: alloc() finds them, no device is asked)
    {
        Probe a(&c, 0);
        double *x = nullptr, *y = nullptr;
        char *z = nullptr;
        CHECK(a.get(32, &x) == 0 && a.get(1, &y) == 0 && a.get(256, &z) == 0);
        CHECK(a.blocks.size() == 3 && c.live.size() == 3 && c.cache.size() == 5);
        a.give_back(y);
        a.give_back(y);         // (no longer the object's: nothing happens)
        a.give_back(nullptr);
        a.give_back(arena + 7 * 256 + 1);
        CHECK(a.blocks.size() == 2 && c.live.size() == 2 && c.cache.size() == 6);
        // what a HostCall allocated for the object becomes the object's, and what the object had goes back with the call
        Scratch call(&c);
        int32_t *u = nullptr;
        CHECK(call.get(8, &u) == 0 && c.live.size() == 3);
        Probe b(&c, 1);
        b.take_blocks(call);
        CHECK(b.blocks.size() == 1 && b.blocks[0] == u && call.blocks.empty());
    }
    CHECK(c.live.empty() && c.cache.size() == 8);
    return 0;
}

static int two_threads() {
    tsc_ctx c;
    reset();
    Probe *keeper = new Probe(&c, -1);
    c.owned.adopt(keeper);
    auto work = [&c](int base, std::vector<Probe *> *mine) {
        for (int i = 0; i < 1000; ++i) {
            mine->push_back(new Probe(&c, base + i));
            c.owned.adopt(mine->back());
            if (i % 2) c.owned.disown(mine->back());   // every other one leaves at once, the rest at the end, oldest first
        }
        for (Probe *p : *mine) c.owned.disown(p);       // (a second time for those that left: nothing happens)
    };
    std::vector<Probe *> got[2];
    std::thread t0(work, 0, &got[0]), t1(work, 1000, &got[1]);
    t0.join(), t1.join();
    CHECK(got[0].size() == 1000 && got[1].size() == 1000 && g_unlisted.size() == 2000);
    CHECK(!c.owned.empty());
    c.owned.disown(keeper);
    CHECK(c.owned.empty() && g_unlisted.size() == 2001);
    delete keeper;
    for (auto &v : got)
        for (Probe *p : v) delete p;
    CHECK(g_destroyed.size() == 2001);
    return 0;
}

int main() {
    if (order_and_once() || unknown_and_self() || blocks_go_back() || two_threads()) return 1;
    printf("owned_check: %d checks passed\n", g_checks);
    return 0;
}
