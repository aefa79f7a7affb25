// owned.hpp -- who owns device blocks of a context's cache, and the one rule of the objects that are created from a context and live longer than
// a call (tsc_prune, tsc_rot_corr, tsc_rot_corr_batch, tsc_embed_prune, tsc_xchg): the base they derive from, the list a context keeps of them.
// No kernel and no HIP call.  common.hpp includes this in front of tsc_ctx, which holds the list, and defines behind it what needs the context
// itself: Scratch's three dealings with the cache and the one destroy path, destroy_owned.
#pragma once

#include <algorithm>
#include <cstddef>
#include <mutex>
#include <type_traits>
#include <vector>

struct tsc_ctx;
struct tsc_prune;

namespace tsc {

// Blocks of a context's cache, all handed back when this goes: the scratch of one call, or (Owned) what an object holds for as long as it lives.
struct Scratch {
    tsc_ctx *ctx;
    std::vector<void *> blocks;
    explicit Scratch(tsc_ctx *c) : ctx(c) {}
    ~Scratch();
    int take(size_t bytes, void **out);
    void give_back(void *p);   // one block ahead of the rest, recycled in stream order like them (null, or not one of them: nothing happens)
    template <typename T>
    int get(size_t count, T **out) {
        void *p = nullptr;
        if (int rc = take(count * sizeof(T), &p)) return rc;
        *out = static_cast<T *>(p);
        return 0;
    }
};

// What a context owns.  Beside the blocks, a kind's destructor gives back what else it holds; unlisted() is called once, with the list's mutex
// held, when the object leaves its context's list: for what a kind keeps IN the context and must change in one critical section with that.
struct Owned : Scratch {
    using Scratch::Scratch;
    virtual ~Owned() {}
    virtual void unlisted() {}
    // what a HostCall allocated and filled while the object was made is the object's once all is in place (an error before: back with the call)
    void take_blocks(Scratch &call) { blocks.swap(call.blocks); }
};

// The live objects of one context, oldest first.  `mutex` is public: tsc_prune keeps more in the context than its entry here and changes
// both under it (adopt_locked).
class OwnedList {
    std::vector<Owned *> items_;

   public:
    std::mutex mutex;
    void adopt_locked(Owned *o) { items_.push_back(o); }
    void adopt(Owned *o) {
        std::lock_guard<std::mutex> lock(mutex);
        adopt_locked(o);
    }
    bool empty() {
        std::lock_guard<std::mutex> lock(mutex);
        return items_.empty();
    }
    // o leaves the list and is the caller's to delete (a pointer the list does not hold: nothing happens)
    void disown(Owned *o) {
        std::lock_guard<std::mutex> lock(mutex);
        auto it = std::find(items_.begin(), items_.end(), o);
        if (it == items_.end()) return;
        items_.erase(it);
        o->unlisted();
    }
    // Whatever is still listed is deleted, newest first (no kind holds another across calls; this is the reverse of creation).  Everything is
    // off the list before the first destructor runs and the mutex is free meanwhile: a destructor that disowns itself finds nothing to do.
    void destroy_all() {
        std::vector<Owned *> all;
        {
            std::lock_guard<std::mutex> lock(mutex);
            all.assign(items_.rbegin(), items_.rend());
            items_.clear();
            for (Owned *o : all) o->unlisted();
        }
        for (Owned *o : all) delete o;
    }
};

// Does tsc_<kind>_destroy wait for the context's stream before the object goes?  Every kind but tsc_prune: their entry points wait for what
// they enqueue, a destroy is rare, and tsc_xchg frees memory that is not the cache's.  tsc_prune does NOT and must not: its blocks go back to
// the cache in stream order -- whoever gets one next enqueues behind the kernels that still use it -- and a pipeline step creates and
// destroys a run per call, inside what the benchmark times.  A wait here is a wait in the hot path.
template <typename T>
constexpr bool destroy_waits = !std::is_same<T, tsc_prune>::value;

}  // namespace tsc
