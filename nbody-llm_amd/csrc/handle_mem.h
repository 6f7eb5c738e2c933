// handle_mem.h -- the owner of every device and pinned allocation of a handle: a registry of what is live, the one grow of a
// pointer-and-cap pair, and a scoped scratch block.  Free of HIP: the four runtime calls come in through MemSeam, fixed at
// construction (nbody_handle.h supplies the HIP-backed one; tools/sanitize_handle_mem.cpp a malloc-backed one that counts).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <vector>

namespace nbody {

// an allocation sets *p and returns 0, or leaves *p alone and returns the runtime's error code (hipError_t behind the handle)
struct MemSeam {
    int (*dev_alloc)(void** p, size_t bytes);
    void (*dev_free)(void* p);
    int (*pin_alloc)(void** p, size_t bytes);
    void (*pin_free)(void* p);
};

// how far a grow-only buffer that holds fewer than n elements is grown
enum class Grow { exact, quarter, half };   // n | n + n / 4 + 1024 | n + n / 2 + 1024
inline size_t grow_cap(Grow rule, size_t n) {
    return rule == Grow::exact ? n : rule == Grow::quarter ? n + n / 4 + 1024 : n + n / 2 + 1024;
}

class HandleMem {
public:
    explicit HandleMem(const MemSeam& seam) : seam_(seam) {}
    HandleMem(const HandleMem&) = delete;
    HandleMem& operator=(const HandleMem&) = delete;

    // `bytes` of device / pinned memory into p.  A block p still holds is freed first; a failure leaves p null.
    template <class T> int dev(T*& p, size_t bytes) { return alloc(dev_, seam_.dev_alloc, seam_.dev_free, p, bytes); }
    template <class T> int pin(T*& p, size_t bytes) { return alloc(pin_, seam_.pin_alloc, seam_.pin_free, p, bytes); }
    // p's block back to the runtime, p nulled.  Null: nothing.  A pointer the registry does not hold is a programming error:
    // reported (bad_frees), and no runtime free is attempted.
    template <class T> void free_dev(T*& p) { release(dev_, seam_.dev_free, p); }
    template <class T> void free_pin(T*& p) { release(pin_, seam_.pin_free, p); }
    // every live block back to the runtime (the pointers that named them dangle: the handle is going away)
    void release_all() {
        for (void* p : dev_) seam_.dev_free(p);
        for (void* p : pin_) seam_.pin_free(p);
        dev_.clear();
        pin_.clear();
    }

    // The one grow of a pointer-and-cap pair (cap in elements of elem_bytes): nothing when n <= cap, else the old block is
    // freed and one of grow_cap(rule, n) elements allocated.  A failure leaves p null and cap 0.
    template <class T> int grow(T*& p, size_t& cap, size_t n, size_t elem_bytes, Grow rule) {
        if (n <= cap) return 0;
        cap = 0;
        const size_t want = grow_cap(rule, n);
        const int e = dev(p, want * elem_bytes);
        if (!e) cap = want;
        return e;
    }
    // ... keeping the first `keep` elements: copy(fresh, old, bytes) moves them (bytes == 0 when there is nothing to keep; it
    // also waits for whatever still reads the old block) before the old block is freed.  When the allocation or the copy fails
    // the fresh block is freed and p, cap and the old block stay as they were.
    template <class T, class Copy> int grow_keep(T*& p, size_t& cap, size_t n, size_t elem_bytes, Grow rule, size_t keep, Copy copy) {
        if (n <= cap) return 0;
        const size_t want = grow_cap(rule, n);
        T* fresh = nullptr;
        int e = dev(fresh, want * elem_bytes);
        if (e) return e;
        e = copy(static_cast<void*>(fresh), static_cast<const void*>(p), (p ? keep : 0) * elem_bytes);
        if (e) { free_dev(fresh); return e; }
        free_dev(p);
        p = fresh;
        cap = want;
        return 0;
    }

    size_t live_dev() const { return dev_.size(); }
    size_t live_pin() const { return pin_.size(); }
    int bad_frees = 0;   // frees of pointers the registry did not hold

private:
    template <class T>
    int alloc(std::vector<void*>& live, int (*get)(void**, size_t), void (*give)(void*), T*& p, size_t bytes) {
        release(live, give, p);
        void* fresh = nullptr;
        const int e = get(&fresh, bytes);
        if (e) return e;
        live.push_back(fresh);
        p = static_cast<T*>(fresh);
        return 0;
    }
    template <class T>
    void release(std::vector<void*>& live, void (*give)(void*), T*& p) {
        if (!p) return;
        void* const block = const_cast<void*>(static_cast<const void*>(p));
        p = nullptr;
        const auto it = std::find(live.rbegin(), live.rend(), block);
        if (it == live.rend()) {
            ++bad_frees;
            std::fprintf(stderr, "HandleMem: free of %p, which this handle does not own\n", block);
            return;
        }
        *it = live.back();
        live.pop_back();
        give(block);
    }

    MemSeam seam_;
    std::vector<void*> dev_, pin_;
};

// a device block for the length of a scope: taken from the handle's registry, given back when the scope ends
class ScratchDev {
public:
    explicit ScratchDev(HandleMem& mem) : mem_(mem) {}
    ~ScratchDev() { mem_.free_dev(p_); }
    ScratchDev(const ScratchDev&) = delete;
    ScratchDev& operator=(const ScratchDev&) = delete;
    int alloc(size_t bytes) { return mem_.dev(p_, bytes); }
    template <class T = void> T* get() const { return static_cast<T*>(p_); }

private:
    HandleMem& mem_;
    void* p_ = nullptr;
};

}  // namespace nbody
