// scratch_carve.h -- how a call's scratch is carved out of one allocation: host code, free of HIP (tools/sanitize_handle_mem.cpp
// drives it on the CPU).  A module describes its blocks once, as a function over a Carver&; run on a measuring carver the
// description gives the bytes to allocate, run on a placing one it gives the pointers, so the two cannot disagree.
#pragma once
#include <cstddef>

namespace nbody {

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// Carver(): measures -- every take returns null and only advances.  Carver(base): places the blocks from base on.  Every block
// starts at a multiple of 256 bytes from base and a block of zero bytes takes no room.
class Carver {
public:
    Carver() = default;
    explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t count) {
        T* p = base_ ? reinterpret_cast<T*>(base_ + at_) : nullptr;
        at_ += up256(count * sizeof(T));
        return p;
    }
    size_t offset() const { return at_; }   // the bytes taken so far

private:
    char* base_ = nullptr;
    size_t at_ = 0;
};

}  // namespace nbody
