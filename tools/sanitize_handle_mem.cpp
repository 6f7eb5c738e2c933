// sanitize_handle_mem.cpp -- the bookkeeping of nbody-llm_amd/csrc/handle_mem.h (the registry of a handle's device and pinned
// blocks, the one grow, the scoped scratch) over a malloc-backed seam that counts its calls and can fail the k-th allocation.
// And the carver of nbody-llm_amd/csrc/scratch_carve.h, which lays a call's scratch out inside one such block.
// Built with -fsanitize=address,undefined by tests/test_handle_mem.py; prints "ok" only when every check held.
#include "handle_mem.h"
#include "scratch_carve.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using nbody::Grow;
using nbody::HandleMem;
using nbody::ScratchDev;

namespace {

int g_allocs = 0, g_frees = 0;     // successful allocations, frees that reached the seam
int g_fail_at = 0;                 // > 0: the g_fail_at-th allocation from now fails
std::set<void*> g_live;            // what the seam has handed out and not taken back
int g_double_frees = 0;

int seam_alloc(void** p, size_t bytes) {
    if (g_fail_at > 0 && --g_fail_at == 0) return 2;   // (hipErrorOutOfMemory's value; any non-zero code)
    void* q = std::malloc(bytes ? bytes : 1);
    if (!q) return 2;
    g_live.insert(q);
    ++g_allocs;
    *p = q;
    return 0;
}
void seam_free(void* p) {
    if (!g_live.erase(p)) { ++g_double_frees; return; }
    ++g_frees;
    std::free(p);
}
const nbody::MemSeam kSeam{seam_alloc, seam_free, seam_alloc, seam_free};

int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

bool balanced() { return g_allocs == g_frees && g_live.empty() && g_double_frees == 0; }

// 1: after a mixed sequence release_all frees exactly the live blocks, each once; a second one does nothing
void check_release_all() {
    HandleMem m(kSeam);
    int* a = nullptr; double* b = nullptr; char* c = nullptr; void* pinned = nullptr; float* g = nullptr;
    size_t g_cap = 0;
    CHECK(m.dev(a, 40) == 0 && m.dev(b, 80) == 0 && m.dev(c, 1) == 0 && m.pin(pinned, 64) == 0);
    CHECK(m.grow(g, g_cap, 10, sizeof(float), Grow::quarter) == 0);
    CHECK(m.grow(g, g_cap, 5000, sizeof(float), Grow::half) == 0);
    m.free_dev(b);
    CHECK(b == nullptr);
    CHECK(m.dev(a, 400) == 0);   // replaces the block a held
    CHECK(m.live_dev() == 3 && m.live_pin() == 1 && g_live.size() == 4);
    m.release_all();
    CHECK(m.live_dev() == 0 && m.live_pin() == 0 && balanced());
    const int frees = g_frees;
    m.release_all();
    CHECK(g_frees == frees && balanced() && m.bad_frees == 0);
}

// 2: the capacity after a grow is the rule's formula; a grow to n <= cap allocates nothing
void check_rules() {
    const size_t sizes[] = {0, 1, 1023, 1024, 1025, 100000};
    for (int r = 0; r < 3; ++r)
        for (size_t n : sizes) {
            const Grow rule = r == 0 ? Grow::exact : r == 1 ? Grow::quarter : Grow::half;
            const size_t want = r == 0 ? n : r == 1 ? n + n / 4 + 1024 : n + n / 2 + 1024;
            HandleMem m(kSeam);
            uint16_t* p = nullptr;
            size_t cap = 0;
            const int before = g_allocs;
            CHECK(m.grow(p, cap, n, sizeof(uint16_t), rule) == 0);
            if (n == 0) { CHECK(p == nullptr && cap == 0 && g_allocs == before); continue; }   // (0 <= cap: nothing to do)
            CHECK(cap == want && p != nullptr && g_allocs == before + 1);
            std::memset(p, 0xab, cap * sizeof(uint16_t));   // the block is that large (ASan)
            const uint16_t* was = p;
            CHECK(m.grow(p, cap, cap, sizeof(uint16_t), rule) == 0 && m.grow(p, cap, n / 2, sizeof(uint16_t), rule) == 0);
            CHECK(p == was && cap == want && g_allocs == before + 1);
            m.release_all();
        }
    CHECK(balanced());
}

// 3: a grow whose allocation fails leaves null and 0 with the old block freed; a later grow succeeds
void check_failed_grow() {
    HandleMem m(kSeam);
    int* p = nullptr;
    size_t cap = 0;
    CHECK(m.grow(p, cap, 100, sizeof(int), Grow::exact) == 0);
    const int frees = g_frees;
    g_fail_at = 1;
    CHECK(m.grow(p, cap, 200, sizeof(int), Grow::exact) != 0);
    CHECK(p == nullptr && cap == 0 && g_frees == frees + 1 && m.live_dev() == 0);
    CHECK(m.grow(p, cap, 200, sizeof(int), Grow::quarter) == 0 && p && cap == 200 + 50 + 1024);
    m.release_all();
    CHECK(balanced());
}

// 4: the keeping grow
void check_grow_keep() {
    HandleMem m(kSeam);
    int* p = nullptr;
    size_t cap = 0;
    int copies = 0;
    const auto copy = [&](void* fresh, const void* old, size_t bytes) { ++copies; if (bytes) std::memcpy(fresh, old, bytes); return 0; };
    CHECK(m.grow_keep(p, cap, 8, sizeof(int), Grow::exact, 4, copy) == 0 && cap == 8 && copies == 1);   // (no old block: nothing kept)
    for (int k = 0; k < 8; ++k) p[k] = 100 + k;
    CHECK(m.grow_keep(p, cap, 8, sizeof(int), Grow::half, 8, copy) == 0 && cap == 8 && copies == 1);    // n <= cap
    CHECK(m.grow_keep(p, cap, 50, sizeof(int), Grow::half, 5, copy) == 0 && cap == 50 + 25 + 1024);
    for (int k = 0; k < 5; ++k) CHECK(p[k] == 100 + k);
    CHECK(m.live_dev() == 1);
    // the copy step fails: the fresh block goes, the old one stays live and registered
    int* const old = p;
    const size_t old_cap = cap;
    const int allocs = g_allocs, frees = g_frees;
    CHECK(m.grow_keep(p, cap, 5000, sizeof(int), Grow::quarter, 5, [](void*, const void*, size_t) { return 7; }) == 7);
    CHECK(p == old && cap == old_cap && g_allocs == allocs + 1 && g_frees == frees + 1 && m.live_dev() == 1);
    CHECK(p[4] == 104);
    // the allocation fails: likewise
    g_fail_at = 1;
    CHECK(m.grow_keep(p, cap, 5000, sizeof(int), Grow::quarter, 5, copy) != 0 && p == old && cap == old_cap && m.live_dev() == 1);
    m.free_dev(p);
    CHECK(m.bad_frees == 0 && balanced());
}

// 5: the scoped scratch frees on every exit path
int two_guards(HandleMem& m, int leave_at) {
    ScratchDev a(m);
    if (a.alloc(64)) return -1;
    std::memset(a.get<char>(), 1, 64);
    if (leave_at == 0) return 0;
    ScratchDev b(m);
    if (b.alloc(128)) return -2;   // (a is given back)
    if (leave_at == 1) return 1;
    std::memset(b.get(), 2, 128);
    return 2;
}
void check_scratch() {
    HandleMem m(kSeam);
    for (int leave_at = 0; leave_at < 3; ++leave_at) {
        CHECK(two_guards(m, leave_at) == leave_at);
        CHECK(m.live_dev() == 0 && balanced());
    }
    g_fail_at = 2;   // the second guard's allocation fails
    CHECK(two_guards(m, 2) == -2 && m.live_dev() == 0 && balanced());
    { ScratchDev never(m); }   // a guard that took nothing gives nothing back
    CHECK(balanced() && m.bad_frees == 0);
}

// 6: null is a no-op; a pointer the registry never held is reported and does not reach the seam
void check_bad_free() {
    HandleMem m(kSeam);
    int* none = nullptr;
    const int frees = g_frees;
    m.free_dev(none);
    m.free_pin(none);
    CHECK(g_frees == frees && m.bad_frees == 0);
    int on_stack = 0;
    int* stray = &on_stack;
    m.free_dev(stray);
    CHECK(stray == nullptr && m.bad_frees == 1 && g_frees == frees && g_double_frees == 0);
    int* pinned = nullptr;
    CHECK(m.pin(pinned, 16) == 0);
    int* alias = pinned;
    m.free_dev(alias);   // a pinned block is not a device block
    CHECK(m.bad_frees == 2 && g_frees == frees && m.live_pin() == 1);
    m.free_pin(pinned);
    CHECK(pinned == nullptr && g_frees == frees + 1 && balanced());
}

// 7: the scratch carver (scratch_carve.h) alone: for sequences of (count, type) takes, zero-length ones among them, the
// measuring pass and the placing pass end at the same offset, every block starts at a multiple of 256 bytes, and the blocks are
// disjoint and lie inside the measured size (every byte of every block is written: ASan sees the allocation's end)
struct Take { size_t count, size; };
template <class T>
char* take_as(nbody::Carver& c, size_t count) { return reinterpret_cast<char*>(c.take<T>(count)); }
char* take_one(nbody::Carver& c, const Take& t) {
    struct Wide { double d[5]; };   // 40 bytes: no power of two
    switch (t.size) {
    case 1: return take_as<char>(c, t.count);
    case 4: return take_as<int>(c, t.count);
    case 8: return take_as<double>(c, t.count);
    default: return take_as<Wide>(c, t.count);
    }
}
void check_carver() {
    CHECK(nbody::up256(0) == 0 && nbody::up256(1) == 256 && nbody::up256(256) == 256 && nbody::up256(257) == 512);
    const Take seqs[][6] = {
        {{1, 8}, {257, 4}, {0, 8}, {64, 4}, {3, 40}, {255, 1}},
        {{0, 4}, {0, 8}, {0, 1}, {0, 40}, {0, 4}, {0, 8}},
        {{0, 40}, {1, 1}, {256, 1}, {257, 1}, {0, 4}, {65536, 8}},
        {{7, 40}, {0, 1}, {1, 4}, {1, 4}, {32, 8}, {33, 8}},
    };
    for (const auto& seq : seqs) {
        nbody::Carver measure;
        for (const Take& t : seq) CHECK(take_one(measure, t) == nullptr);
        const size_t bytes = measure.offset();
        char* base = nullptr;
        CHECK(posix_memalign(reinterpret_cast<void**>(&base), 256, bytes ? bytes : 1) == 0);
        nbody::Carver place(base);
        size_t end = 0;   // where the block before ended: the blocks ascend, so disjoint means start >= end
        for (const Take& t : seq) {
            char* p = take_one(place, t);
            const size_t at = size_t(p - base), len = t.count * t.size;
            CHECK(at % 256 == 0 && at >= end && at + len <= bytes);
            std::memset(p, 0x5a, len);
            end = at + len;
        }
        CHECK(place.offset() == bytes && bytes % 256 == 0);
        std::free(base);
    }
}

}  // namespace

int main() {
    check_release_all();
    check_rules();
    check_failed_grow();
    check_grow_keep();
    check_scratch();
    check_bad_free();
    check_carver();
    if (g_failed || !balanced()) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("ok\n");
    return 0;
}
