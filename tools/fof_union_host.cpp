// fof_union_host.cpp -- the union-find of csrc/fof_union.h on the host: 8 threads unite random and adversarial edge lists
// through relaxed std::atomic<int> operations, then every body's root must be the lowest index of its component as a serial
// union-find sees it.  Meant to be built with -fsanitize=thread: it exercises the termination and lowest-root argument of the
// header (no lock, no wait, every word only decreases) before k_fof_link runs on a device.
//
//     g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -I nbody-llm_amd/csrc tools/fof_union_host.cpp -o fof_union_host
//     ./fof_union_host [lists]        (default 2000; prints "fof_union_host ok: ..." and returns 0, or says what differs)
#include "fof_union.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

namespace {

using Edges = std::vector<std::pair<int, int>>;
constexpr int kThreads = 8;

struct HostParent {
    std::atomic<int>* p;
    int load(int x) const { return p[x].load(std::memory_order_relaxed); }
    int cas(int x, int expect, int want) const {
        p[x].compare_exchange_strong(expect, want, std::memory_order_relaxed);
        return expect;   // (what the word was: `expect` itself on success)
    }
    void lower(int x, int v) const {   // atomicMin: a failed exchange means someone else lowered the word
        int cur = p[x].load(std::memory_order_relaxed);
        while (cur > v && !p[x].compare_exchange_strong(cur, v, std::memory_order_relaxed)) {}
    }
};

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    int below(int n) { return int(next() % uint64_t(n)); }
};

void shuffle(Edges& e, Rng& r) {
    for (size_t k = e.size(); k > 1; --k) std::swap(e[k - 1], e[size_t(r.below(int(k)))]);
}

std::vector<int> permutation(int n, Rng& r) {
    std::vector<int> p(size_t(n), 0);
    std::iota(p.begin(), p.end(), 0);
    for (int k = n; k > 1; --k) std::swap(p[size_t(k - 1)], p[size_t(r.below(k))]);
    return p;
}

// kind 0: random edges, about n / 2 of them (many small components); 1: random, 2 n (a giant component); 2: chains -- a path
// through a random permutation of the bodies, cut in a few places, edges in scrambled order; 3: stars -- a few hubs, everybody
// else tied to one of them; 4: every edge twice and both ways round
Edges make_edges(int kind, int n, Rng& r) {
    Edges e;
    if (n < 2) return e;
    if (kind == 0 || kind == 1 || kind == 4) {
        const int m = kind == 1 ? 2 * n : n / 2;
        for (int k = 0; k < m; ++k) {
            const int a = r.below(n), b = r.below(n);
            e.emplace_back(a, b);
            if (kind == 4) e.emplace_back(b, a);
        }
    } else if (kind == 2) {
        const std::vector<int> p = permutation(n, r);
        const int cuts = 1 + r.below(3);
        for (int k = 0; k + 1 < n; ++k)
            if (r.below(n) >= cuts) e.emplace_back(p[size_t(k)], p[size_t(k + 1)]);
    } else {
        const int hubs = 1 + r.below(3);
        const std::vector<int> p = permutation(n, r);
        for (int k = hubs; k < n; ++k) {
            const int hub = p[size_t(r.below(hubs))];
            if (r.below(2)) e.emplace_back(hub, p[size_t(k)]);
            else e.emplace_back(p[size_t(k)], hub);
        }
    }
    shuffle(e, r);
    return e;
}

std::vector<int> serial_min_labels(int n, const Edges& e) {
    std::vector<int> parent(size_t(n), 0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&parent](int x) {
        while (parent[size_t(x)] != x) x = parent[size_t(x)] = parent[size_t(parent[size_t(x)])];
        return x;
    };
    for (const auto& ab : e) {
        const int a = find(ab.first), b = find(ab.second);
        if (a != b) parent[size_t(std::max(a, b))] = std::min(a, b);
    }
    std::vector<int> label(size_t(n), 0);
    for (int i = 0; i < n; ++i) label[size_t(i)] = find(i);
    return label;
}

// the edges dealt to kThreads threads round-robin (neighbouring edges of the list run at the same time)
bool run_list(int kind, int n, uint64_t seed) {
    Rng r{seed};
    const Edges e = make_edges(kind, n, r);
    std::unique_ptr<std::atomic<int>[]> words(new std::atomic<int>[size_t(std::max(n, 1))]);
    for (int i = 0; i < n; ++i) words[size_t(i)].store(i, std::memory_order_relaxed);
    const HostParent parent{words.get()};
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&e, parent, t] {
            for (size_t k = size_t(t); k < e.size(); k += kThreads) nbody::fof::fof_link(parent, e[k].first, e[k].second);
        });
    for (std::thread& t : pool) t.join();
    const std::vector<int> want = serial_min_labels(n, e);
    for (int i = 0; i < n; ++i) {
        const int p = parent.load(i);
        if (p > i) {
            std::fprintf(stderr, "kind %d n %d seed %llu: parent[%d] = %d is above it\n", kind, n, (unsigned long long)seed, i, p);
            return false;
        }
        int root = i;   // (plain chain walk: the threads are joined)
        while (parent.load(root) != root) root = parent.load(root);
        if (root != want[size_t(i)]) {
            std::fprintf(stderr, "kind %d n %d seed %llu: body %d has root %d, its component's lowest index is %d\n", kind, n,
                         (unsigned long long)seed, i, root, want[size_t(i)]);
            return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int lists = argc > 1 ? std::atoi(argv[1]) : 2000;
    Rng sizes{12345};
    int done = 0;
    for (int k = 0; k < lists; ++k) {
        const int kind = k % 5;
        const int n = k < 10 ? k / 5 * 2 + (k % 2) : 2 + sizes.below(k % 97 == 0 ? 4000 : 300);   // 0, 1, 2 and 3 bodies first
        if (!run_list(kind, n, 1000 + uint64_t(k))) return 1;
        ++done;
    }
    // long ones: a chain and a star of 100 000 bodies
    if (!run_list(2, 100000, 7) || !run_list(3, 100000, 8)) return 1;
    std::printf("fof_union_host ok: %d lists and 2 long ones from %d threads, every root its component's lowest index\n", done, kThreads);
    return 0;
}
