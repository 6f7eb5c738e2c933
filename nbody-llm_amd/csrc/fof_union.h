// fof_union.h -- the lock-free union-find of the friends-of-friends group finder (kernels_fof.hip, k_fof_link), written once
// over the atomic operations it needs so that the same text runs on the device against parent[] in global memory and on the
// host against std::atomic<int> (tools/fof_union_host.cpp, under ThreadSanitizer).
//
// `P` names one parent[] array and supplies three operations, each atomic on one word and relaxed:
//     int  load(int x)                      the word, or ANY value it held earlier (a stale read is allowed)
//     int  cas(int x, int expect, int want) parent[x] = want if it is `expect`; returns what it was (never stale)
//     void lower(int x, int v)              parent[x] = min(parent[x], v)
//
// THE INVARIANT.  parent[x] <= x; a word only ever DECREASES; and it always names a body of x's own tree -- hence of x's
// connected component, because trees are joined only along links.  The three writes keep it:
//   - fof_unite's cas(hi, hi, lo) with lo < hi succeeds only while hi is a root at that instant (the cas is not stale).  A root
//     is the lowest index of its tree (every chain descends), so lo < hi lies in ANOTHER tree: the cas hangs one whole tree
//     under a body of the tree it is linked to.  lo itself may have stopped being a root; that does not matter.
//   - fof_find's lower(x, g) replaces x's parent by a body g < x that was an ancestor of x at some earlier time.  Trees never
//     split, so g is still in x's tree.
// So a stale read costs steps, never correctness: every value a word ever held is <= x and in x's tree, every chain strictly
// descends and ends at a word that reads parent[r] == r, and two bodies whose finds (stale or not) end at the same r are in one
// tree already.  When every link has been united and all writes are visible (the kernel boundary), a tree is exactly one
// connected component and its one root is the component's lowest index.
//
// NOBODY WAITS.  fof_find walks down at most x steps.  fof_unite's loop repeats only after a lost cas, which returned a value
// below hi: someone else lowered that word, and (hi + lo) strictly falls from one iteration to the next.  There is no lock, no
// flag to spin on and no exit that depends on another thread making progress.
#pragma once

#if defined(__HIPCC__)
#define FOF_HD __host__ __device__ __forceinline__
#else
#define FOF_HD inline
#endif

namespace nbody { namespace fof {

// a body r of x's tree with parent[r] == r as read; halves the path on the way (x's parent becomes its grandparent)
template <class P>
FOF_HD int fof_find(const P& parent, int x) {
    for (;;) {
        const int p = parent.load(x);
        if (p == x) return x;
        const int g = parent.load(p);   // g <= p < x
        if (g < p) parent.lower(x, g);
        x = g;
    }
}

// joins the trees of a and b: on return they are one tree (it may be one that other threads are still lowering)
template <class P>
FOF_HD void fof_unite(const P& parent, int a, int b) {
    for (;;) {
        a = fof_find(parent, a);
        b = fof_find(parent, b);
        if (a == b) return;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int was = parent.cas(hi, hi, lo);
        if (was == hi) return;
        a = was;   // < hi, and in hi's tree: go on from there
        b = lo;
    }
}

// the link of bodies i and j: nothing to do when their parent words already read equal (one tree)
template <class P>
FOF_HD void fof_link(const P& parent, int i, int j) {
    if (parent.load(i) == parent.load(j)) return;
    fof_unite(parent, i, j);
}

}}  // namespace nbody::fof
