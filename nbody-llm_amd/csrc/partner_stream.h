// partner_stream.h -- the one-sided partner stream of the read-only f64 pair kernels (kernels_pot.hip k_pot_os, kernels_field.hip
// k_probe_pairs), and the windows the one-sided kernels draw their partners from (those two and kernels_bf64.hip k_bf64_os);
// device code only.  A partner list is the bodies of nw windows, concatenated in window order; a wave takes slice
// [R slice / K, R (slice + 1) / K) of its R bodies, 64 at a time through its own LDS tile, the next 64 prefetched while these
// are read back as wave-uniform broadcasts.
#pragma once
#include "real.h"   // widen

namespace nbody {

struct Win { int seg, lo, hi; };   // one window of partners: bodies [lo, hi) of segment seg

// MODE 0: every own body; MODE 1: what a symmetric kernel over A sets leaves over (the own set and, for even A, the opposite
// set); MODE 2: the other segments' bodies
template <int MODE>
__device__ __forceinline__ int n_windows(int n_seg, int A) {
    return MODE == 0 ? 1 : MODE == 1 ? ((A % 2 == 0 && A > 1) ? 2 : 1) : n_seg - 1;
}

template <int MODE>
__device__ __forceinline__ Win window(int w, const int* __restrict__ seg_count, int my_seg, int n_own, int set_size, int A, int a) {
    if (MODE == 0) return Win{my_seg, 0, n_own};
    if (MODE == 1) {
        int set = (w == 0) ? a : a + A / 2;
        if (set >= A) set -= A;
        const int lo = min(n_own, set * set_size), hi = min(n_own, lo + set_size);
        return Win{my_seg, lo, hi};
    }
    const int s = w < my_seg ? w : w + 1;   // every other segment, in order
    return Win{s, 0, seg_count[s]};
}

// visit(pj, seg, j) for every body of slice `slice` of K of the list win_of(0) .. win_of(nw - 1), in list order: pj the widened
// body, (seg, j) its place -- what a caller that is itself a body compares with its own place, the one use of an index.
// tile: the calling wave's own 64 entries of LDS (its LDS operations complete in program order: no barrier).
template <class P, class WinOf, class Visit>
__device__ __forceinline__ void stream_partners(double4* tile, int lane, const P* __restrict__ pos_all, int seg_cap, int nw, WinOf win_of, int slice,
                                                int K, Visit visit) {
    long long R = 0;
    for (int w = 0; w < nw; ++w) {
        const Win win = win_of(w);
        R += max(0, win.hi - win.lo);
    }
    const long long r0 = R * slice / K, r1 = R * (slice + 1) / K;
    long long first = 0;   // index of the window's first body in the concatenated list
    for (int w = 0; w < nw; ++w) {
        const Win win = win_of(w);
        const int len = max(0, win.hi - win.lo);
        const long long lo = max(r0, first), hi = min(r1, first + len);
        if (lo < hi) {
            const P* __restrict__ ps = pos_all + size_t(win.seg) * seg_cap + win.lo;   // ps[c - first]: body c of the list
            double4 nxt = (lo + lane < hi) ? widen(ps[lo + lane - first]) : make_double4(0.0, 0.0, 0.0, 0.0);   // (lanes past hi: never read back)
            for (long long c0 = lo; c0 < hi; c0 += 64) {
                tile[lane] = nxt;
                if (c0 + 64 + lane < hi) nxt = widen(ps[c0 + 64 + lane - first]);
                const int cnt = int(min(64LL, hi - c0)), j0 = win.lo + int(c0 - first);
                for (int t = 0; t < cnt; ++t) visit(tile[t], win.seg, j0 + t);   // wave-uniform address: an LDS broadcast
            }
        }
        first += len;
    }
}

}  // namespace nbody
