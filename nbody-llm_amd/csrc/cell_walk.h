// cell_walk.h -- the one walk of the cell-list kernels (kernels_cells.hip) over the candidates of a gridded body: device code.
//
// The n_gridded bodies stand in key order, one per lane at place s, and key order is (k_x, k_y, k_z) order (cell_grid.h).  The
// three cells k_z - 1 .. k_z + 1 of one (k_x, k_y) column are one contiguous key range, clamped at the walls: two binary
// searches over the sorted keys find its places [a, b).  A column outside the grid is left out.
//
//   Walk::full  the nine columns around the lane's own, searched from place 0; visit(t) for every t != s.  The candidates
//               counted are the places after s: b - max(a, s + 1) where positive.
//   Walk::half  EVERY UNORDERED PAIR ONCE, from its earlier place: a candidate that stands after s lies in the rest of the
//               lane's own column -- from its own cell k_z on, since the cell below holds earlier places only -- or in one of
//               the four columns (0, +1), (+1, -1), (+1, 0), (+1, +1), which key order puts wholly after s.  So the five
//               columns are searched from s + 1, the own column from k_z, and visit(t) is called for every t in them: if t is
//               a candidate of s and t > s this walk reaches it, and s is never reached from t.  The count is b - a.
// Within a cell the places ascend with the original row (the sort is stable), so "earlier" is the lower row there.
#pragma once
#include <hip/hip_runtime.h>
#include "cell_grid.h"

namespace nbody { namespace cells {

enum class Walk { half, full };

// the first place in keys[lo, hi) whose key is >= k (kAfter: > k); hi when there is none
template <bool kAfter>
__device__ __forceinline__ int key_bound(const uint64_t* __restrict__ keys, int lo, int hi, uint64_t k) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const uint64_t v = keys[mid];
        if (kAfter ? v <= k : v < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the places [a, b) of column (cx, cy), cells z0 .. z1, among the n gridded bodies; false: the column lies outside the grid
__device__ __forceinline__ bool column_range(const uint64_t* __restrict__ keys, int from, int n, long long cx, long long cy, uint64_t z0,
                                             uint64_t z1, int* a, int* b) {
    if (cx < 0 || cy < 0 || cx > (long long)kCellMax || cy > (long long)kCellMax) return false;
    *a = key_bound<false>(keys, from, n, cell_key(uint64_t(cx), uint64_t(cy), z0));
    *b = key_bound<true>(keys, *a, n, cell_key(uint64_t(cx), uint64_t(cy), z1));
    return true;
}

// visit(t) for the candidate places of place s < n_gridded; returns how many candidates the lane counts (above)
template <Walk kShape, class Visit>
__device__ __forceinline__ unsigned long long cell_walk(const uint64_t* __restrict__ keys, int n_gridded, int s, Visit&& visit) {
    constexpr bool kHalf = kShape == Walk::half;
    const uint64_t key = keys[s];
    const long long kx = (long long)(key >> (2 * kCellBits)), ky = (long long)((key >> kCellBits) & kCellMax);
    const uint64_t kz = key & kCellMax;
    const uint64_t z0 = kz ? kz - 1 : 0, z1 = kz < kCellMax ? kz + 1 : kCellMax;   // clamped at the walls
    unsigned long long cand = 0;
    for (int c = 0; c < (kHalf ? 5 : 9); ++c) {   // half: (0, 0) | (0, +1) | (+1, -1), (+1, 0), (+1, +1)
        const int dx = kHalf ? c >= 2 : c / 3 - 1, dy = !kHalf ? c % 3 - 1 : c == 0 ? 0 : c == 1 ? 1 : c - 3;
        int a, b;
        if (!column_range(keys, kHalf ? s + 1 : 0, n_gridded, kx + dx, ky + dy, kHalf && c == 0 ? kz : z0, z1, &a, &b)) continue;
        const int after = kHalf ? a : max(a, s + 1);
        if (b > after) cand += (unsigned long long)(b - after);
        // (full: the step over s is part of the increment -- no branch per candidate)
        for (int t = a + (!kHalf && a == s); t < b; t += 1 + (!kHalf && t + 1 == s)) visit(t);
    }
    return cand;
}

}}  // namespace nbody::cells
