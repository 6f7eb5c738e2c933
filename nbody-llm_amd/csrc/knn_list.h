// knn_list.h -- the per-lane sorted lists of the k-nearest-neighbour kernels (kernels_knn.hip, kernels_cells.hip k_cells_knn):
// device code.  A block of 256 lanes keeps 256 lists of at most k {r2, index} entries in LDS as [slot][lane]; a list is
// ascending in (r2, index).  Nothing here adds or multiplies: the lists hold bits that the callers computed.
#pragma once
#include <hip/hip_runtime.h>
#include "device_util.h"     // inf64
#include "kernels_pairs.h"   // kPairBlock

namespace nbody { namespace knn {

// [slot][lane]: the lanes of a wave read and write one slot at consecutive addresses (8-byte words over all 64 banks, 4-byte
// words over 32), so an access that the whole wave makes is conflict-free; a lane alone touches one bank per word
template <int kSlots>
struct ListLds {
    double r2[kSlots][pairs::kPairBlock];
    int j[kSlots][pairs::kPairBlock];
};

// One lane's list and what admits a candidate to it: `held` entries (<= k), and the last entry of a full list -- {+inf, INT_MAX}
// while it is not full, so every r2 < +inf comes before it
struct ListState {
    int held = 0;
    double last_r2 = inf64();
    int last_j = 0x7fffffff;
    // (r2, j) comes before the last entry of a full list, or the list is not full and r2 < +inf; a NaN never does
    __device__ __forceinline__ bool admits(double r2, int j) const { return r2 < last_r2 || (r2 == last_r2 && j < last_j); }
};

// Puts (r2, j) at its place in lane `lane`'s list; st.admits(r2, j) held.  The entries after it move one slot down and the last
// one of a full list is dropped.  Slow and divergent by design: after the first tiles almost no candidate gets here.
template <int kSlots>
__device__ __forceinline__ void list_insert(ListLds<kSlots>& l, int lane, int k, ListState& st, double r2, int j) {
    int p = st.held < k ? st.held : k - 1;   // (0 <= p <= k - 1 < kSlots)
    while (p > 0) {
        const double pr = l.r2[p - 1][lane];
        const int pj = l.j[p - 1][lane];
        if (!(pr > r2 || (pr == r2 && pj > j))) break;
        l.r2[p][lane] = pr;
        l.j[p][lane] = pj;
        --p;
    }
    l.r2[p][lane] = r2;
    l.j[p][lane] = j;
    if (st.held < k) ++st.held;
    if (st.held == k) {
        st.last_r2 = l.r2[k - 1][lane];
        st.last_j = l.j[k - 1][lane];
    }
}

}}  // namespace nbody::knn
