// pair_tiles.h -- the frame of the all-pairs query kernels (k_partner, k_within_pairs, k_fof_link, k_pair_hist; k_knn_pairs
// has the same loop written out, for its speed): device code.  The grid is (groups of kPairBlock rows) x K partner slices (kernels_pairs.h PartnerPlan); a block holds one row
// per lane and streams the partners of its slice through LDS in tiles of kPairBlock, j ascending.
//
// The live count is live_count's max(0, min(*count, n_upper)) in every kernel.  *count is never negative in a valid handle, so
// for k_partner, which used to take min(*count, n_upper) alone, nothing changes: the two agree on every state it can see.
#pragma once
#include <hip/hip_runtime.h>
#include "device_util.h"     // live_count
#include "kernels_pairs.h"   // kPairBlock

namespace nbody { namespace pairs {

// what a block derives from blockIdx.x: its rows are first .. first + kPairBlock - 1, its partners [lo, hi) -- slice `slice` of
// `partners` partners, [partners slice / K, partners (slice + 1) / K)
struct PairFrame {
    int group, slice, first, lo, hi;
    __device__ __forceinline__ PairFrame(int groups, int K, int partners)
        : group(int(blockIdx.x) % groups), slice(int(blockIdx.x) / groups), first(group * kPairBlock),
          lo(int((long long)partners * slice / K)), hi(int((long long)partners * (slice + 1) / K)) {}
    // For a symmetric metric over the rows themselves only j > i is looked at.  false: no partner of the slice lies above the
    // block's lowest row, the block has nothing to do (block-uniform: return before the first barrier).  Else the tiles below
    // its first row are skipped, not masked.
    __device__ __forceinline__ bool triangle() {
        if (hi - 1 <= first) return false;
        lo = max(lo, first);
        return true;
    }
};

// The tile loop.  For every tile of partners t0 .. t0 + cnt - 1: lane tid < cnt stages partner t0 + tid with load(tid, j),
// which writes slot tid of the kernel's LDS tiles; then every lane calls visit(j, t) for j = t0 + t, t = 0 .. cnt - 1 -- slot
// t is the same address for the whole wave, so reading it is an LDS broadcast --; then after_tile().  EVERY LANE OF THE BLOCK
// MUST GET HERE: the two barriers of a tile are the loop's own, and lo and hi are block-uniform.
template <class Load, class Visit, class AfterTile>
__device__ __forceinline__ void for_each_partner(const PairFrame& f, Load&& load, Visit&& visit, AfterTile&& after_tile) {
    const int tid = threadIdx.x;
    for (int t0 = f.lo; t0 < f.hi; t0 += kPairBlock) {
        const int cnt = min(kPairBlock, f.hi - t0);
        __syncthreads();
        if (tid < cnt) load(tid, t0 + tid);   // (t0 + tid < hi <= the partners)
        __syncthreads();
        for (int t = 0; t < cnt; ++t) visit(t0 + t, t);
        after_tile();
    }
}
template <class Load, class Visit>
__device__ __forceinline__ void for_each_partner(const PairFrame& f, Load&& load, Visit&& visit) {
    for_each_partner(f, load, visit, [] {});
}

}}  // namespace nbody::pairs
