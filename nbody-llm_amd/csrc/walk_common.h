// walk_common.h -- the two fragments every split tree walk of kernels_bh.hip, kernels_f64.hip and kernels_quad.hip starts
// and ends with.  Device code only.
#pragma once
#include "kernels.h"   // NBODY_WALK_COUNTER_SLOTS

namespace nbody {

// Which of the K node-range segments workgroup (bx of gx, blockIdx.y = kk) walks.  The launch lasts as long as its slowest
// wave, and a body group's long walks are in the segments around its own place in the tree (that is where cells are opened
// down to the leaves).  Bodies are in tree order, so group bx of gx sits near node bx/gx * n_nodes: the segments are taken
// by distance from that "diagonal" -- kk = 0 is the group's own segment, then +1, -1, +2, ... -- and the dispatcher, which
// hands out workgroups in blockIdx order (x fastest), starts the heavy ones first.
// (Index: unsigned for blockIdx.x itself, int for a remapped one -- the 64-bit product is formed from it as it comes.)
template <class Index>
__device__ __forceinline__ int nearest_first_segment(Index bx, unsigned gx, int kk, int K) {
    const int diag = int((long long)bx * K / gx);
    const int off = (kk & 1) ? (kk + 1) / 2 : -(kk / 2);
    return ((diag + off) % K + K) % K;
}

// The lanes' {accepted, visited} counts added up over the wave and into pair `slot` (taken modulo the slot count) of
// `counters` (may be null): one atomic pair per wave, spread over NBODY_WALK_COUNTER_SLOTS address pairs -- 16 384 atomics
// on ONE address pair serialise in L2 at ~13 ns each (0.21 ms per walk at 8 segments, measured with theta2 = 1e9).
// Called by every lane of the wave, outside divergent code.
__device__ __forceinline__ void add_walk_counts(unsigned long long* __restrict__ counters, unsigned slot, unsigned int n_acc,
                                                unsigned int n_vis) {
    for (int off = 32; off > 0; off >>= 1) {
        n_acc += __shfl_down(n_acc, off);
        n_vis += __shfl_down(n_vis, off);
    }
    if ((threadIdx.x & 63) == 0 && counters) {
        slot &= NBODY_WALK_COUNTER_SLOTS - 1;
        atomicAdd(&counters[2 * slot], (unsigned long long)n_acc);
        atomicAdd(&counters[2 * slot + 1], (unsigned long long)n_vis);
    }
}

}  // namespace nbody
