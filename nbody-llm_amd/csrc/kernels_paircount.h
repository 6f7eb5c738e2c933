// kernels_paircount.h -- launchers of the binned pair-separation counts (kernels_paircount.hip): how many pairs of bodies, or
// of bodies and caller points, stand at each separation.  The all-pairs pass runs on k_partner's frame (kernels_pairs.h); the
// pass over the cells of a grid is kernels_cells.h's launch_pair_hist and fills the same array.  The bin rule and the
// block-private LDS histogram are stated once, below, for all of them.  Internal to libnbody_hip.so.
//
// THE OVERFLOW BOUND of the LDS histogram.  A block keeps one 32-bit word per slot and adds its words to the call's 64-bit
// array with integer atomics.  In the all-pairs pass a lane adds at most one count per partner, a tile holds 256 partners and
// a block 256 lanes: T tiles put at most 256 * 256 * T = 65 536 T counts into one word.  The block therefore hands its words
// over after every T <= kFlushTilesMax = 65 535 tiles (65 536 * 65 535 = 2^32 - 65 536 < 2^32) and once more at its end; a
// slice of fewer than 16 776 960 partners -- every launch the default plan makes below 2^24 bodies -- flushes once.  In the
// pass over a grid a lane's candidates are not bounded by a tile, so a lane counts its own additions: the first 256 T go to
// LDS (256 lanes * 256 T: the same bound), any further one straight to the 64-bit array.  T is the pair_hist_flush knob
// (0: kFlushTilesMax); integer additions commute, so T, K and the launch shape cannot show in the result.
#pragma once
#include "nbody_hip.h"
#include "kernels_pairs.h"   // PartnerPlan, kPairBlock
#include "shard.h"

namespace nbody { namespace paircount {

using pairs::kPairBlock;
using pairs::PartnerPlan;

constexpr int kMaxBins = NBODY_PAIR_COUNT_MAX_BINS;
constexpr int kSlots = kMaxBins + 2;      // slot 0: below E2[0] | slot b + 1: bin b | slot n_bins + 1: everything else
constexpr int kFlushTilesMax = 65535;

// how a launch counts: tiles between two flushes of the LDS words, and how the lanes of a wave that hit the same slot at the
// same partner are combined before the LDS atomic (the pair_hist_combine knob)
enum { kCombineNone = 0,     // every lane adds its own 1
       kCombineFirst = 1,    // the lanes that share the first counting lane's slot add their number once; the others add their own 1
       kCombineAll = 2 };    // every distinct slot of the wave adds its number once
struct HistPlan { int flush_tiles = kFlushTilesMax, combine = kCombineNone; };
HistPlan make_hist_plan();   // from the knobs of the handle this thread serves

// the steps of the bin search: the highest power of two <= n_bins - 1 (0 for one bin) -- ceil(log2(n_bins)) steps, 10 for 1 024
inline int search_top(int n_bins) {
    int top = 0;
    for (int p = 1; p <= n_bins - 1; p <<= 1) top = p;
    return top;
}

// The scratch of one call, carved out of one allocation of scratch_bytes.
struct HistScratch {
    double* e2 = nullptr;                 // [n_bins + 1] the squared edges
    unsigned long long* hist = nullptr;   // [n_bins + 2] the slots, 64 bits each
    double* points = nullptr;             // [batch][3] (pair_counts_at) the caller's points of one batch
};
size_t scratch_bytes(int n_bins, size_t batch);
HistScratch scratch_layout(void* base, int n_bins, size_t batch);

// k_pair_hist<F, false>: every pair i < j of the live bodies into w.hist (added to what it holds)
template <class F>
void launch_auto(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, const HistPlan& hp, int n_bins, const HistScratch& w);
// k_pair_hist<F, true>: every (live body, point of w.points[0 .. m)) pair into w.hist; p: rows = bodies, partners = points
template <class F>
void launch_cross(hipStream_t s, const ShardT<F>& sh, int n_upper, int m, const PartnerPlan& p, const HistPlan& hp, int n_bins,
                  const HistScratch& w);

#if defined(__HIPCC__)
// ---- what every counting pass shares on the device (k_pair_hist; k_cells_pair_hist of kernels_cells.hip)
// THE BIN RULE.  e2[0 .. n_bins] strictly ascending and finite.  The slot of r2: 0 iff r2 < e2[0]; b + 1 iff
// e2[b] <= r2 && r2 < e2[b + 1] (closed below, open above); n_bins + 1 for everything else, i.e. !(r2 < e2[n_bins]) -- a NaN
// fails every comparison, matches no bin and lands there with +inf.  The bin is a branch-free binary search: b only ever moves
// to an edge that is <= r2, in ceil(log2(n_bins)) steps from `top` = search_top(n_bins) down.
__device__ __forceinline__ int bin_slot(const double* e2, int n_bins, int top, double r2) {
    int b = 0;
    for (int step = top; step > 0; step >>= 1) {
        const int c = b + step;
        const double edge = e2[c < n_bins ? c : n_bins];   // (no read past the edges; c >= n_bins is never taken)
        b = (c < n_bins && edge <= r2) ? c : b;
    }
    return r2 < e2[0] ? 0 : (r2 < e2[n_bins] ? b + 1 : n_bins + 1);
}

// the block's LDS copy of the edges and its zeroed words; the caller synchronises the block before it uses either
__device__ __forceinline__ void hist_begin(const double* __restrict__ e2_global, int n_bins, double* e2, unsigned* hist) {
    for (int k = threadIdx.x; k <= n_bins; k += kPairBlock) e2[k] = e2_global[k];
    for (int k = threadIdx.x; k < n_bins + 2; k += kPairBlock) hist[k] = 0u;
}

// the block's words added to the call's 64-bit slots (vector integer atomics) and zeroed again; every thread of the block calls it
__device__ __forceinline__ void hist_flush(unsigned* hist, int n_bins, unsigned long long* out) {
    __syncthreads();
    for (int k = threadIdx.x; k < n_bins + 2; k += kPairBlock) {
        const unsigned v = hist[k];
        if (v) atomicAdd(out + k, (unsigned long long)v);
        hist[k] = 0u;
    }
    __syncthreads();
}

// one count into hist[slot] (slot < 0: this lane counts nothing).  Every lane of the wave calls it together.
template <int kCombine>
__device__ __forceinline__ void hist_add(unsigned* hist, int slot) {
    if constexpr (kCombine == kCombineNone) {
        if (slot >= 0) atomicAdd(hist + slot, 1u);
    } else {
        unsigned long long todo = __ballot(slot >= 0);
        const int lane = int(threadIdx.x) % 64;
        while (todo) {   // (wave-uniform)
            const int lead = __builtin_ctzll(todo);
            const int s0 = __shfl(slot, lead, 64);
            const unsigned long long same = __ballot(slot == s0);
            if (lane == lead) atomicAdd(hist + s0, unsigned(__popcll(same)));
            todo &= ~same;
            if constexpr (kCombine == kCombineFirst) {
                if ((todo >> lane) & 1ull) atomicAdd(hist + slot, 1u);
                break;
            }
        }
    }
}
#endif

}}  // namespace nbody::paircount
