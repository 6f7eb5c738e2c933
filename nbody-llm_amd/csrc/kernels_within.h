// kernels_within.h -- launchers of the fixed-radius neighbour lists (kernels_within.hip): every body's neighbours within a
// radius as a CSR list in ascending index, the density estimates that walk that list, and the block sums of the density
// centre.  The all-pairs passes run on k_partner's frame (kernels_pairs.h); the passes over the cells of a grid are
// kernels_cells.h's launch_within_*, and fill the same arrays.  Internal to libnbody_hip.so.
#pragma once
#include "nbody_hip.h"
#include "kernels_pairs.h"   // PartnerPlan, kPairBlock
#include "shard.h"

namespace nbody { namespace within {

using pairs::kPairBlock;
using pairs::PartnerPlan;

constexpr int kCenterSums = 4;   // sum rho, sum rho x, sum rho y, sum rho z

// What a call allocates before it knows how many neighbours there are, for n_upper rows and K partner slices (the passes over
// a grid: K = 1), carved out of one allocation of count_scratch_bytes.
struct CountScratch {
    unsigned long long* total = nullptr;   // [1] directed neighbours, summed in 64 bits (an integer: the order cannot show)
    int* count = nullptr;                  // [n_upper K + 1] neighbours of (body, slice), body-major; the last word stays 0
    int* place = nullptr;                  // [n_upper K + 1] exclusive prefix sums of count: where each slice's run begins
    int* offset = nullptr;                 // [n_upper + 1] place[i K]: where body i's list begins; K == 1: `place` itself
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    size_t words = 0;                      // n_upper K + 1
};
size_t count_scratch_bytes(size_t n_upper, int K);
CountScratch count_scratch_layout(void* base, size_t n_upper, int K);

// What it allocates once the total is known (0 < total <= 2^31 - 1): the lists, and for the passes over a grid the unsorted
// lists and rocPRIM's temporary storage beside them.
struct ListScratch {
    int* neighbor = nullptr;   // [total] the lists in ascending index, body after body
    int* raw = nullptr;        // [total] (grid) the lists in the order the cells were walked
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
};
size_t list_scratch_bytes(size_t n_upper, size_t total, bool sorted);
ListScratch list_scratch_layout(void* base, size_t n_upper, size_t total, bool sorted);

// zeroes c.total and c.count (all words)
void launch_clear(hipStream_t s, const CountScratch& c);

// k_within_pairs<F, false>: c.count of every (body, slice) and *c.total, over all pairs (rows past the live count: 0)
template <class F>
void launch_count_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double R2, const CountScratch& c);

// the integer scan of c.count into c.place, and c.offset from it.  Returns 0, or -1 when the scan could not be enqueued.
int launch_places(hipStream_t s, int n_upper, int K, const CountScratch& c);

// k_within_pairs<F, true>: l.neighbor, every slice's run written in ascending j at c.place -- the lists are ascending as written
template <class F>
void launch_fill_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double R2, const CountScratch& c,
                       const ListScratch& l, size_t total);

// rocPRIM's segmented radix sort of l.raw into l.neighbor over the segments c.offset[i] .. c.offset[i + 1] (the keys of a
// segment are distinct integers: one result).  Returns 0, or -1 when it could not be enqueued.
int launch_sort_lists(hipStream_t s, int n_upper, const CountScratch& c, const ListScratch& l, size_t total);

// k_within_density<F>: rho and count of the live rows (either may be null) from the lists -- one lane per body, its terms in
// ascending index with its own term among them, summed sequentially from +0.0.  spline: the M4 kernel, else the top hat;
// hs = radius * 0.5 and norm as the header writes them, formed by the caller.
template <class F>
void launch_density(hipStream_t s, const ShardT<F>& sh, int n_upper, bool spline, double hs, double norm, const int* offset,
                    const int* neighbor, double* rho, int* count);

// k_within_center<F>: part[block][kCenterSums] -- per block of 256 rows the pairwise tree of rho and rho x_c (rows past the
// live count add +0.0), as k_diag_moments forms its sums
template <class F>
void launch_center(hipStream_t s, const ShardT<F>& sh, int n_upper, const double* rho, double* part);

}}  // namespace nbody::within
