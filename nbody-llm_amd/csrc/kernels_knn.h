// kernels_knn.h -- launchers of the exact k-nearest-neighbour lists (kernels_knn.hip): every body's k nearest bodies in the
// order (r2 ascending, then index ascending) as rows of k {index, r2}, the Casertano-Hut density from such a row, and the
// list of the rows the cell pass left unfinished.  The all-pairs pass runs on k_partner's frame (kernels_pairs.h); the pass
// over the cells of a grid is kernels_cells.h's launch_knn and fills the same arrays.  Internal to libnbody_hip.so.
#pragma once
#include "nbody_hip.h"
#include "kernels_pairs.h"   // PartnerPlan, kPairBlock
#include "shard.h"

namespace nbody { namespace knn {

using pairs::kPairBlock;
using pairs::PartnerPlan;

// The lists of a block stand in LDS as [slot][lane]: lane-contiguous 8-byte and 4-byte words, so a wave's access to one slot
// touches every bank once.  A kernel is compiled for 8 or for 32 slots (list_slots); k itself is a launch argument.
constexpr int kSlotsSmall = 8, kSlotsLarge = NBODY_KNN_MAX_K;
inline int list_slots(int k) { return k <= kSlotsSmall ? kSlotsSmall : kSlotsLarge; }
// the LDS of one block of the all-pairs pass: the lists and the partner tile
constexpr size_t lds_bytes(int slots) { return size_t(slots) * kPairBlock * (sizeof(double) + sizeof(int)) + kPairBlock * sizeof(double4); }
static_assert(lds_bytes(kSlotsLarge) <= 160 * 1024, "a block's lists and its partner tile fit a CU's LDS");

// The scratch of one call for n_upper rows and lists of k, carved out of one allocation of scratch_bytes (cells: with what the
// cell pass and the list of unfinished rows need) -- and the slice lists of an all-pairs pass, an allocation of their own of
// record_bytes, made once the pass's plan is known: for the second pass that is after the read-back of the rows it answers.
struct KnnScratch {
    int* neighbor = nullptr;    // [n_upper][k] the result: indices, -1 where a row holds fewer than k
    double* dist2 = nullptr;    // [n_upper][k] their r2, +inf where a row holds fewer
    double* rec_r2 = nullptr;   // [K][k][groups 256] the list of every (slice, row place), padded with +inf
    int* rec_j = nullptr;       // [K][k][groups 256] ... and -1
    int* found = nullptr;       // [n_upper] (cells) how many bodies with r2 < R2 the cell pass kept for the row, at most k
    int* flag = nullptr;        // [n_upper] 1: the row goes to the all-pairs pass
    int* offset = nullptr;      // [n_upper] exclusive prefix sums of flag
    int* list = nullptr;        // [n_upper] the flagged rows in ascending index
    int* total = nullptr;       // [1] how many
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
};
size_t scratch_bytes(size_t n_upper, int k, bool cells);
KnnScratch scratch_layout(void* base, size_t n_upper, int k, bool cells);
// rec_r2 and rec_j for a pass under the plan p: K k (groups 256) entries each
size_t record_bytes(const PartnerPlan& p, int k);
void record_layout(void* base, const PartnerPlan& p, int k, KnnScratch* w);

// k_knn_pairs<F> and k_knn_merge: w.neighbor / w.dist2 of `rows` rows against all live bodies.  list == nullptr: the rows are
// 0 .. rows - 1 (rows = n_upper; rows past the live count are left alone); else the rows are list[0 .. rows - 1].  p: the
// plan for that many rows (make_partner_plan(rows, n_upper)).
template <class F>
void launch_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, int k, const int* list, int rows, const PartnerPlan& p, const KnnScratch& w);

// After kernels_cells.h's launch_knn filled w.found: k_knn_flag, the integer scan and k_knn_compact -- w.list and *w.total, the
// live rows with found < k in ascending index.  live_count: the shard's own count, on the device.  Returns 0, or -1 when the
// scan could not be enqueued.
int launch_unfinished(hipStream_t s, const int* live_count, int n_upper, int k, const KnnScratch& w);

// k_knn_density<F>: rho and rk2 (either may be null) of the live rows from w.neighbor / w.dist2, one lane per body
template <class F>
void launch_density(hipStream_t s, const ShardT<F>& sh, int n_upper, int k, const KnnScratch& w, double* rho, double* rk2);

}}  // namespace nbody::knn
