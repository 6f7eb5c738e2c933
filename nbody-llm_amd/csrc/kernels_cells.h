// kernels_cells.h -- launchers of the cell-list pair search (kernels_cells.hip): the bodies of a handle sorted by the cell of a
// uniform grid (cell_grid.h), and over that order the two fixed-radius passes -- the links of the friends-of-friends group
// finder and every body's nearest body within a radius.  They fill the arrays the all-pairs passes fill (kernels_fof.h
// FofScratch::parent, kernels_pairs.h PairScratch::partner / energy), so everything after them runs unchanged.  Internal to
// libnbody_hip.so.
#pragma once
#include "cell_grid.h"
#include "kernels_fof.h"
#include "kernels_pairs.h"
#include "shard.h"

namespace nbody { namespace cells {

// the integer-mapped bounds of the gridded bodies and their number, as k_cells_bounds leaves them
struct BoundsWords {
    unsigned long long lo[3], hi[3];   // ordered_of(min), ordered_of(max)
    unsigned long long gridded;
    unsigned long long reserved;
};
// (what the device wrote, on the host) the bounds as doubles; returns the gridded bodies
size_t bounds_of(const BoundsWords& w, double lo[3], double hi[3]);

// the integer counts of one search, formed on the device
struct Counters {
    unsigned long long occupied;     // distinct keys
    unsigned long long candidates;   // unordered pairs of gridded bodies whose cell indices differ by at most 1 on every axis
};

// The scratch of one search over n_upper rows, carved out of one allocation of scratch_bytes.  (The BoundsWords are an
// allocation of their own: the caller needs them before it knows whether there will be a search.)
struct CellScratch {
    Counters* counters = nullptr;
    uint64_t* keys = nullptr;    // [2 n_upper] unsorted | sorted (rows past the live count and ungridded bodies: all ones, last)
    int* rows = nullptr;         // [2 n_upper] the row index, unsorted | in key order (stable: ascending row within a cell)
    double4* spos = nullptr;     // [n_upper] the gridded bodies' positions in key order ({x, y, z, mass})
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
    const uint64_t* sorted_keys(size_t n_upper) const { return keys + n_upper; }
    const int* sorted_rows(size_t n_upper) const { return rows + n_upper; }
};
size_t scratch_bytes(size_t n_upper);
CellScratch scratch_layout(void* base, size_t n_upper);

// k_cells_bounds<F>: *bounds (on the device) of the live, gridded bodies of sh, zeroed and filled; the caller copies it to the host
template <class F>
void launch_bounds(hipStream_t s, const ShardT<F>& sh, int n_upper, BoundsWords* bounds);

// k_cells_keys<F>, the stable radix sort of (key, row), k_cells_gather<F>: the sorted keys and rows, w.spos, and
// w.counters->occupied; w.counters->candidates is zeroed.  n_gridded: what launch_bounds counted.  Returns 0, or -1 when the
// rocPRIM call could not be enqueued.
template <class F>
int launch_order(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_gridded, const Grid& g, const CellScratch& w);

// k_cells_link between k_fof_init and k_fof_flatten (kernels_fof.h): f.label and f.size of the live rows for the links
// r2 < B2, as launch_components leaves them; w.counters->candidates.  live_count: the shard's own count, on the device.
void launch_link_components(hipStream_t s, const int* live_count, int n_upper, int n_gridded, double B2, const CellScratch& w,
                            const fof::FofScratch& f);

// k_cells_nearest: p.partner / p.energy of every row = the body of least r2 < R2 (among equal r2 the lowest index) and that r2,
// or -1 and +inf -- what launch_nearest leaves wherever launch_contacts looks; w.counters->candidates
void launch_nearest_within(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, const pairs::PairScratch& p);

// k_cells_within<false>: found[i] of every gridded row = the bodies j != i with r2 < R2 (the other rows are left as they are:
// the caller zeroed them), their number added to *total in 64 bits; w.counters->candidates
void launch_within_count(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, int* found, unsigned long long* total);
// k_cells_within<true>: those bodies' indices at raw[offset[i]] on, in the order of the walk over the cells (not ascending);
// cap: the words of raw
void launch_within_fill(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, const int* offset, int* raw, size_t cap);

// k_cells_knn: row i's k {index, r2} at neighbor[i k] / dist2[i k] on, for every gridded row -- the at most k bodies j != i with
// r2 < R2 that come first in (r2, j), padded with {-1, +inf} --, and found[i] = how many (zeroed here for every row first);
// the other rows' lists are left alone; 1 <= k <= NBODY_KNN_MAX_K; w.counters->candidates as launch_nearest_within counts them
void launch_knn(hipStream_t s, int n_upper, int n_gridded, int k, double R2, const CellScratch& w, int* found, int* neighbor, double* dist2);

// k_cells_pair_hist: every candidate pair with r2 < e2[n_bins] added to hist[slot of its r2] (kernels_paircount.h: slot 0 below
// e2[0], slot b + 1 bin b; hist[n_bins + 1] is left alone: the caller subtracts); e2 [n_bins + 1] and hist [n_bins + 2] on the
// device; flush_tiles: HistPlan's; w.counters->candidates as launch_link_components counts them
void launch_pair_hist(hipStream_t s, int n_upper, int n_gridded, const CellScratch& w, const double* e2, int n_bins, int flush_tiles,
                      unsigned long long* hist);

}}  // namespace nbody::cells
