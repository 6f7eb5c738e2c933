// kernels_deposit.h -- launchers of the grid deposit (kernels_deposit.hip): the bodies of a handle assigned to a regular grid
// in 64-bit fixed point.  The arithmetic is deposit_grid.h's.  Internal to libnbody_hip.so.
#pragma once
#include "deposit_grid.h"
#include "shard.h"

namespace nbody { namespace deposit {

constexpr int kDepositBlock = 256;
constexpr int kTileSlots = 1024;   // int64 slots of a block's LDS table (deposit_lds): 8 KiB of sums and 4 KiB of tags

inline int blocks_for(int n) { return n <= 0 ? 0 : (n + kDepositBlock - 1) / kDepositBlock; }

// how a call deposits (the deposit_sort, deposit_combine and deposit_lds knobs)
struct Plan {
    int sort = 1;      // 1: the rows ordered by home cell first; 0: in row order
    int combine = 1;   // 1: a wave's runs of equal cells are summed by a segmented scan and their last lane adds; 0: every lane adds its own term
    int lds = 1;       // 1: additions go to the block's tagged LDS table first, which is flushed at the block's end
    int code() const { return sort | combine << 1 | lds << 2; }
};
Plan make_plan();   // from the knobs of the handle this thread serves

// the words a call's kernels share, on the device
struct Words {
    unsigned long long qmax_bits;    // the bits of the largest |q| among the bodies that are not skipped (they order as the doubles)
    unsigned long long counts[4];    // inside, partial, outside, skipped
    unsigned long long terms;        // terms that landed on the grid
    unsigned long long atomics;      // 64-bit atomics sent to global memory
    unsigned long long reserved;
};

// The scratch of one call over n_upper rows and `cells` cells, carved out of one allocation of scratch_bytes.  with_grid ==
// false (counts only): words and q alone.
struct Scratch {
    Words* words = nullptr;
    double* q = nullptr;           // [n_upper]
    long long* acc = nullptr;      // [cells] the fixed-point sums, then the doubles in place
    uint32_t* keys = nullptr;      // [2 n_upper] home cells, unsorted | sorted (rows past the live count and skipped bodies: `cells`, last)
    int* rows = nullptr;           // [2 n_upper] the row index, unsorted | in key order
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
};
size_t scratch_bytes(size_t n_upper, size_t cells, bool with_grid, bool sorted);
Scratch scratch_layout(void* base, size_t n_upper, size_t cells, bool with_grid, bool sorted);

// k_deposit_q<F>: w.words zeroed and filled (but terms and atomics), w.q of every live row
template <class F>
void launch_q(hipStream_t s, const ShardT<F>& sh, int n_upper, const Grid& g, int quantity, const Scratch& w);

// w.acc zeroed; p.sort: k_deposit_keys<F> and the stable radix sort of (home cell, row); k_deposit<F>; k_deposit_convert.
// Returns 0, or -1 when the rocPRIM call could not be enqueued.  ordered_rows (nbody_pm.cpp): the n_upper rows in home-cell order,
// made already -- no keys and no sort here, whatever p.sort says, and w.keys, w.rows and w.sort_tmp are not touched.
template <class F>
int launch_deposit(hipStream_t s, const ShardT<F>& sh, int n_upper, const Grid& g, const Plan& p, const Scratch& w,
                   const int* ordered_rows = nullptr);

}}  // namespace nbody::deposit
