// kernels_sample.h -- launchers of the grid sample (kernels_sample.hip): a grid read back at points with the deposit's stencil,
// values and central-difference gradients.  The arithmetic is sample_grid.h's.  Internal to libnbody_hip.so.
#pragma once
#include "sample_grid.h"
#include "shard.h"

namespace nbody { namespace sample {

constexpr int kSampleBlock = 256;

inline int blocks_for(size_t n) { return int((n + kSampleBlock - 1) / kSampleBlock); }

// how a call samples (the sample_sort and sample_pregrad knobs)
struct Plan {
    int sort = 1;      // 1: the points visited in home-cell order; 0: in row order
    int pregrad = 0;   // 1: k_grid_diff writes the three difference grids first and k_sample reads them as three fields
    int code() const { return sort | pregrad << 1; }
};
// from the knobs of the handle this thread serves; pregrad is 0 for NBODY_SAMPLE_VALUE and when 3 cells > NBODY_DEPOSIT_MAX_CELLS
Plan make_plan(int op, size_t cells);

// the words a call's kernels share, on the device
struct Words {
    unsigned long long counts[4];   // inside, partial, outside, skipped
    unsigned long long reads;       // grid reads k_sample issued
    unsigned long long reserved[3];
};

// The scratch of one call over at most n rows, carved out of one allocation of scratch_bytes.
struct Scratch {
    Words* words = nullptr;
    double* grid = nullptr;     // [fields][cells] the caller's grid
    double* diff = nullptr;     // [3][cells] the difference grids (pregrad)
    double* xyz = nullptr;      // [n][3] the points: the bodies' positions widened, or the caller's
    double* out = nullptr;      // [n][width]
    uint8_t* cls = nullptr;     // [n]
    uint32_t* keys = nullptr;   // [2 n] home cells, unsorted | sorted (rows past the live count and skipped points: `cells`, last)
    int* rows = nullptr;        // [2 n] the row index, unsorted | in key order
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
};
// own_grid == false (nbody_pm.cpp): no room for w.grid, which the caller points at a grid that is on the device already
size_t scratch_bytes(size_t n, size_t cells, int fields, int op, const Plan& p, bool own_grid = true);
Scratch scratch_layout(void* base, size_t n, size_t cells, int fields, int op, const Plan& p, bool own_grid = true);

// k_sample_stage<F>: w.xyz of every live row of sh
template <class F>
void launch_stage(hipStream_t s, const ShardT<F>& sh, int n_upper, const Scratch& w);

// k_grid_diff: w.diff from w.grid (one field)
void launch_diff(hipStream_t s, const Grid& g, int op, const Scratch& w);

// k_sample_keys and the stable radix sort of (home cell, row) over the n rows of w.xyz: w.rows + n is the rows in key order.
// Returns 0, or -1 when the rocPRIM call could not be enqueued.
int launch_order(hipStream_t s, const int* count, int n, const Grid& g, const Scratch& w);

// The n rows of w.xyz in home-cell order, for a gather: null when `sort` is off (row order); else w.rows + n, made first by
// launch_order unless `ordered` says that it holds the order of these rows already.  *rc: launch_order's, or 0; *sorts (may be
// null) += 1 when launch_order was enqueued.
const int* ordered_rows(hipStream_t s, const int* count, int n, const Grid& g, const Scratch& w, bool sort, bool ordered, int* rc,
                        uint64_t* sorts = nullptr);

// w.words zeroed; the rows from ordered_rows(p.sort, ordered); k_sample over the n rows of w.xyz, of which the first *count are
// live (count == nullptr: all n).  Returns 0, or -1 when the rocPRIM call could not be enqueued.
int launch_sample(hipStream_t s, const int* count, int n, const Grid& g, int fields, int op, const Plan& p, const Scratch& w,
                  bool ordered = false);

}}  // namespace nbody::sample
