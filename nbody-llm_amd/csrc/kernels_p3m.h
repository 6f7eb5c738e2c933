// kernels_p3m.h -- launchers of the P3M field's short-range part (kernels_p3m.hip): the bodies ordered by chain cell, the dense
// cell-start table and k_p3m_short, the periodic minimum-image pair sum.  The arithmetic is p3m_pairs.h's.  Internal to
// libnbody_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "p3m_pairs.h"
#include "shard.h"

namespace nbody { namespace p3m {

constexpr int kP3mBlock = 128;   // lanes of a block of k_p3m_short: the targets of a tile, and the partners staged at a time

// how a call sums (the p3m_lds knob)
struct Plan {
    int lds = 1;   // 1: the partner stream staged through LDS; 0: every lane reads its partners from global memory, the cross-check
    int code() const { return lds; }
};
Plan make_plan();   // from the knobs of the handle this thread serves

// the words a call's kernels share, on the device
struct Words {
    unsigned long long looked;    // partners looked at
    unsigned long long counted;   // terms with r2 < R2
    unsigned long long reserved[2];
};

// one set of rows ordered by chain cell
struct Order {
    double4* stage = nullptr;    // [n] {x, y, z, m} by row (a point: m = 0.0)
    double4* sorted = nullptr;   // [n] the same in chain order
    uint32_t* keys = nullptr;    // [2 n] chain cells, unsorted | sorted (no chain cell, and rows past the live count: `cells`, last)
    int* rows = nullptr;         // [2 n] the row index, unsorted | in key order
    int* start = nullptr;        // [cells + 2] start[c] = the first place of the order whose key is >= c
};

// The scratch of the short-range part over n_bodies body rows and n_rows target rows, carved out of scratch_bytes bytes.
// at_points == false: the targets are the bodies and `pts` stays empty.
struct Scratch {
    Entry* table = nullptr;   // [4097]
    Words* words = nullptr;
    Order bodies, pts;
    double4* out = nullptr;   // [n_rows] {acc_short, phi_short} by target row
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
};
size_t scratch_bytes(size_t n_bodies, size_t n_rows, size_t chain_cells, bool at_points);
Scratch scratch_layout(void* base, size_t n_bodies, size_t n_rows, size_t chain_cells, bool at_points);

// k_p3m_body_keys<F>, the stable radix sort of (chain cell, row), k_p3m_gather and k_p3m_starts: w.bodies of the n_upper rows of
// sh.  Returns 0, or -1 when the rocPRIM call could not be enqueued.
template <class F>
int launch_body_order(hipStream_t s, const ShardT<F>& sh, int n_upper, const deposit::Grid& g, const Chain& ch, const Scratch& w);

// the same for the n points xyz (on the device): w.pts
int launch_point_order(hipStream_t s, const double* xyz, int n, const deposit::Grid& g, const Chain& ch, const Scratch& w);

// w.out zeroed over n_rows rows; k_p3m_short<at_points, lds>, one block per chain cell: w.out of every target with a chain cell,
// and w.words added to.  n_bodies: the rows launch_body_order ordered; n_rows: the targets (at the bodies: n_bodies again)
void launch_short(hipStream_t s, int n_bodies, int n_rows, bool at_points, const Plan& plan, const Chain& ch, const Params& p, double g,
                  const Scratch& w);

// k_p3m_add: over the first live rows (count == nullptr: all n), acc[i][c] (and phi[i], where not null) = the mesh part plus
// w.out's, or under NBODY_P3M_SHORT_ONLY w.out's alone
void launch_add(hipStream_t s, const int* count, int n, int terms, const Scratch& w, double* acc, double* phi);

}}  // namespace nbody::p3m
