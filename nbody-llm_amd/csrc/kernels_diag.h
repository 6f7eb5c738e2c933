// kernels_diag.h -- launchers of the whole-state diagnostics (kernels_diag.hip): the ten moment sums and the Lagrangian radii;
// internal to libnbody_hip.so.
#pragma once
#include "shard.h"

namespace nbody { namespace diag {

constexpr int kDiagBlock = 256;
constexpr int kMoments = 10;   // {M, X[3], P[3], L[3]}

inline int blocks_for(int n) { return n <= 0 ? 0 : (n + kDiagBlock - 1) / kDiagBlock; }

// per block of kDiagBlock bodies the ten sums {m, m x, m v, m (x cross v)} of the n_upper >= live bodies, each added pairwise
// in a fixed tree (part[blocks_for(n_upper)][kMoments]; rows past the live count add +0.0)
template <class F>
void launch_diag_moments(hipStream_t s, const ShardT<F>& sh, int n_upper, double* part);

// The scratch of one nbody_lagrangian_radii call for n_upper rows, carved out of one allocation of radii_scratch_bytes.
struct RadiiScratch {
    unsigned long long* keys = nullptr;   // [2][n_upper] bit patterns of r2, unsorted | sorted; all ones = left out
    int* idx = nullptr;                   // [2][n_upper] body index, unsorted | sorted
    double* c = nullptr;                  // [n_upper] masses in sorted order, then their inclusive prefix sums
    double* totals = nullptr;             // [2][tiles] double-double totals of the scan's tiles, hi | lo
    int* n_valid = nullptr;               // [1] bodies in the order
    double* center = nullptr;             // [3]
    double* fractions = nullptr;          // [n_frac]
    double* out = nullptr;                // [n_frac] radii | [1] mass
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
};
size_t radii_scratch_bytes(size_t n_upper, size_t n_frac);
RadiiScratch radii_scratch_layout(void* base, size_t n_upper, size_t n_frac);

// keys, sort, gather, scan, one lane per fraction: out[k] = sqrt(r2) of the first body whose prefix reaches fractions[k] *
// mass, out[n_frac] = mass (the last prefix).  center and fractions are already on the device.  Returns 0, or -1 when the
// sort could not be enqueued.
template <class F>
int launch_diag_radii(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_frac, const RadiiScratch& w);

}}  // namespace nbody::diag
