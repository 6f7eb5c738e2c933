// kernels_field.h -- launchers behind nbody_field_at (internal to libnbody_hip.so): acceleration and potential of all bodies
// at caller-chosen points.  Probes arrive as f64 triples and are rounded once to the handle's precision; every kernel leaves
// {sum m d / s^3, sum m / s} (d = x_j - x, s = sqrt(|d|^2 + eps2)) per (segment or slice, probe) in planes of double4, each
// entry written once; k_field_reduce adds them in plane order, multiplies by +g / -g and scatters to the caller's order.
#pragma once
#include "kernels_pot.h"

namespace nbody {

// the tree a field call walks: the force pass's nodes and split points (FieldBufs)
struct FieldTree {
    const void* nodes = nullptr;   // NodeDev (f32 handles) or Node64 (f64)
    int K = 1;
    const int* first = nullptr;
    const int* anc = nullptr;
    const int* n_anc = nullptr;
};

// Morton keys of n probes in the handle's box (the device build's key layout; outside the box the orthant descent saturates,
// NaN compares false), then {key, place in the batch} sorted by key: idx [n] = the batch's probes in tree order
size_t field_sort_tmp_bytes(size_t n_cap);
int field_sort_probes(hipStream_t s, const double* xyz, int n, int f64, const double center[3], double width, void* tmp, size_t tmp_bytes,
                      unsigned long long* keys /* [2][n_cap] */, int* idx /* [2][n_cap] */, size_t n_cap, const int** sorted_idx);

// NBODY_POTENTIAL_TREE: one probe per lane in idx order over the node-range split, the potential walk's tests (DIRECT rule);
// terms in the handle's precision, four f64 sums.  want: bit 0 the vector part, bit 1 the scalar part (0: count only)
void launch_bh_field_walk(hipStream_t s, const FieldTree& t, const double* xyz, const int* idx, int n, float eps2, float theta2, int want,
                          double4* planes, size_t stride, unsigned long long* counters);
}  // namespace nbody
namespace nbody64 {
void launch_bh_field_walk(hipStream_t s, const nbody::FieldTree& t, const double* xyz, const int* idx, int n, double eps2, double theta2, int want,
                          double4* planes, size_t stride, unsigned long long* counters);
}
namespace nbody {

// NBODY_POTENTIAL_PAIRS: every live body of every segment, one-sided, in f64; K slices of the concatenated body list
void launch_field_pairs(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double4* planes, size_t stride);
// slices for a batch of n probes against n_bodies bodies, so that a few thousand probes still fill the chip
int field_pairs_slices(size_t n, size_t n_bodies);

// planes added in plane order; acc [n][3] = +g sum, phi [n] = -g sum, at place idx[t] (idx == nullptr: t); either may be null
void launch_field_reduce(hipStream_t s, const double4* planes, int K, size_t stride, const int* idx, int n, double g, double* acc, double* phi);

}  // namespace nbody
