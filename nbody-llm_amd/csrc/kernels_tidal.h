// kernels_tidal.h -- launchers behind nbody_tidal_at (internal to libnbody_hip.so): the tidal tensor of all bodies at
// caller-chosen points, T_ab = sum m (3 d_a d_b / q^(5/2) - delta_ab / q^(3/2)), d = x_j - x, q = |d|^2 + eps2.  The probes, the
// batches, the Morton sort, the tree's view and the slices are nbody_field_at's (kernels_field.h); every kernel here leaves
// the six sums {xx, xy, xz, yy, yz, zz} per (segment or slice, probe) in planes of rows of three double2, each row written
// once; k_tidal_reduce adds them in plane order, multiplies by g and scatters to the caller's order.  One term, every line
// one rounding (f64 for PAIRS, the handle's precision for TREE; IEEE sqrt and divide, nothing contracted):
//     inv = 1 / sqrt(q)   st = m inv   k = st / q   k3 = (3 k) / q   u_c = d_c k3
//     xx += dx u_x - k    yy += dy u_y - k    zz += dz u_z - k    xy += dx u_y    xz += dx u_z    yz += dy u_z
// (the two divides by q, not products with inv, keep a component within 24 u of the term's scale: tests/tidal_list.py counts).
#pragma once
#include "kernels_field.h"

namespace nbody {

constexpr int kTidalRow = 3;   // double2 per plane row: {xx, xy} {xz, yy} {yz, zz}

// NBODY_POTENTIAL_TREE: the field walk's traversal, entry, tests and counters (launch_bh_field_walk), six f64 sums of terms in
// the handle's precision.  sums == 0: count only (planes are not written)
void launch_bh_tidal_walk(hipStream_t s, const FieldTree& t, const double* xyz, const int* idx, int n, float eps2, float theta2, int sums,
                          double2* planes, size_t stride, unsigned long long* counters);
}  // namespace nbody
namespace nbody64 {
void launch_bh_tidal_walk(hipStream_t s, const nbody::FieldTree& t, const double* xyz, const int* idx, int n, double eps2, double theta2, int sums,
                          double2* planes, size_t stride, unsigned long long* counters);
}
namespace nbody {

// NBODY_POTENTIAL_PAIRS: launch_field_pairs' shape (one wave per (probe group, slice of the concatenated body list)), in f64
void launch_tidal_pairs(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double2* planes, size_t stride);
// slices for a batch of n probes against n_bodies bodies (field_pairs_slices with this kernel's probes per lane)
int tidal_pairs_slices(size_t n, size_t n_bodies);

// planes added in plane order; out [n][6] = g sum, at row idx[t] (idx == nullptr: t)
void launch_tidal_reduce(hipStream_t s, const double2* planes, int K, size_t stride, const int* idx, int n, double g, double* out);

}  // namespace nbody
