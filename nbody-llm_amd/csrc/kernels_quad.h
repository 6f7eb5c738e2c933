// kernels_quad.h -- launchers behind nbody_set_multipole(h, NBODY_MULTIPOLE_QUADRUPOLE) (internal to libnbody_hip.so):
// the cells' traceless quadrupole tensors in a side array beside the 32-byte node records, and the fast f32 walk that adds
// their term for every accepted internal node (kernels_quad.hip); and the walks of NBODY_POTENTIAL_TREE_QUADRUPOLE, which
// read the same side array.
#pragma once
#include "kernels.h"
#include "kernels_field.h"

namespace nbody {

// One record per node, 32 bytes, 32-byte aligned (one L1/L2 sector): {xx, xy, xz, yy}, {yz, zz, 0, 0} of
//     Q = sum_l m_l (3 d_l d_l^T - |d_l|^2 I),   d_l = c_l - c,
// over the leaves l of the node's subtree (the pre-order range (i, skip[i])), c = the node's stored centre of mass.
constexpr size_t kQuadRecBytes = 32;

// Fills quad[0 .. n) from the device-resident node array: differences, products and sums in f64, stored as f32; a leaf
// gets zeros.  info != nullptr: n = min(info[0], n_nodes) is read on the device (steps without read-back; n_nodes is
// then the capacity of both arrays); *poison != 0: nothing is written.
void launch_tree_quad(hipStream_t s, const float4* nodes, int n_nodes, float4* quad, const int* info, const int* poison);

// k_bh_walk<FAST, DIRECT> with the quadrupole term: one body per lane in tree order over the node-range split, the same
// opening tests, the same split planes and counter slots, then launch_bh_reduce.  Tuning::bh_walk_duo is ignored.
void launch_bh_walk_quad(hipStream_t s, const Shard& sh, const TreeDev& t, const float4* quad, float g, float g_soft2, float theta2,
                         unsigned long long* counters, int leaf_direct, const float* kick_dt, int* kicked);

// NBODY_POTENTIAL_TREE_QUADRUPOLE, nbody_potentials: launch_bh_pot_walk (kernels_pot.h) with the scalar quadrupole part
// 1/2 (d^T Q d) inv^5 of every accepted internal node, IEEE f32 arithmetic, f64 sums; then launch_pot_reduce.
void launch_bh_pot_walk_quad(hipStream_t s, const float4* own_pos, const TreeDev& t, const float4* quad, float g_soft2, float theta2,
                             double* planes, size_t plane_stride, double* sum, unsigned long long* counters);
// ... nbody_field_at: launch_bh_probe_walk (kernels_field.h) with the scalar and the vector part; the caller reduces
void launch_bh_field_walk_quad(hipStream_t s, const FieldTree& t, const float4* quad, const double* xyz, const int* idx, int n, float eps2,
                               float theta2, int want, double4* planes, size_t stride, unsigned long long* counters);

}  // namespace nbody
