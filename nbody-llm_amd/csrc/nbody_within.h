// nbody_within.h -- the fixed-radius neighbour lists behind include/nbody_hip.h ("neighbours within a radius"): internal entry
// points.
#pragma once
#include "nbody_handle.h"
#include "kernels_within.h"

namespace nbody { namespace within {

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal), confirmed enqueued steps and
// checked the radius and the kernel id.  n_upper >= the live count of sh (the host's view, which no call refreshes): the
// launches are sized from it and read the live count on the device.  Scratch is allocated and freed inside the call; nothing
// of the handle's is written but the record behind nbody_pair_search_stats.
template <class F>
int neighbors(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, uint64_t* offset, size_t cap, int32_t* neighbor,
              size_t neighbor_cap, size_t* n_out, uint64_t* n_neighbors_out);
template <class F>
int density(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, int kernel, double* rho, int32_t* count, size_t cap,
            size_t* n_out);
template <class F>
int density_center(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, int kernel, double center[3], double* rho_sum);

// The centre's four sums {sum rho, sum rho x, sum rho y, sum rho z} for rho [n_upper] on the device (already enqueued on the
// handle's stream): k_within_center's block sums, added on the host in ascending block order from +0.0.  Synchronises.
// nbody_knn_density_center (nbody_knn.cpp) ends with it too.
template <class F>
int center_sums(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* d_rho, double sum[kCenterSums]);

}}  // namespace nbody::within
