// nbody_knn.h -- the exact k-nearest-neighbour lists behind include/nbody_hip.h ("k nearest neighbours"): internal entry
// points.
#pragma once
#include "nbody_handle.h"
#include "kernels_knn.h"

namespace nbody { namespace knn {

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal), confirmed enqueued steps and
// checked k and the hint (0, or finite and > 0).  n_upper >= the live count of sh (the host's view, which no call refreshes): the
// launches are sized from it and read the live count on the device.  Scratch is allocated and freed inside the call; nothing
// of the handle's is written but -- when the cell search ran -- the record behind nbody_pair_search_stats.
template <class F>
int neighbors(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, int32_t* neighbor, double* dist2, size_t cap,
              size_t* n_out, uint64_t stats[2]);
template <class F>
int density(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, double* rho, double* rk2, size_t cap, size_t* n_out);
template <class F>
int density_center(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, double center[3], double* rho_sum);

}}  // namespace nbody::knn
