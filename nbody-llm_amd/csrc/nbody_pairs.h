// nbody_pairs.h -- the binary census behind include/nbody_hip.h ("binary census"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_pairs.h"

namespace nbody { namespace pairs {

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal) and confirmed enqueued steps.
// n_upper >= the live count of sh (the host's view, which neither call refreshes): the launches are sized from it and read the
// live count on the device.  g and g_soft are the handle's, widened.  Scratch is allocated and freed inside the call; nothing
// of the handle's is written.
template <class F>
int partners(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, int32_t* partner, double* energy, size_t cap,
             size_t* n_out);
template <class F>
int bound_pairs(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, NbodyBoundPair* pairs, size_t cap,
                size_t* n_pairs, double* binding_sum);

}}  // namespace nbody::pairs
