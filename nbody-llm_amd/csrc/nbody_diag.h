// nbody_diag.h -- whole-state diagnostics behind include/nbody_hip.h ("diagnostics of the state as a whole"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_diag.h"

namespace nbody { namespace diag {

// why the handle takes neither call (null: it does)
const char* refusal(const NbodyHandle* h);

// The callers have bound the device and confirmed enqueued steps.  n_upper >= the live count of sh (the host's view, which
// neither call refreshes): the launches are sized from it and read the live count on the device.  Scratch is allocated and
// freed inside the call; nothing of the handle's is written.
template <class F>
int moments(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double out[10]);
// center == nullptr: the centre of mass X / M of moments()
template <class F>
int lagrangian_radii(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* center, const double* fractions, size_t n_frac,
                     double* radii, double* mass_out);

}}  // namespace nbody::diag
