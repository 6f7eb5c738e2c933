// nbody_deposit.h -- the grid deposit behind include/nbody_hip.h ("grid deposit"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_deposit.h"

#include <string>

namespace nbody { namespace deposit {

// (spec_refusal and the host call are deposit_grid.h's)

// The caller has bound the device, refused the handles nbody_moments refuses (diag::refusal), confirmed enqueued steps and
// checked the spec and the capacity.  n_upper >= the live count of sh (the host's view, which no call refreshes): the launches
// are sized from it and read the live count on the device.  Scratch is allocated and freed inside the call; nothing of the
// handle's is written but the record behind nbody_deposit_stats.  grid and counts may be null.
template <class F>
int deposit(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, double* grid, uint64_t* counts);

}}  // namespace nbody::deposit
