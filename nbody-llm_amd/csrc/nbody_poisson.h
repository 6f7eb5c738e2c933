// nbody_poisson.h -- the grid Poisson solve behind include/nbody_hip.h ("grid Poisson"): the internal entry point.
#pragma once
#include "nbody_handle.h"
#include "kernels_poisson.h"

namespace nbody { namespace poisson {

// (call_refusal and the host calls are poisson_grid.h's)

// The caller has bound the device, refused the handles nbody_deposit refuses, confirmed enqueued steps and checked the call
// (poisson_grid.h call_refusal) and the capacity.  The handle lends its stream and its memory: scratch is one allocation, freed
// inside the call; nothing of the handle's is written but the record behind nbody_grid_poisson_stats.  mass may be phi.
int solve(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const double* mass, double* phi);

}}  // namespace nbody::poisson
