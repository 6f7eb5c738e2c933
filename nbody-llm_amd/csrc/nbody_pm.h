// nbody_pm.h -- the particle-mesh field behind include/nbody_hip.h ("particle-mesh field"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_pm.h"

namespace nbody { namespace pm {

// (call_refusal and the host call are pm_grid.h's)

// The caller has bound the device, refused the handles nbody_deposit refuses, confirmed enqueued steps and checked the call
// (pm_grid.h call_refusal).  n_upper >= the live count of sh (the host's view, which no call refreshes): the launches are sized
// from it and read the live count on the device.  Scratch is one allocation, freed inside the call; nothing of the handle's is
// written but the record behind nbody_pm_field_stats.  phi, cls, n_out and counts may be null.
template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, double* acc, double* phi,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts);

// the same at n_points caller points: the bodies are deposited and the grid is solved once, the points go by in batches
template <class F>
int at_points(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const double* xyz,
              size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts);

}}  // namespace nbody::pm
