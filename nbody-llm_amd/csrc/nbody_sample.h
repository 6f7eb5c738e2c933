// nbody_sample.h -- the grid sample behind include/nbody_hip.h ("grid sample"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_sample.h"

namespace nbody { namespace sample {

// (call_refusal and the host call are sample_grid.h's)

constexpr size_t kPointBatch = size_t(1) << 22;   // nbody_grid_sample_at: points per pass over the uploaded grid

// The caller has bound the device, refused the handles nbody_deposit refuses, confirmed enqueued steps and checked the call
// (sample_grid.h call_refusal).  n_upper >= the live count of sh (the host's view, which no call refreshes): the launches are
// sized from it and read the live count on the device.  Scratch is one allocation, freed inside the call; nothing of the
// handle's is written but the record behind nbody_grid_sample_stats.  cls, n_out and counts may be null.
template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const double* grid, int fields, int op, double* out,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts);

// the same at n_points caller points: the handle lends its stream and its memory only
int at_points(NbodyHandle* h, const NbodyGridSpec& spec, const double* grid, int fields, int op, const double* xyz, size_t n_points, double* out,
              uint8_t* cls, uint64_t* counts);

}}  // namespace nbody::sample
