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

// What solve enqueues between its two copies, for a caller whose mass is on the device already (nbody_pm.cpp): the tables of t
// on their way up -- t outlives the caller's synchronisation -- and every launch from k_poisson_load to k_poisson_store, so
// that w.real, which held the mass, holds phi.  Nothing is waited for and no record is written.  launches_out and
// transforms_out (may be null): the butterfly launches made and the 3-D transforms (2 periodic, 3 isolated).
// held (nbody_mesh.cpp, whose scratch outlives the call): what w holds already and is neither sent nor made again -- the tables
// (kHeldTables), and on an isolated grid the transformed kernel in w.k (kHeldKernel: two transforms then, every output's
// expression tree as it was).  split (nbody_p3m.cpp): t is tables_of(..., r_split > 0), whose D carries the Gaussian split:
// k_poisson_green multiplies by it whatever ps.deconvolve is, and w was laid out with room for D.
enum { kHeldTables = 1, kHeldKernel = 2 };
// the twiddles, the Green factors and the deconvolution factors of t on their way to w's three axes (t outlives the wait)
hipError_t upload_tables(NbodyHandle* h, const Tables& t, const Scratch& w);
hipError_t enqueue(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const Shape& sh, const Tables& t, const Plan& plan,
                   const Scratch& w, int* launches_out, int* transforms_out, int held = 0, bool split = false);

}}  // namespace nbody::poisson
