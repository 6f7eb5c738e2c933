// nbody_mesh.h -- mesh gravity behind include/nbody_hip.h ("mesh gravity"): the setting of a handle, the state that stays on
// the device between passes, and the pass both engines call in place of their pair kernels.
#pragma once
#include "nbody_handle.h"
#include "kernels_mesh.h"

namespace nbody { namespace mesh {

inline bool on(const NbodyHandle* h) { return h->mesh.on; }

// nullptr if the handle takes mesh gravity, else why not (the caller prefixes the entry point's name)
const char* refusal(const NbodyHandle* h);

// the setting, checked by the caller (pm_grid.h call_refusal); the resident state is made by the first pass
void set(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPmSpec& pm);
// off: the stream is waited for and the resident state freed; the counters behind nbody_mesh_gravity_stats stay
int clear(NbodyHandle* h);
// what nbody_destroy does before the registry lets every block go
void destroy(NbodyHandle* h);

// The self-gravity pass of a handle with mesh gravity on, enqueued on the handle's stream: with x the positions of the live rows
// of sh (n_upper >= their number, the host's view) and g the handle's g, widened exactly,
//     sh.acc[i] = F(nbody_host_pm_field(x, m, spec, pm with poisson.g := g).acc[i])
// and, with kick_dt, real.h's kick_half_drift of every live row.  An f32 handle's tracers get the same field at their own
// positions (tracer_kick_dt: their kick).  No synchronisation, no allocation and no read-back unless the resident state must
// be made or regrown, which happens before anything is enqueued.
template <class F>
int pass(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, const F* kick_dt, const float* tracer_kick_dt);

}}  // namespace nbody::mesh
