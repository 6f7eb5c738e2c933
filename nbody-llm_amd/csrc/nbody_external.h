// nbody_external.h -- the static external field behind include/nbody_hip.h ("external field"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_external.h"

namespace nbody { namespace ext {

inline bool on(const NbodyHandle* h) { return h->ext.n > 0; }
// why the handle takes no field (null: it does)
const char* refusal(const NbodyHandle* h);
// "" or what is wrong with the components: kind, reserved, finite, ranges -- as given and, f32 != 0, as rounded to f32
std::string invalid(const NbodyExternalComponent* comps, size_t n, bool f32);
// the field in the precision of a pass (centre and parameters rounded to F)
template <class F> FieldT<F> rounded(const ExternalField& e);

// after a force pass: acc += s(pos) on the shard (bodies: count_step, tracers: not), with the step's kick + half drift when
// kick_dt is given.  Enqueues only.
template <class F>
int add(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, F g, const F* kick_dt, bool count_step);

// the callers have bound the device, confirmed enqueued steps and refreshed the live count n of sh
template <class F>
int potentials(NbodyHandle* h, const ShardT<F>& sh, size_t n, double g, double* phi, double* energy);
int at(NbodyHandle* h, double g, const double* xyz, size_t n_points, double* acc, double* phi);

}}  // namespace nbody::ext
