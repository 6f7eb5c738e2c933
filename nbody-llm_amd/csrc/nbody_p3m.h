// nbody_p3m.h -- the P3M field behind include/nbody_hip.h ("P3M field"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_p3m.h"

namespace nbody { namespace p3m {

// (call_refusal and the host calls are p3m_pairs.h's)

// The caller has bound the device, refused the handles nbody_deposit refuses, confirmed enqueued steps and checked the call
// (p3m_pairs.h call_refusal).  n_upper >= the live count of sh, as in nbody_pm.h.  Scratch is one allocation -- the mesh stages'
// (kernels_pm.h) and the short-range part's (kernels_p3m.h) one after the other --, freed inside the call; nothing of the handle's
// is written but the record behind nbody_p3m_field_stats.  phi, cls, n_out and counts may be null.
template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyP3mSpec& p3m, double* acc, double* phi,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts);

// the same at n_points caller points: the bodies are deposited, solved and ordered by chain cell once, the points go by in batches
template <class F>
int at_points(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyP3mSpec& p3m, const double* xyz,
              size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts);

}}  // namespace nbody::p3m
