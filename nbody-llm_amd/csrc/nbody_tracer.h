// nbody_tracer.h -- host side of the tracers (nbody_tracers_*, include/nbody_hip.h) of an f32 single-rank handle (nbody_tracer.cpp).
#pragma once
#include "nbody_handle.h"
#include "kernels_tracer.h"

namespace nbody { namespace tracer {

inline bool on(const NbodyHandle* h) { return h->tr.n_host > 0; }

// nullptr if the handle takes tracers, else why not (the caller prefixes the entry point's name)
const char* refusal(const NbodyHandle* h);

int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride, size_t capacity);
int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out);
int count(NbodyHandle* h, size_t* n_out);
int stats(NbodyHandle* h, uint64_t out[2]);
int reset_stats(NbodyHandle* h);
int clone_state(const NbodyHandle* src, NbodyHandle* dst);   // (src's stream is idle)

// the step's pieces, enqueued on the handle's stream; each returns at once when the handle has no tracers
int drift_retain(NbodyHandle* h, float dt);                  // half drift + retain of the tracer vector
int forces(NbodyHandle* h, const float* kick_dt);            // brute force: the tracer force pass over the bodies as they stand; kick_dt: + kick and half drift
int tree_forces(NbodyHandle* h, const nbody::TreeDev& td, const float* kick_dt);   // Barnes-Hut: the tracers' walk of the tree the body pass just built; kick_dt: likewise

}}  // namespace nbody::tracer
