// nbody_f32.h -- F = f32 handles (NbodyConfig.dtype == NBODY_F32) on one shard or over index-block shards, and the body store
// of a spatial shard: internal entry points behind include/nbody_hip.h.  Name for name what nbody_f64.h has for F = f64; what
// the two are the same text in is nbody_engine.h's.
#pragma once
#include "nbody_handle.h"

namespace nbody32 {

// the bodies, their settings and the tree of an f32 handle (a base of nbody_f32.cpp's State)
EngineBodies<float>& bodies(NbodyHandle* h);
const EngineBodies<float>& bodies(const NbodyHandle* h);

int create(NbodyHandle* h);                                   // after the stream (and, for Barnes-Hut, pool + counters) exist and the handle has its shape
void destroy(NbodyHandle* h);
int clone_state(NbodyHandle* src, NbodyHandle* dst);
int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride);
int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out);
int count(NbodyHandle* h, size_t* n_out);
int count_global(NbodyHandle* h, size_t* n_out);
int add_point(NbodyHandle* h, const void* particle);          // index-block shards: collective
int remove_point(NbodyHandle* h, size_t index);               // likewise
int merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts);   // nbody_pairs.h
int init(NbodyHandle* h);
int step_by(NbodyHandle* h, float dt);
int steps(NbodyHandle* h, int k);
int update_forces(NbodyHandle* h);
int stats(NbodyHandle* h, NbodyStats* out);
int reset_stats(NbodyHandle* h);
int energy(NbodyHandle* h, double* kinetic, double* potential);
int tree_export_quadrupoles(NbodyHandle* h, float* q6, size_t cap, size_t* n_nodes);
// (potentials_device: nbody_pot.h, beside the f64 one)

// Barnes-Hut steps enqueued without a read-back: confirms them, or replays from the step whose build needed the host.  Every
// call that reads or changes the state starts with it; NBODY_OK at once on a handle that enqueues no such steps (f64 ones included).
int resolve_async(NbodyHandle* h);

// the phases of a step between the exchanges, for the one-process emulation of G ranks (nbody_debug_step_*): begin, the caller's
// copy of every peer's segment, forces, the caller's copy of the partial sums (debug_import_partials), finish
int step_begin(NbodyHandle* h, float dt);
int step_forces(NbodyHandle* h, float dt);
int step_finish(NbodyHandle* h, float dt);
int debug_import_partials(NbodyHandle* h, NbodyHandle* peer);

}  // namespace nbody32
