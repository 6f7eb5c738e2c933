// nbody_f64.h -- F = f64 handles (NbodyConfig.dtype == NBODY_F64): internal entry points behind include/nbody_hip.h.
#pragma once
#include "nbody_handle.h"

namespace nbody64 {

// the bodies, their settings and the tree of an f64 handle (a base of nbody_f64.cpp's State)
EngineBodies<double>& bodies(NbodyHandle* h);
const EngineBodies<double>& bodies(const NbodyHandle* h);

int create(NbodyHandle* h);                                   // after the stream (and, for Barnes-Hut, pool + counters) exist and the handle has its shape
void destroy(NbodyHandle* h);
int clone_state(NbodyHandle* src, NbodyHandle* dst);
int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride);
int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out);
int count(NbodyHandle* h, size_t* n_out);
int count_global(NbodyHandle* h, size_t* n_out);
int add_point(NbodyHandle* h, const void* particle);
int remove_point(NbodyHandle* h, size_t index);
int merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts);   // nbody_pairs.h, + a removal's bookkeeping
int set_settings(NbodyHandle* h, double g, double g_soft, double dt, double theta2);   // (the setters and init invalidate the Hermite state)
int set_bounds(NbodyHandle* h, const double center[3], double width);
int init(NbodyHandle* h);
int step_by(NbodyHandle* h, double dt);
int steps(NbodyHandle* h, int k);
int update_forces(NbodyHandle* h);
int stats(NbodyHandle* h, NbodyStats* out);
int reset_stats(NbodyHandle* h);
int energy(NbodyHandle* h, double* kinetic, double* potential);
// the fourth-order Hermite integrator (brute force, one rank; include/nbody_hip.h "integrator")
int set_integrator(NbodyHandle* h, int integrator);
int get_integrator(const NbodyHandle* h);
int download_jerk(NbodyHandle* h, double* jerk3, size_t cap, size_t* n_out);
int suggest_dt(NbodyHandle* h, double eta, double* dt_out);
// block individual time steps of a Hermite handle (include/nbody_hip.h "block steps"); refused on a leapfrog handle
int set_block_steps(NbodyHandle* h, double eta, int max_level);
int get_block_steps(const NbodyHandle* h, double* eta, int* max_level);
int download_levels(NbodyHandle* h, int32_t* level, size_t cap, size_t* n_out);
int block_step_counts(NbodyHandle* h, uint64_t out[2]);
int debug_hermite_forces_of(NbodyHandle* h, const int32_t* ids, size_t n_ids, double* acc3, double* jerk3);

}  // namespace nbody64
