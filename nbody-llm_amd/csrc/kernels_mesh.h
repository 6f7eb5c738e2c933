// kernels_mesh.h -- launchers of mesh gravity's last stage (kernels_mesh.hip): the gather of a mesh pass, which reads the
// acceleration off the resident potential, rounds it once to the handle's precision, stores it in the shard's acc row and,
// inside a step, kicks and half-drifts the body.  The arithmetic is sample_grid.h's and real.h's.  Internal to libnbody_hip.so.
#pragma once
#include "kernels_pm.h"

namespace nbody { namespace mesh {

// how a pass runs (the mesh_kick_fuse and mesh_keep_kernel knobs)
struct Plan {
    int kick_fuse = 1;     // 1: k_mesh_kick; 0: pm's gather to f64 rows, k_mesh_round, and launch_kick_drift inside a step
    int keep_kernel = 1;   // 1: an isolated grid's transformed kernel is made once per spec; 0: at every pass
    int code() const { return kick_fuse | keep_kernel << 1; }
};
Plan make_plan();   // from the knobs of the handle this thread serves

// k_mesh_kick<F, kReach, kScheme> over the n rows of w.smp.xyz, of which the first *count are live, against w.smp.grid:
// sh.acc[row] = F(0.0 - grad), and with kick_dt kick_half_drift of the row.  rows: the n rows in home-cell order, or null.
template <class F>
void launch_kick(hipStream_t s, const ShardT<F>& sh, const int* count, int n, const deposit::Grid& g, int gradient_op, const int* rows,
                 const pm::Scratch& w, const F* kick_dt);

// k_mesh_round<F>: sh.acc[i] = F(rows3[i]) over the live rows (the f64 rows of pm::launch_gather or of k_sample and k_pm_negate)
template <class F>
void launch_round(hipStream_t s, const ShardT<F>& sh, const int* count, int n, const double* rows3);

}}  // namespace nbody::mesh
