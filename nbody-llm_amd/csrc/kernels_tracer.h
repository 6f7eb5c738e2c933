// kernels_tracer.h -- launchers of the tracer force passes (kernels_tracer.hip; internal to libnbody_hip.so).
//
// Tracers are massless particles that feel the bodies and exert nothing (include/nbody_hip.h, "tracers").  Their state is a
// second nbody::Shard of one segment, so the half drift, the retain and the kick + half drift are the bodies' kernels
// (kernels_integrate.hip) launched on that struct, unchanged.  What is new is the ONE-SIDED force pass: tracers x bodies.
#pragma once
#include "kernels.h"

namespace nbody {

// Shape of the fast pass for m tracers in the field of n bodies (host upper bounds of both):
//   a lane keeps `ipt` tracers in registers, a workgroup of kTrBlock lanes a GROUP of kTrBlock * ipt of them;
//   the body range is cut into K SLICES of slice_len bodies (the last one shorter), one workgroup per (group, slice).
// K == 1: the kernel writes the accelerations itself; K > 1: planes [K][groups * kTrBlock * ipt] and a reduce kernel.
constexpr int kTrBlock = 256;
constexpr int kTrTile = 1024;     // bodies per LDS tile
constexpr int kTrMaxSlices = 256;
struct TracerPlan { int ipt; int groups; int K; int slice_len; };
TracerPlan tracer_plan(size_t n_tracers, size_t n_bodies);
inline size_t tracer_plan_pad(const TracerPlan& p) { return size_t(p.groups) * kTrBlock * size_t(p.ipt); }

// `tr`: the tracers' state (one segment); `bodies`: the handle's single-shard body state, read only.
// stats (may be null): [0] += live tracers x live bodies, counted on the device.
// kick_dt != nullptr: integrate_after_force of the tracers rides in the pass (the arithmetic of k_kick_drift).
void launch_tr_bf_strict(hipStream_t s, const Shard& tr, int m_upper, const Shard& bodies, float g, float g_soft2,
                         unsigned long long* stats);
void launch_tr_bf_fast(hipStream_t s, const Shard& tr, int m_upper, const Shard& bodies, const TracerPlan& p, float4* planes,
                       float g, float g_soft2, const float* kick_dt, unsigned long long* stats);

// ---- Barnes-Hut handles: the tracers walk the tree the body force pass just built (k_tr_bh_walk, beside the walks it is
// modelled on in kernels_bh.hip), monopoles only.
// The live tracers in tree order (kernels_tree.hip: the build's key kernel and the probes' sort): keys [2][n_cap], idx [2][n_cap],
// scratch_info [3] ints; *sorted_idx = the sorted half of idx.  0 on success
size_t tracer_sort_tmp_bytes(size_t n_cap);
int tracer_sort(hipStream_t s, const float4* pos, const int* d_count, int n_upper, const float center[3], float width, void* tmp, size_t tmp_bytes,
                unsigned long long* keys, int* idx, size_t n_cap, int* scratch_info, const int** sorted_idx);
// runs of consecutive node-range segments the walk of m_upper tracers is cut into (1 .. n_split)
int tracer_walk_groups(size_t m_upper, int n_split);
// t: the body pass's nodes, split points and poison flag (its order, planes and counts are not touched);
// planes [groups][plane_stride] (groups > 1); counters [NBODY_WALK_COUNTER_SLOTS][2] += {accepted, visited}
void launch_tr_bh_walk(hipStream_t s, const Shard& tr, int m_upper, const int* idx, const TreeDev& t, int groups, float4* planes,
                       size_t plane_stride, float g, float g_soft2, float theta2, int leaf_direct, const float* kick_dt,
                       unsigned long long* counters);

}  // namespace nbody
