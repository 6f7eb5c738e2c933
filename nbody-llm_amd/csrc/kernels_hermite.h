// kernels_hermite.h -- launchers of the fourth-order Hermite integrator's kernels (kernels_hermite.hip): brute-force
// NBODY_F64 handles of a one-rank world with nbody_set_integrator(NBODY_INTEGRATOR_HERMITE4).  Internal to libnbody_hip.so.
#pragma once
#include "kernels_f64.h"

namespace nbody64 {

// what a Hermite handle keeps beside Dev's pos / vel / acc (acc holds the held a0)
struct HermiteDev {
    double4* jerk = nullptr;   // [cap] the held j0
    double4* xp = nullptr;     // [cap] predicted {x, y, z, mass}
    double4* vp = nullptr;     // [cap] predicted velocities
    double4* a1 = nullptr;     // [cap] strict math: F at the predicted state, read by the corrector
    double4* j1 = nullptr;     // [cap]
    double* ratio = nullptr;   // [ceil(cap / 256)] nbody_suggest_dt: per-workgroup minima of |a| / |j|
};

// the step's coefficients, rounded once on the host (tests/hermite_ref.py forms the same five numbers):
//   dt,  c2 = (dt * dt) * 0.5,  c3 = ((dt * dt) * dt) / 6,  h = dt * 0.5,  c12 = (dt * dt) / 12
struct HermiteCoef { double dt, c2, c3, h, c12; };
inline HermiteCoef hermite_coef(double dt) { return HermiteCoef{dt, (dt * dt) * 0.5, ((dt * dt) * dt) / 6.0, dt * 0.5, (dt * dt) / 12.0}; }

// xp = ((x0 + v0 * dt) + a0 * c2) + j0 * c3,  vp = (v0 + a0 * dt) + j0 * c2   (separate multiplies and adds)
void launch_hm_predict(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, const HermiteCoef& c);
// NBODY_MATH_STRICT: (a, j) = F(x, v), one body per lane, partners in ascending index order, in the expression order
// include/nbody_hip.h states; adds n (n - 1) to Dev::inter
void launch_hm_strict(hipStream_t s, const Dev& d, const double4* x, const double4* v, double4* out_a, double4* out_j, int n_upper, double g, double eps2);
// the corrector on (hd.a1, hd.j1), in place on pos / vel / acc / jerk, with Bounds::contains' flags for the retain:
//   v1 = (v0 + (a0 + a1) * h) + (j0 - j1) * c12,  x1 = (x0 + (v0 + v1) * h) + (a0 - a1) * c12
void launch_hm_correct(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, const HermiteCoef& c, const Bounds64& b);
// Vec::retain over pos, vel, acc and jerk together (retain.h's tile scan with a fourth array)
// level != nullptr: the block-step levels travel along
void launch_hm_compact(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, int* level = nullptr);
// per-workgroup minima of |a_i| / |j_i| over live bodies with |j_i| > 0 (+inf where there is none) -> hd.ratio; returns the workgroups
int launch_hm_min_ratio(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper);

// NBODY_MATH_FAST: every unordered pair once (k_hm_sym, kernels_bf64.hip's scheme with velocities and six accumulators a
// side) + the left-over pairs one-sided (k_hm_os), into planes of double4[n_pad]: plane p of the accelerations at
// planes + p * n_pad, of the jerks at planes + (n_planes + p) * n_pad.  A plan from make_bf64_plan(.., hermite_ipt(bf64_ipt)).
// Bodies per lane of a resident set: four (104 registers of resident state) at every size; eight only where bf64_ipt asks
// for it (it builds without scratch but spills 118..148 registers into the accumulation file and runs one wave per SIMD:
// DESIGN.md section 3.10)
inline int hermite_ipt(int bf64_ipt) { return bf64_ipt == 8 ? 8 : 4; }
void launch_hm_sym(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* x, const double4* v, double4* planes, double eps2);
void launch_hm_own(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* x, const double4* v, double4* planes, double eps2);
// the planes added in a fixed order, times g, into (out_a, out_j); c != nullptr: the corrector rides along instead (in place
// on pos / vel / acc / jerk, as launch_hm_correct).  Adds n (n - 1) to Dev::inter.
void launch_hm_reduce(hipStream_t s, const Dev& d, const HermiteDev& hd, const Bf64Plan& p, const double4* planes, int n_upper, double g,
                      double4* out_a, double4* out_j, const HermiteCoef* c, const Bounds64& b);

// ---- block individual time steps (nbody_set_block_steps; include/nbody_hip.h "block steps")
// what a handle with block steps keeps beside HermiteDev
struct BlockDev {
    int* level = nullptr;        // [cap] l_i: body i steps by T >> l_i ticks; carried across macro steps (and by the retain)
    int* tau = nullptr;          // [cap] tick of body i's last correction within the macro step
    int* list = nullptr;         // [cap] the due bodies of the block step, ascending
    int* tile_count = nullptr;   // [ceil(cap / 1024)] due bodies per 1024-body tile
    int* smin = nullptr;         // [2] min (tau_i + s_i) of this block step and the slot armed for the next; then
    int* sched = nullptr;        // [2] = smin + 2: {tau*, due bodies}, what the host reads back once per block step
    double4* planes = nullptr;   // k_hm_act's partial sums: K planes of accelerations, then K of jerks, groups * 64 rows each
    size_t plane_rows = 0;       // rows of one kind the buffer holds (hm_act_plane_rows)
};
// start levels from the held (a0, j0): dtc = eta (|a| / |j|), l = 0, s = |dt|, while (s > dtc && l < max_level) { s *= 0.5; ++l; }
void launch_hmb_start_levels(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_upper, double eta, double abs_dt,
                             int max_level);
// one block step's schedule, three launches: tau* = min (tau_i + (T >> l_i)) into bd.smin[slot] (bd.smin[slot ^ 1] re-armed);
// the due bodies' indices ascending into bd.list and {tau*, how many} into bd.sched; every body predicted to tau* into
// (hd.xp, hd.vp) with its own dp = f64(tau* - tau_i) tick.  bd.smin holds 0x7f7f7f7f in both slots before a macro step's first.
void launch_hmb_schedule(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_upper, int T, double tick, int slot);
// NBODY_MATH_FAST, F of the n_act listed bodies against all n of (x, v): 64-body groups x K partner slices, about bf64_waves
// waves (default 2048), a slice no shorter than one 64-partner tile
struct HmActPlan { int groups = 0, K = 1; };
HmActPlan make_hm_act_plan(int n_act, int n);
size_t hm_act_plane_rows(int cap);   // rows of one kind (accelerations or jerks) any plan of a handle of this capacity needs
void launch_hm_act(hipStream_t s, const Dev& d, const BlockDev& bd, const HmActPlan& p, const double4* x, const double4* v, double eps2);
// NBODY_MATH_STRICT: one listed body per lane, partners ascending; row p of (hd.a1, hd.j1) belongs to bd.list[p]
void launch_hm_act_strict(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_act, const double4* x, const double4* v,
                          double g, double eps2);
// the due bodies' (a1, j1) (p != nullptr: the K planes in a fixed order, times g; else rows of hd.a1 / hd.j1), the corrector
// with h_i = f64(T >> l_i) tick, the step criterion and the new level, tau_i = tau*; adds n_act (n - 1) to Dev::inter
void launch_hmb_finish(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, const HmActPlan* p, int n_act, double g, int T,
                       int max_level, double tick, double abs_dt, double eta, const Bounds64& b);
// the planes alone into rows of (hd.a1, hd.j1): nbody_debug_hermite_forces_of on a fast handle
void launch_hm_act_reduce(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, const HmActPlan& p, int n_act, double g);

}  // namespace nbody64
