// kernels_external.h -- launchers of the external-field kernels (kernels_external.hip); internal to libnbody_hip.so.
#pragma once
#include "external_field.h"
#include "shard.h"

namespace nbody { namespace ext {

constexpr int kExtBlock = 256;

// acc_c = acc_c + s_c(pos) for the live bodies (or tracers) of sh, s from acc_sum<F>; kick_dt != null: the kick + half drift
// of k_kick_drift on the new acceleration in the same lane (the same rounded operations: the bits of k_ext_add followed by
// k_kick_drift).  Honours sh.poison like k_kick_drift; count_step: this launch is the step's kick of the BODIES and bumps the
// step-complete count at poison + 1 (the tracers' launch does not).  With count_step and a poison word an empty shard still
// launches one block.
template <class F>
void launch_ext_add(hipStream_t s, const ShardT<F>& sh, int n_upper, const FieldT<F>& f, F g, const F* kick_dt, bool count_step);

// phi_i = phi_sum(pos_i) in f64 for the n_upper >= live bodies (phi may be null) and, per block of kExtBlock bodies, the sum
// of m_i phi_i added pairwise in a fixed tree (part[blocks_for(n_upper)]; bodies past the live count add 0)
template <class F>
void launch_ext_phi(hipStream_t s, const ShardT<F>& sh, int n_upper, const FieldT<double>& f, double g, double* phi, double* part);

// probes: xyz [n][3] -> acc [n][3] and / or phi [n] (either may be null), all f64
void launch_ext_at(hipStream_t s, const double* xyz, int n, const FieldT<double>& f, double g, double* acc, double* phi);

inline int blocks_for(int n) { return n <= 0 ? 0 : (n + kExtBlock - 1) / kExtBlock; }

}}  // namespace nbody::ext
