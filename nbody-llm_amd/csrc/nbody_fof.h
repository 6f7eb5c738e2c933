// nbody_fof.h -- the friends-of-friends group finder behind include/nbody_hip.h ("friends-of-friends groups"): internal entry
// points.
#pragma once
#include "nbody_handle.h"
#include "kernels_fof.h"

namespace nbody { namespace fof {

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal), confirmed enqueued steps and
// checked the linking length and min_members.  n_upper >= the live count of sh (the host's view, which neither call
// refreshes): the launches are sized from it and read the live count on the device.  Scratch is allocated and freed inside the
// call; nothing of the handle's is written.
template <class F>
int labels(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double linking_length, int32_t* label, size_t cap, size_t* n_out,
           size_t* n_groups_out);
template <class F>
int groups(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double linking_length, int min_members, NbodyGroup* groups,
           size_t group_cap, size_t* n_groups, int32_t* members, size_t member_cap, size_t* n_members);
// nbody_fof_bound_groups: groups' catalogue, then evaluation passes (kernels_unbind.h) until no listed group has an unbound
// member or max_iterations is reached; one integer crosses to the host per pass.  The caller has also checked min_members >= 2
// and 1 <= max_iterations <= 1024.
template <class F>
int bound_groups(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, double linking_length, int min_members,
                 int max_iterations, NbodyBoundGroup* groups, size_t group_cap, size_t* n_groups, int32_t* members, size_t member_cap,
                 size_t* n_members, double* energy);

}}  // namespace nbody::fof
