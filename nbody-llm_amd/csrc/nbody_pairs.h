// nbody_pairs.h -- the binary census and the sticky mergers behind include/nbody_hip.h ("binary census", "sticky mergers"):
// internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_pairs.h"

namespace nbody { namespace pairs {

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal) and confirmed enqueued steps.
// n_upper >= the live count of sh (the host's view, which neither call refreshes): the launches are sized from it and read the
// live count on the device.  g and g_soft are the handle's, widened.  Scratch is allocated and freed inside the call; nothing
// of the handle's is written.
template <class F>
int partners(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, int32_t* partner, double* energy, size_t cap,
             size_t* n_out);
template <class F>
int bound_pairs(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, NbodyBoundPair* pairs, size_t cap,
                size_t* n_pairs, double* binding_sum);

// ---- sticky mergers.  nearest and contacts: the contract above, nothing of the handle's is written.  The callers have checked
// the radius.
template <class F>
int nearest(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int32_t* nearest_out, double* dist2, size_t cap, size_t* n_out);
template <class F>
int contacts(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, NbodyContact* list, size_t cap, size_t* n_contacts);
// The contacts of b's bodies, then -- unless there is none, or `list` is too short -- the merged records into their rows and
// the handle's retain: `retain(h, n_upper)` enqueues it (launch_compact, or launch_hm_compact with the jerk and the levels),
// `jerk` is a Hermite handle's held j0 (else null).  With *n_contacts > 0 on NBODY_OK b's view of the count is exact again
// (BodyStore::set_own_count, as nbody_remove_point leaves it) and the caller marks what else a removal makes stale; a call
// that found nothing has written nothing, on the device or here.
template <class F>
int merge_contacts(NbodyHandle* h, BodyStore<F>& b, double radius, NbodyContact* list, size_t cap, size_t* n_contacts,
                   typename ShardT<F>::V4* jerk, void (*retain)(NbodyHandle*, int));

}}  // namespace nbody::pairs
