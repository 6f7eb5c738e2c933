// nbody_pot.h -- host side of nbody_potentials / nbody_energy_world shared by the f32 and the f64 handles (nbody_pot.cpp).
#pragma once
#include "nbody_handle.h"
#include "kernels_pot.h"

namespace nbody { namespace pot {

// d_sum for `bodies` own bodies, the counters (zeroed on the handle's stream for the call that starts here)
int begin(NbodyHandle* h, size_t bodies);
// at least `doubles` entries of PotBufs::d_planes
int ensure_planes(NbodyHandle* h, size_t doubles);
// NBODY_POTENTIAL_PAIRS for n own bodies and n_remote bodies of the other blocks: S_i into PotBufs::d_sum
int pairs(NbodyHandle* h, const PotBodies& b, size_t n, size_t n_remote, double eps2);
// phi_i = -g S_i for the n own bodies to the caller's buffer, {terms summed, opening tests} of the call
int download(NbodyHandle* h, size_t n, double g, double* phi, size_t cap, size_t* n_out, uint64_t counts[2]);
// KE and 1/2 sum m_i phi_i of the n own bodies (block partials added in block order), then every rank's pair through
// Transport::host_all_gather, added in rank order
int energy(NbodyHandle* h, const PotBodies& b, size_t n, double g, double* kinetic, double* potential);

}}  // namespace nbody::pot

// S_i of the own bodies into PotBufs::d_sum at the handle's current positions (collective on a sharded world); *n = own bodies
// field = true: nbody_field_at's preparation (nbody_f32.cpp potentials_device has the contract, nbody_api.cpp's the checks)
namespace nbody64 {
int potentials_device(NbodyHandle* h, int mode, size_t* n, nbody::PotBodies* bodies, double* g, bool field = false);
}
namespace nbody32 {
int potentials_device(NbodyHandle* h, int mode, size_t* n, nbody::PotBodies* bodies, double* g, bool field = false);
}
