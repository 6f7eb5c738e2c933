// nbody_field.h -- host side of nbody_field_at for handles of either dtype (nbody_field.cpp).
#pragma once
#include "nbody_handle.h"
#include "kernels_field.h"

namespace nbody { namespace field {

// After potentials_device(.., field = true): the bodies are gathered (PAIRS) or the tree stands in FieldBufs (TREE), the
// counters are zeroed.  Sends the probes through the device in batches of kFieldBatch: TREE sorts each batch by Morton key,
// walks it and scatters back in the reduce; PAIRS sums K slices of the body list.  K is chosen once per call, so a probe's
// bits do not depend on the batch or the lane it lands in.
int run(NbodyHandle* h, int mode, const PotBodies& b, double g, const double* xyz, size_t n_points, double* acc, double* phi, uint64_t counts[2]);

}}  // namespace nbody::field
