// nbody_field.h -- host side of nbody_field_at and nbody_tidal_at for handles of either dtype (nbody_field.cpp).
#pragma once
#include "nbody_handle.h"
#include "kernels_field.h"

namespace nbody { namespace field {

// After potentials_device(.., field = true): the bodies are gathered (PAIRS) or the tree stands in FieldBufs (TREE), the
// counters are zeroed.  Sends the probes through the device in batches of kFieldBatch: TREE sorts each batch by Morton key,
// walks it and scatters back in the reduce; PAIRS sums K slices of the body list.  K is chosen once per call, so a probe's
// bits do not depend on the batch or the lane it lands in.
// What the call returns: nbody_field_at acc [n][3] and phi [n]; nbody_tidal_at (tidal = true) tidal6 [n][6], the same
// kernels with another ProbeTerm over the same batches.  Every pointer may be null (all null: count only).
struct Out {
    double* acc = nullptr;
    double* phi = nullptr;
    double* tidal6 = nullptr;
    bool tidal = false;
};
int run(NbodyHandle* h, int mode, const PotBodies& b, double g, const double* xyz, size_t n_points, const Out& out, uint64_t counts[2]);

}}  // namespace nbody::field
