// pm_grid.h -- nbody_host_pm_field and the checks of nbody_pm_field and nbody_pm_field_at (include/nbody_hip.h, "particle-mesh
// field"), stated once: the C entry points (nbody_api.cpp) and tools/sanitize_pm.cpp run this code, and tests/pm_ref.py restates
// it by composing the three restatements.  There is no arithmetic here but the negation: the call IS the composition of
// deposit_grid.h's, poisson_grid.h's and sample_grid.h's host calls.
#pragma once

#include "poisson_grid.h"
#include "sample_grid.h"

namespace nbody { namespace pm {

// why the call is not valid (empty: it is): the union of what the three calls refuse in a spec, and the call's own
inline std::string call_refusal(const NbodyGridSpec* spec, const NbodyPmSpec* pm) {
    std::string why = deposit::spec_refusal(spec, true);
    if (!why.empty()) return why;
    if (spec->quantity != NBODY_DEPOSIT_MASS) return "quantity must be NBODY_DEPOSIT_MASS (0)";
    if (!pm) return "pm is NULL";
    const double held = 0.0;   // (the grids are the call's own: only the spec and the constants are looked at)
    why = poisson::call_refusal(spec, &pm->poisson, &held, &held);
    if (!why.empty()) return why;
    if (pm->gradient != NBODY_SAMPLE_GRADIENT2 && pm->gradient != NBODY_SAMPLE_GRADIENT4)
        return "gradient must be NBODY_SAMPLE_GRADIENT2 (1) or NBODY_SAMPLE_GRADIENT4 (2)";
    if (pm->reserved[0] != 0 || pm->reserved[1] != 0 || pm->reserved[2] != 0) return "reserved must be 0";
    return sample::call_refusal(spec, &held, 1, pm->gradient);
}

// the composition, on a checked call.  xyz == nullptr: the points are the bodies.  r_split (p3m_pairs.h): poisson::host_call's
inline int host_call(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec& spec, const NbodyPmSpec& pm,
                     const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts, double r_split = 0.0) {
    const size_t cells = deposit::cells_of(deposit::grid_of(spec));
    std::vector<double> grid(cells, 0.0);   // M, then Phi in place (nbody_host_grid_poisson allows it)
    uint64_t counted[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = deposit::host_call(body_xyz, body_m, n_bodies, spec, grid.data(), cells, counted);
    if (rc) return rc;
    rc = poisson::host_call(spec, pm.poisson, grid.data(), grid.data(), r_split);
    if (rc) return rc;
    const double* P = xyz ? xyz : body_xyz;
    const size_t n = xyz ? n_points : n_bodies;
    rc = sample::host_call(P, n, spec, grid.data(), 1, pm.gradient, acc, cls, counted + 4);
    if (rc) return rc;
    for (size_t i = 0; i < 3 * n; ++i) acc[i] = 0.0 - acc[i];
    if (phi) rc = sample::host_call(P, n, spec, grid.data(), 1, NBODY_SAMPLE_VALUE, phi, nullptr, nullptr);
    if (counts) std::copy(counted, counted + 8, counts);
    return rc;
}

// nbody_host_pm_field
inline int host_entry(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec* spec, const NbodyPmSpec* pm,
                      const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts) {
    if (!call_refusal(spec, pm).empty()) return int(NBODY_ERR_INVALID);
    if ((n_bodies && (!body_xyz || !body_m)) || n_bodies > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    if (xyz && n_points > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    if ((xyz ? n_points : n_bodies) && !acc) return int(NBODY_ERR_INVALID);
    return host_call(body_xyz, body_m, n_bodies, *spec, *pm, xyz, n_points, acc, phi, cls, counts);
}

}}  // namespace nbody::pm
