"""The leapfrog under mesh gravity restated (include/nbody_hip.h, "mesh gravity"): external_ref.leapfrog_orbits' loop -- half drift,
retain by the inclusive walls with order kept, the kick, half drift -- with a = F(nb.host_pm_field(x, m, ...).acc) [+ external_ref.acc].
Nothing is restated here but the loop: the field is the library's host call, the grids and worlds are pm_ref's."""
import numpy as np

import external_ref
import pm_ref


def field(nb, x, m, g, grid, scheme, gradient, dtype, points=None, **poisson):
    """F(nbody_host_pm_field(x, m, grid, g).acc) at the bodies, or at points: [n, 3] of dtype, rounded once"""
    origin, spacing, dims, periodic, axis = pm_ref.GRIDS[grid]
    acc = nb.host_pm_field(np.asarray(x, np.float64), np.asarray(m, np.float64), origin, spacing, dims, float(g), scheme=scheme, gradient=gradient,
                           periodic=periodic, project_axis=axis, points=None if points is None else np.asarray(points, np.float64), phi=False,
                           **poisson)[0]
    return acc.astype(dtype)


def _half_drift_retain(rec, dt, lo, hi, F):
    x = rec["position"] + (rec["velocity"] * F(0.5)) * dt
    keep = ((x >= F(lo)) & (x <= F(hi))).all(axis=1)   # (a NaN fails every comparison and is dropped)
    rec = rec[keep]
    rec["position"] = x[keep]
    return rec


def _kick_half_drift(rec, a, dt, F):
    v = rec["velocity"] + a * dt
    rec["velocity"] = v
    rec["position"] = rec["position"] + (v * F(0.5)) * dt
    rec["acceleration"] = a
    return rec


def step(nb, rec, dts, lo, hi, g, grid, scheme, gradient, ext=None, tracers=None, **poisson):
    """rec after one step per dt (and the tracers, when given: (rec, tracers)).  g: the handle's g; it is rounded to the records'
    dtype and widened, as the handle holds it.  ext: external_ref components.  tracers: PointParticle<f32> records."""
    rec = rec.copy()
    tr = None if tracers is None else tracers.copy()
    dtype = rec["position"].dtype
    F = dtype.type
    g = F(g)
    for dt in dts:
        dt = F(dt)
        rec = _half_drift_retain(rec, dt, lo, hi, F)
        if tr is not None:
            tr = _half_drift_retain(tr, dt, lo, hi, F)
        x, m = rec["position"], rec["mass"]
        a = field(nb, x, m, g, grid, scheme, gradient, dtype, **poisson)
        if ext:
            a = a + external_ref.acc(ext, g, x, dtype)
        if tr is not None:
            at = field(nb, x, m, g, grid, scheme, gradient, dtype, points=tr["position"], **poisson)
            if ext:
                at = at + external_ref.acc(ext, g, tr["position"], dtype)
            tr = _kick_half_drift(tr, at, dt, F)   # (the bodies' positions above are the half-drifted ones: read before their kick)
        rec = _kick_half_drift(rec, a, dt, F)
    return rec if tracers is None else (rec, tr)


def forces(nb, rec, g, grid, scheme, gradient, **poisson):
    """what nbody_update_forces leaves in the acceleration rows under mesh gravity"""
    dtype = rec["position"].dtype
    return field(nb, rec["position"], rec["mass"], dtype.type(g), grid, scheme, gradient, dtype, **poisson)
