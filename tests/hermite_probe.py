"""Probe worlds for the Hermite pair-jerk kernels, F(x, v): every mass is 0 except body k's, and EVERY body moves.

With d = x_k - x_i, w = v_k - v_i, q = |d|^2 + eps^2 body i != k then receives exactly one acceleration term and one jerk term,
    S_a = g m_k d / q^(3/2),        S_j = g m_k [ w - 3 (d.w)/q d ] / q^(3/2),
and body k receives exactly nothing (its partners are massless; its self pair is excluded, which eps = 0 checks: the self pair
would give 0 * inf).  A wrong-velocity pair shows only if the velocities differ from body to body, so they are drawn (fixed seed)
and none is zero.  Columns are tests/bf_probe.py's probe_columns; positions, g, eps and the mass are f32-representable as in
tests/test_bf64_fast_gpu.py, so every reference sees exactly the values the handle holds.

check_probe_aj asserts, against the one term in np.longdouble,
    |a_i - S_a| <= PROBE64 |S_a|        (bf64_bound.PROBE64: the twin leapfrog kernels' probe bound)
    |j_i - S_j| <= RJP T_j,             T_j = g m_k (|w| + 3 |d.w| |d| / q) / q^(3/2)   (hermite_ref.direct_aj's convention)
    rows k of a and j exactly zero and finite.
A dropped, doubled, wrong-sign or wrong-velocity pair is an error of order T_j (tests/test_hermite_probe_checker.py).

This module is plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

from bf64_bound import PROBE64
from bf_probe import PROBE_G, PROBE_MASS, probe_columns  # noqa: F401  (re-exported for the probe tests)

#: |j_i - S_j| <= RJP T_j for every body i != k of a probe world.  From arithmetic one term carries the 12 roundings
#: hermite_ref.py's docstring lists and the product with g a 13th: 13 * 2^-53 = 1.4e-15.  Measured on an MI355X over every case of
#: tests/test_hermite_pair_coverage_gpu.py (k_hm_sym<4|8, 0|1>, k_hm_os<0|1>, k_hm_act; 65 to 20 000 bodies): the worst
#: |j - S_j| / T_j is MEASURED_RJP_WORST (n = 20 000 at the default tuning) and the worst |a - S_a| / |S_a| 1.05e-15.  RJP is about
#: 3x the former (bf64_bound.py's convention).  Must stay <= 1e-13: a wrong pair is an error of order T_j, so a larger value would
#: be a finding, not a reason to raise it.
MEASURED_RJP_WORST = 9.4e-16
RJP = 3.0e-15


def probe_velocities(n: int, seed: int = 0) -> np.ndarray:
    """[n, 3] f64 velocities, fixed by (n, seed), every one non-zero and no two equal."""
    v = np.random.default_rng([n, seed, 0x6a]).normal(size=(n, 3)) * 0.5
    assert (np.abs(v).max(1) > 0).all()
    return v


def probe_records64(dtype, pos: np.ndarray, vel: np.ndarray) -> np.ndarray:
    """Records at `pos` ([n, 3]) moving with `vel` ([n, 3]), zero acceleration and mass."""
    rec = np.zeros(len(pos), dtype=dtype)
    rec["position"] = pos
    rec["velocity"] = vel
    return rec


def set_probe(rec: np.ndarray, k: int, mass: float = PROBE_MASS) -> np.ndarray:
    """The same records with every mass 0 except body k's; the velocities stay (in place; returned for chaining)."""
    rec["mass"] = 0.0
    rec["acceleration"] = 0.0
    rec["mass"][k] = mass
    return rec


def probe_reference_aj(pos, vel, k: int, g: float, eps: float, mass: float = PROBE_MASS):
    """(S_a [n, 3], S_j [n, 3], T_j [n]) in np.longdouble: the one term body k sends to every body.  Row k is exactly 0."""
    L = np.longdouble
    p, v = np.asarray(pos, np.float64).astype(L), np.asarray(vel, np.float64).astype(L)
    d, w = p[k] - p, v[k] - v
    d2 = (d * d).sum(1)
    q = d2 + L(eps) * L(eps)
    q[k] = 1
    c = (L(g) * L(mass)) / (q * np.sqrt(q))
    c[k] = 0
    dw = (d * w).sum(1)
    Sa = d * c[:, None]
    Sj = (w - (3 * dw / q)[:, None] * d) * c[:, None]
    Tj = (np.sqrt((w * w).sum(1)) + 3 * np.abs(dw) * np.sqrt(d2) / q) * c
    return Sa, Sj, Tj


def probe_errors_aj(a, j, k: int, ref, rows=None):
    """(|a_i - S_a| / |S_a|, |j_i - S_j| / T_j) per row; `rows` names the bodies the rows of a and j belong to (all, in order,
    if None).  A row with a zero denominator must be exact, a non-finite row is inf, and body k's rows are 0 if they are exactly
    (0, 0, 0), else inf."""
    Sa, Sj, Tj = ref
    rows = np.arange(len(Sa)) if rows is None else np.asarray(rows, np.int64)
    a, j = np.asarray(a, np.float64), np.asarray(j, np.float64)
    assert a.shape == j.shape == (len(rows), 3), f"{a.shape} accelerations, {j.shape} jerks for {len(rows)} rows"
    out = []
    for got, S, den in ((a, Sa[rows], np.sqrt((Sa[rows] ** 2).sum(1))), (j, Sj[rows], Tj[rows])):
        num = np.sqrt(((got.astype(np.longdouble) - S) ** 2).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0, np.inf))
        err = np.asarray(err, np.float64)
        err[~np.isfinite(got).all(1)] = np.inf
        at_k = rows == k
        err[at_k] = np.where(np.isfinite(got[at_k]).all(1) & (got[at_k] == 0).all(1), 0.0, np.inf)
        out.append(err)
    return out[0], out[1]


def check_probe_aj(a, j, pos, vel, k: int, g: float, eps: float, mass: float = PROBE_MASS, rows=None, ref=None, rtol_a: float = PROBE64,
                   rj: float | None = None, what: str = ""):
    """Assert the probe world's accelerations and jerks (`rows`: the bodies they belong to; `ref`: probe_reference_aj of the same
    world and column, if the caller holds it); returns the worst |a - S_a| / |S_a| and the worst |j - S_j| / T_j."""
    rj = RJP if rj is None else rj
    ref = probe_reference_aj(pos, vel, k, g, eps, mass) if ref is None else ref
    ids = np.arange(len(pos)) if rows is None else np.asarray(rows, np.int64)
    ea, ej = probe_errors_aj(a, j, k, ref, ids)
    worst_a = float(ea.max()) if len(ea) else 0.0
    worst_j = float(ej.max()) if len(ej) else 0.0
    for name, err, bound in (("accelerations", ea, rtol_a), ("jerks", ej, rj)):
        if len(err) and not err.max() <= bound:
            bad = np.flatnonzero(~(err <= bound))
            raise AssertionError(f"{what}: probe column k={k} of n={len(pos)} (eps={eps}): {len(bad)} {name} off the bound {bound:g}, "
                                 f"first bodies {ids[bad[:8]].tolist()} with errors {err[bad[:8]].tolist()}")
    return worst_a, worst_j
