"""Per-body bound for the fast f64 brute-force kernels (kernels_bf64.hip), and the probe bound of their exact pair coverage.

For a chosen row i the reference is the direct sum in np.longdouble,
    S_i = sum_{j != i} g m_j r_ij / (|r_ij|^2 + eps^2)^(3/2),       r_ij = x_j - x_i,
and the scale of its rounding is the sum of the terms' magnitudes,
    T_i = sum_{j != i} |g m_j r_ij| / (|r_ij|^2 + eps^2)^(3/2).
The check is |a_i - S_i| <= R T_i.  A fast kernel's a_i is the same terms with a handful of f64 roundings each (rsqrt, the
cube, the product with the mass) added in another order, so its error is a small multiple of 1e-16 T_i; a dropped,
doubled, wrong-sign or wrong-mass pair is an error of one whole term, far above R T_i (tests/test_bf64_checker.py).

PROBE64 is the rtol passed to tests/bf_probe.py's check_probe on its probe worlds built from PARTICLE_DTYPE64 records: one
term per body, to a few f64 roundings.  Probe positions, g, eps and the mass are f32-representable, so bf_probe's f64
reference sees exactly the values the handle holds.

R and PROBE64 are about 3x the worst values measured on an MI355X over tests/test_bf64_fast_gpu.py.

This module is plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

#: |a_i - S_i| <= R T_i
R = 1.0e-14
#: check_probe rtol for the f64 probe worlds
PROBE64 = 4.0e-15


def direct_rows(pos, mass, g: float, eps: float, rows):
    """(S, T) for `rows` of the world (pos [n, 3], mass [n]): S [len(rows), 3] and T [len(rows)] in np.longdouble."""
    p = np.asarray(pos, np.float64).astype(np.longdouble)
    m = np.asarray(mass, np.float64).astype(np.longdouble)
    rows = np.asarray(rows, np.int64)
    n = len(p)
    gl, e2 = np.longdouble(g), np.longdouble(eps) * np.longdouble(eps)
    S = np.zeros((len(rows), 3), np.longdouble)
    T = np.zeros(len(rows), np.longdouble)
    step = max(1, (1 << 20) // max(1, n))
    for c0 in range(0, len(rows), step):
        r = rows[c0:c0 + step]
        d = p[None, :, :] - p[r, None, :]                    # r_ij = x_j - x_i
        d2 = (d * d).sum(-1)
        self_ = np.arange(n)[None, :] == r[:, None]
        r2 = np.where(self_, np.longdouble(1), d2 + e2)
        w = np.where(self_, np.longdouble(0), gl * m[None, :] / (r2 * np.sqrt(r2)))
        S[c0:c0 + step] = (d * w[..., None]).sum(1)
        T[c0:c0 + step] = (np.sqrt(d2) * np.abs(w)).sum(1)
    return S, T


def bound_errors(acc, S, T) -> np.ndarray:
    """Per row |a_i - S_i| / T_i (vector norms; a row with T_i = 0 must equal S_i exactly, else inf)."""
    a64 = np.asarray(acc, np.float64)
    num = np.sqrt(((a64.astype(np.longdouble) - S) ** 2).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(T > 0, num / np.where(T > 0, T, 1), np.where(num == 0, 0, np.inf))
    err = np.asarray(err, np.float64)
    err[~np.isfinite(a64).all(1)] = np.inf
    return err


def check_bound(acc, pos, mass, g, eps, rows=None, r_bound: float = R, what: str = "") -> float:
    """Assert |a_i - S_i| <= R T_i for `rows` (every row if None) of the accelerations `acc` of the world (pos, mass);
    returns the worst |a_i - S_i| / T_i."""
    rows = np.arange(len(pos)) if rows is None else np.asarray(rows, np.int64)
    a_rows = np.asarray(acc, np.float64)[rows]
    S, T = direct_rows(pos, mass, g, eps, rows)
    err = bound_errors(a_rows, S, T)
    worst = float(err.max()) if len(err) else 0.0
    if not worst <= r_bound:
        bad = np.flatnonzero(~(err <= r_bound))
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} rows off the bound R = {r_bound:g}: rows {rows[bad[:8]].tolist()} "
                             f"with |a - S| / T = {err[bad[:8]].tolist()}")
    return worst
