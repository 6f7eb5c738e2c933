"""numpy restatement of the fourth-order Hermite integrator (kernels_hermite.hip, include/nbody_hip.h "integrator").

With d = x_j - x_i, w = v_j - v_i, q = |d|^2 + eps^2 the pair sum F(x, v) is
    a_i = g sum_j m_j d / q^(3/2),        j_i = g sum_j m_j [ w - 3 (d.w)/q d ] / q^(3/2).

direct_aj   the reference in np.longdouble: S_a, T_a as tests/bf64_bound.py, S_j, and the scale of the jerk's rounding
            T_j = sum_j g m_j (|w| + 3 |d.w| |d| / q) / q^(3/2), the sum of the terms' magnitudes.  The fast kernels are
            checked with |a - S_a| <= R T_a (bf64_bound.R) and |j - S_j| <= RJ T_j.
strict_aj   the f64, ascending-partner-order restatement of k_hm_strict: bit for bit.
hermite_step  predictor, F, corrector and retain in the kernels' expression order: bit for bit beside a strict handle.

A fast kernel's jerk term carries a handful of f64 roundings (rsqrt, the square and the cube, (d.w), the product with -3,
three FMAs for the shared vector, the mass product), so its error is a small multiple of 1e-16 T_j; a dropped, doubled or
wrong-sign pair is an error of one whole term (tests/test_hermite_checker.py).

This module is plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

from bf64_bound import R  # noqa: F401  (the acceleration's bound, re-exported for the Hermite tests)

#: |j_i - S_j,i| <= RJ T_j,i.  Measured on an MI355X (pytest -s): the worst |j - S_j| / T_j is 6.6e-16 over tests/test_hermite_gpu.py's
#: fast cases (n = 1500, few slices) and 7.3e-16 over tests/test_hermite_block_gpu.py's k_hm_act rows (n = 1500); 3x that would be
#: 2.2e-15.  RJ stays at the looser figure arithmetic gives for any order of summation, which the measurement does not violate:
#: at most 12 roundings of 1.1e-16 in a term, and at most 1499 additions of the same size relative to T_j in a sum of the
#: largest case's 1500 terms: (12 + 1499) * 1.1e-16 = 1.7e-13.  Must stay <= 1e-12; the smallest single
#: term of world(256) is 1.1e-6 T_j.  What catches a wrong pair at the plans a user gets is the probe bound, hermite_probe.RJP.
RJ = 2.0e-13

G, EPS = 1.0, 0.05
BOX = ((0.0, 0.0, 0.0), 64.0)


def world(n: int, seed: int = 7):
    """(pos [n, 3], vel [n, 3], mass [n]) f64: a cold-ish Gaussian cluster with its mass-weighted mean velocity removed."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)) * 0.6
    v = rng.normal(size=(n, 3)) * 0.5
    m = rng.uniform(0.5, 1.5, n) / n
    if n:
        v = v - (m[:, None] * v).sum(0) / m.sum()
    return x, v, m


def direct_aj(pos, vel, mass, g: float, eps: float, rows):
    """(S_a [k, 3], T_a [k], S_j [k, 3], T_j [k]) in np.longdouble for `rows` of the world."""
    L = np.longdouble
    p, v, m = (np.asarray(a, np.float64).astype(L) for a in (pos, vel, mass))
    rows = np.asarray(rows, np.int64)
    n = len(p)
    gl, e2 = L(g), L(eps) * L(eps)
    Sa, Sj = np.zeros((len(rows), 3), L), np.zeros((len(rows), 3), L)
    Ta, Tj = np.zeros(len(rows), L), np.zeros(len(rows), L)
    step = max(1, (1 << 19) // max(1, n))
    for c0 in range(0, len(rows), step):
        r = rows[c0:c0 + step]
        d = p[None, :, :] - p[r, None, :]
        w = v[None, :, :] - v[r, None, :]
        d2 = (d * d).sum(-1)
        dw = (d * w).sum(-1)
        self_ = np.arange(n)[None, :] == r[:, None]
        q = np.where(self_, L(1), d2 + e2)
        k = np.where(self_, L(0), gl * m[None, :] / (q * np.sqrt(q)))
        Sa[c0:c0 + step] = (d * k[..., None]).sum(1)
        Ta[c0:c0 + step] = (np.sqrt(d2) * np.abs(k)).sum(1)
        Sj[c0:c0 + step] = ((w - (3 * dw / q)[..., None] * d) * k[..., None]).sum(1)
        Tj[c0:c0 + step] = ((np.sqrt((w * w).sum(-1)) + 3 * np.abs(dw) * np.sqrt(d2) / q) * np.abs(k)).sum(1)
    return Sa, Ta, Sj, Tj


def strict_aj(pos, vel, mass, g: float, eps: float):
    """(a [n, 3], j [n, 3]) f64 as k_hm_strict forms them: partners in ascending index order, every product and sum rounded
    on its own, in the order include/nbody_hip.h states."""
    x, v, m = (np.ascontiguousarray(a, np.float64) for a in (pos, vel, mass))
    n = len(x)
    a, jk = np.zeros((n, 3)), np.zeros((n, 3))
    g, eps2 = np.float64(g), np.float64(eps) * np.float64(eps)
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        for j in range(n):                       # one partner at a time, for every body at once: ascending order per body
            d = x[j] - x                          # [n, 3]
            dv = v[j] - v
            r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + eps2
            rv = (d[:, 0] * dv[:, 0] + d[:, 1] * dv[:, 1]) + d[:, 2] * dv[:, 2]
            w = (g * m[j]) / (r2 * np.sqrt(r2))
            al = (3.0 * rv) / r2
            live = idx != j
            ta = d * w[:, None]
            tj = (dv - al[:, None] * d) * w[:, None]
            a[live] += ta[live]
            jk[live] += tj[live]
    return a, jk


def coef(dt: float):
    """The step's five coefficients, each rounded once (kernels_hermite.h hermite_coef)."""
    dt = np.float64(dt)
    dt2 = dt * dt
    return dt, dt2 * 0.5, (dt2 * dt) / 6.0, dt * 0.5, dt2 / 12.0


def contains(x, center, width):
    """Bounds::contains (shared.rs:210-212) with Bounds::new's walls: inclusive, a NaN is outside."""
    c = np.asarray(center, np.float64)
    hw = np.float64(width) * 0.5
    lo, hi = c + (-hw), c + hw
    with np.errstate(invalid="ignore"):
        return ((x >= lo) & (x <= hi)).all(1)


def hermite_step(state, dt: float, g: float = G, eps: float = EPS, box=BOX, force=strict_aj):
    """One nbody_step_by of a Hermite handle whose held (a0, j0) are valid.  state = (x, v, a, j, m); returns the next one
    (retained: bodies outside the box after the corrector are dropped, order preserved, survivors keep their a1, j1)."""
    x0, v0, a0, j0, m = state
    dt, c2, c3, h, c12 = coef(dt)
    xp = ((x0 + v0 * dt) + a0 * c2) + j0 * c3
    vp = (v0 + a0 * dt) + j0 * c2
    a1, j1 = force(xp, vp, m, g, eps)
    v1 = (v0 + (a0 + a1) * h) + (j0 - j1) * c12
    x1 = (x0 + (v0 + v1) * h) + (a0 - a1) * c12
    keep = contains(x1, *box)
    return x1[keep], v1[keep], a1[keep], j1[keep], m[keep]


def start(x, v, m, g: float = G, eps: float = EPS, force=strict_aj):
    """The state of a handle whose held derivatives have just been evaluated at (x, v)."""
    a, j = force(x, v, m, g, eps)
    return np.array(x, np.float64), np.array(v, np.float64), a, j, np.array(m, np.float64)


def fast_aj(pos, vel, mass, g: float, eps: float, rows=None):
    """F in vectorised f64 (no fixed order): for the order tests, where only the integrator's truncation error matters.
    `rows`: those bodies' rows only (a large world is evaluated a block of rows at a time: fast_aj_blocked)."""
    x, v, m = (np.asarray(a, np.float64) for a in (pos, vel, mass))
    r = np.arange(len(x)) if rows is None else np.asarray(rows, np.int64)
    d = x[None, :, :] - x[r, None, :]
    w = v[None, :, :] - v[r, None, :]
    q = (d * d).sum(-1) + eps * eps
    self_ = (np.arange(len(r)), r)
    q[self_] = 1.0
    k = g * m[None, :] / (q * np.sqrt(q))
    k[self_] = 0.0
    dw = (d * w).sum(-1)
    return (d * k[..., None]).sum(1), ((w - (3.0 * dw / q)[..., None] * d) * k[..., None]).sum(1)


def fast_aj_blocked(pos, vel, mass, g: float, eps: float, block: int = 256):
    """fast_aj of every row, `block` rows at a time: the same values in a bounded amount of memory."""
    parts = [fast_aj(pos, vel, mass, g, eps, rows=np.arange(r0, min(r0 + block, len(pos)))) for r0 in range(0, len(pos), block)]
    if not parts:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def suggest_dt(acc, jerk, eta: float) -> float:
    """nbody_suggest_dt from the downloaded arrays: eta * min |a| / |j| over bodies with |j| > 0, +inf if there is none."""
    a, j = np.asarray(acc, np.float64), np.asarray(jerk, np.float64)
    na = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    nj = np.sqrt((j[:, 0] * j[:, 0] + j[:, 1] * j[:, 1]) + j[:, 2] * j[:, 2])
    ok = nj > 0
    return float(np.float64(eta) * (na[ok] / nj[ok]).min()) if ok.any() else float("inf")


def records(dtype, x, v, m):
    rec = np.zeros(len(x), dtype)
    rec["position"], rec["velocity"], rec["mass"] = x, v, m
    return rec
