"""numpy restatement of a Hermite handle's block individual time steps (include/nbody_hip.h "block steps",
kernels_hermite.hip k_hmb_* / k_hm_act*): one nbody_step_by(dt) as a macro step of T = 2^L ticks, bit for bit beside a strict
handle.  It reuses tests/hermite_ref.py's pieces (world, the shared step, the retain's rule).

strict_rows   F for the listed rows against ALL bodies, partners in ascending index order: k_hm_act_strict bit for bit
fast_rows     the same sums vectorised (no fixed order): for runs where only the scheme matters
macro_step    schedule, per-body predictor, F of the due bodies, corrector with h_i, step criterion, new levels, retain
Handle        what a handle keeps between calls: state, levels and their validity, elapsed and the counters
tight_pair_world   hermite_ref.world with bodies 0 and 1 replaced by a bound pair

A run's `log` collects the block steps, the body updates, the directed pair terms, the smallest relative distance of any
dtc to one of the level thresholds |dt| 2^-k (a fast handle whose dtc differs in its last bits takes the same levels as
long as that distance stays well above those bits), whether every macro step ended with all bodies at T and whether any
step doubled off its grid.

This module is plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

import hermite_ref as hr


def tight_pair_world(n: int, seed: int = 7, sep: float = 0.02, g: float = hr.G):
    """hermite_ref.world(n, seed) with bodies 0 and 1 replaced by a bound pair: separation `sep` along x about body 0's place,
    the Kepler circular speed sqrt(g (m0 + m1) / sep) along y about body 0's velocity, split by the masses."""
    x, v, m = hr.world(n, seed)
    M = m[0] + m[1]
    c, u = x[0].copy(), v[0].copy()
    vrel = np.sqrt(g * M / sep)
    x[0] = c + np.array([sep * m[1] / M, 0.0, 0.0])
    x[1] = c - np.array([sep * m[0] / M, 0.0, 0.0])
    v[0] = u + np.array([0.0, vrel * m[1] / M, 0.0])
    v[1] = u - np.array([0.0, vrel * m[0] / M, 0.0])
    return x, v, m


def strict_rows(xp, vp, m, g: float, eps: float, rows):
    """(a [k, 3], j [k, 3]) f64 of `rows` as k_hm_act_strict forms them: partners j = 0 .. n-1 in ascending order, j != i,
    every product and sum rounded on its own (hermite_ref.strict_aj's expressions)."""
    x, v, m = (np.ascontiguousarray(c, np.float64) for c in (xp, vp, m))
    rows = np.asarray(rows, np.int64)
    xi, vi = x[rows], v[rows]
    a, jk = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    g, eps2 = np.float64(g), np.float64(eps) * np.float64(eps)
    with np.errstate(all="ignore"):
        for j in range(len(x)):
            d = x[j] - xi
            dv = v[j] - vi
            r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + eps2
            rv = (d[:, 0] * dv[:, 0] + d[:, 1] * dv[:, 1]) + d[:, 2] * dv[:, 2]
            w = (g * m[j]) / (r2 * np.sqrt(r2))
            al = (3.0 * rv) / r2
            live = rows != j
            ta = d * w[:, None]
            tj = (dv - al[:, None] * d) * w[:, None]
            a[live] += ta[live]
            jk[live] += tj[live]
    return a, jk


def fast_rows(xp, vp, m, g: float, eps: float, rows):
    """F of `rows` in vectorised f64 (no fixed order)."""
    x, v, m = (np.asarray(c, np.float64) for c in (xp, vp, m))
    rows = np.asarray(rows, np.int64)
    d = x[None, :, :] - x[rows, None, :]
    w = v[None, :, :] - v[rows, None, :]
    q = (d * d).sum(-1) + eps * eps
    self_ = np.arange(len(x))[None, :] == rows[:, None]
    q = np.where(self_, 1.0, q)
    k = np.where(self_, 0.0, g * m[None, :] / (q * np.sqrt(q)))
    dw = (d * w).sum(-1)
    return (d * k[..., None]).sum(1), ((w - (3.0 * dw / q)[..., None] * d) * k[..., None]).sum(1)


def norm3(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def new_log():
    return dict(block_steps=0, updates=0, pair_terms=0, min_gap=np.inf, all_at_T=True, off_grid=0)


def levels_for(dtc, abs_dt, L: int, log=None):
    """l = 0; s = |dt|; while (s > dtc && l < L) { s *= 0.5; ++l; } for every entry: a NaN dtc gives 0, dtc == 0 gives L."""
    dtc = np.asarray(dtc, np.float64)
    lv = np.zeros(len(dtc), np.int64)
    s = np.full(len(dtc), np.float64(abs_dt))
    with np.errstate(invalid="ignore"):
        for k in range(L):
            if log is not None and len(dtc):
                thr = np.ldexp(np.float64(abs_dt), -k)
                gap = np.abs(dtc - thr) / thr
                gap = gap[np.isfinite(gap)]
                if len(gap):
                    log["min_gap"] = min(log["min_gap"], float(gap.min()))
            go = s > dtc
            s = np.where(go, s * 0.5, s)     # (s only shrinks: a lane that stopped stays stopped)
            lv += go
    return lv


def start_levels(a, j, eta: float, abs_dt, L: int, log=None):
    """Start levels from the held derivatives: dtc = eta (|a| / |j|)."""
    with np.errstate(all="ignore"):
        dtc = np.float64(eta) * (norm3(a) / norm3(j))
    return levels_for(dtc, abs_dt, L, log)


def macro_step(state, levels, dt: float, eta: float, L: int, g: float = hr.G, eps: float = hr.EPS, box=hr.BOX, force=strict_rows, log=None):
    """One nbody_step_by(dt != 0) with block steps on, from a state whose held (a0, j0) are valid.  levels: [n] ints, or None
    for start levels.  Returns (state, levels) after the retain."""
    x, v, a, j, m = (np.array(c, np.float64) for c in state)
    n = len(x)
    dt = np.float64(dt)
    adt = np.abs(dt)
    log = new_log() if log is None else log
    lv = start_levels(a, j, eta, adt, L, log) if levels is None else np.array(levels, np.int64)
    T = 1 << L
    tick = np.ldexp(dt, -L)
    tau = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(T):
            if not n or (tau == T).all():
                break
            nxt = tau + (T >> lv)
            ts = int(nxt.min())
            act = np.flatnonzero(nxt == ts)
            dp = ((ts - tau).astype(np.float64) * tick)[:, None]
            c2, c3 = (dp * dp) * 0.5, ((dp * dp) * dp) / 6.0
            xp = ((x + v * dp) + a * c2) + j * c3
            vp = (v + a * dp) + j * c2
            a1, j1 = force(xp, vp, m, g, eps, act)
            la = lv[act]
            h = ((T >> la).astype(np.float64) * tick)[:, None]
            hh, c12 = h * 0.5, (h * h) / 12.0
            x0, v0, a0, j0 = x[act], v[act], a[act], j[act]
            v1 = (v0 + (a0 + a1) * hh) + (j0 - j1) * c12
            x1 = (x0 + (v0 + v1) * hh) + (a0 - a1) * c12
            da = a0 - a1
            h2 = h * h
            h3 = h2 * h
            a3 = (da * 12.0 + (j0 + j1) * (h * 6.0)) / h3
            a2 = ((da * -6.0 - (j0 * 4.0 + j1 * 2.0) * h) / h2) + a3 * h
            na, nj, n2, n3 = norm3(a1), norm3(j1), norm3(a2), norm3(a3)
            dtc = np.sqrt(np.float64(eta) * ((na * n2 + nj * nj) / (nj * n3 + n2 * n2)))
            want = levels_for(dtc, adt, L, log)
            up = want > la
            grid = T >> np.maximum(la - 1, 0)
            down = (want < la) & (la > 0) & (ts % grid == 0)
            nl = np.where(up, want, np.where(down, la - 1, la))
            log["off_grid"] += int(((nl < la) & (ts % (T >> nl) != 0)).sum())
            x[act], v[act], a[act], j[act] = x1, v1, a1, j1
            lv[act] = nl
            tau[act] = ts
            log["block_steps"] += 1
            log["updates"] += len(act)
            log["pair_terms"] += len(act) * (n - 1)
    log["all_at_T"] = log["all_at_T"] and bool((tau == T).all())
    keep = hr.contains(x, *box)
    return (x[keep], v[keep], a[keep], j[keep], m[keep]), lv[keep]


class Handle:
    """What a strict Hermite handle with block steps on does between upload and download: F at the uploaded state before the
    first step (one pass that interactions counts), start levels whenever the levels are invalid or |dt| changes in bits."""

    def __init__(self, x, v, m, eta: float, L: int, g: float = hr.G, eps: float = hr.EPS, box=hr.BOX, force=strict_rows):
        self.eta, self.L, self.g, self.eps, self.box, self.force = eta, L, g, eps, box, force
        self.x, self.v, self.m = (np.array(c, np.float64) for c in (x, v, m))
        self.state = None          # (x, v, a, j, m) once the held derivatives are valid
        self.levels, self.lv_dt = None, None
        self.elapsed, self.steps, self.interactions = 0.0, 0, 0
        self.log = new_log()

    def update_forces(self, dt=None):
        x, v, m = (self.x, self.v, self.m) if self.state is None else (self.state[0], self.state[1], self.state[4])
        n = len(x)
        a, j = self.force(x, v, m, self.g, self.eps, np.arange(n))
        self.state = (x, v, a, j, m)
        self.interactions += n * (n - 1)
        self.levels = None
        if dt is not None:
            self.levels, self.lv_dt = start_levels(a, j, self.eta, abs(np.float64(dt)), self.L, self.log), abs(np.float64(dt))

    def step_by(self, dt: float):
        if self.state is None:
            self.update_forces()
        adt = abs(np.float64(dt))
        if self.levels is not None and self.lv_dt.tobytes() != adt.tobytes():
            self.levels = None
        before = self.log["pair_terms"]
        self.state, self.levels = macro_step(self.state, self.levels, dt, self.eta, self.L, self.g, self.eps, self.box, self.force, self.log)
        self.lv_dt = adt
        self.interactions += self.log["pair_terms"] - before
        self.elapsed += dt
        self.steps += 1


def energy(state, g: float = hr.G, eps: float = hr.EPS) -> float:
    """KE + PE of a state in f64 (softened pair potential, every unordered pair once)."""
    x, v, m = state[0], state[1], state[4]
    ke = 0.5 * float((m * (v * v).sum(1)).sum())
    d = x[None, :, :] - x[:, None, :]
    r = np.sqrt((d * d).sum(-1) + eps * eps)
    iu = np.triu_indices(len(x), 1)
    return ke - g * float((m[:, None] * m[None, :] / r)[iu].sum())
