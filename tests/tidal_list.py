"""Checking nbody_tidal_at against the sums over its own node list (TREE) and over all bodies (PAIRS).

`replay_tidal(tree, points, theta2, g_soft)` is tests/field_list.py's `replay` loop -- the field walk's opening tests under the
DIRECT leaf rule, in the tree's precision, at the points rounded to the tree's precision (`rounded`, `eps2_of` are imported from
there; the loop is restated because its term is not a parameter, and tests/test_tidal_list_checker.py holds its counts to
field_list.replay's) -- with the tidal term: per probe, over the accepted nodes j with d = c_j - x, q = |d|^2 + eps^2,

    S6 = sum m_j [3 d_a d_b / q^(5/2) - delta_ab / q^(3/2)]   in the order {xx, xy, xz, yy, yz, zz},
    W  = sum 4 m_j / q^(3/2),   accepted, visited.

`pair_tidal(rec, points, g_soft)` is the same over all bodies with r2 != 0.  Both evaluate and accumulate in np.longdouble
from the stored values (S6 and W are returned in longdouble), so their own rounding (2^-64 per operation where longdouble is the
x87 format) is far below the bound.

The bound, by counting the roundings of the expression the kernels implement (include/nbody_hip.h; u = unit roundoff of the
handle's precision for TREE, 2^-53 for PAIRS; first order in u; every line is one rounding):

    d_c = fl(c_c - x_c)                                      1 u on each component
    r2 = fl(fl(dx dx + dy dy) + dz dz), q = fl(r2 + eps2)    3 u per square, 1 u per add, all terms positive: q within 6 u
    inv = fl(1 / fl(sqrt(q)))                                3 u from q, sqrt 1 u, divide 1 u: 5 u
    st = fl(m inv)                                           6 u
    k = fl(st / q)                                           6 u + 6 u + 1 u = 13 u          of m / q^(3/2)
    k3 = fl(fl(3 k) / q)                                     13 u + 1 u + 6 u + 1 u = 21 u   of 3 m / q^(5/2)
    u_c = fl(d_c k3)                                         21 u + 1 u + 1 u = 23 u
    fl(d_a u_b)                                              23 u + 1 u (d_a) + 1 u = 25 u   of 3 m |d_a d_b| / q^(5/2)
    fl(fl(d_a u_a) - k)                                      one more rounding, of |3 d_a^2 / q - 1| m / q^(3/2) <= 2 m / q^(3/2)

With w = 4 m / q^(3/2), the term's share of W, and d_a^2 <= q, |d_a d_b| <= q / 2:

    a diagonal entry      25 u * 3 m / q^(3/2) + 13 u * m / q^(3/2) + 1 u * 2 m / q^(3/2) = 90 u m / q^(3/2) = 22.5 u w
    an off-diagonal one   25 u * 1.5 m / q^(3/2) = 9.4 u w

The conversion to f64 is exact; the n_i terms are then added in f64 (partial sums stay below W / 2, 2^-53 each) and the sum is
multiplied by g once (2^-53 of |g S6| <= g W / 2).  22.5 for the worst entry, one for the product with g and what second
order adds: C = 24, and per component

    |T_c - g S6_c| <= (24 u + n_i 2^-53) g W        n_i = the probe's accepted nodes (TREE) or the bodies of the world (PAIRS).

No probe is left out: a probe with W = 0 must return exactly 0, and check_tidal takes no mask.  The bound is relative, so it
holds inside the handle's number range only: a finite probe so far away that r2 overflows gets exact zeros from the device,
where the longdouble sums here are tiny and non-zero (tests/test_tidal_gpu.py checks that contract on its own).

Worst observed ratios to the bound on an MI355X (tests/test_tidal_gpu.py, pytest -s): see WORST_OBSERVED.

Plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

from field_list import LD, U32, U64, _ratio, eps2_of, rounded

C_TIDAL = 24.0
#: worst ratio to the bound seen on the device over the cases of tests/test_tidal_gpu.py
WORST_OBSERVED = {"tree_f32": 0.105, "tree_f64": 0.122, "pairs_f32": 0.100, "pairs_f64": 0.117}


def _terms(d, s2, mass):
    """The six entries [m, 6] and the share of W [m] of m terms: d [m, 3], s2 = |d|^2 + eps^2, mass (longdouble)."""
    k = mass / (s2 * np.sqrt(s2))
    k3 = 3 * k / s2
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    six = np.stack([dx * dx * k3 - k, dx * dy * k3, dx * dz * k3, dy * dy * k3 - k, dy * dz * k3, dz * dz * k3 - k], 1)
    return six, 4 * k


def replay_tidal(tree, points, theta2, g_soft, drop=None, wrong_mass=None) -> dict:
    """DIRECT walk of every probe over `tree` (field_list.replay's loop); S6 [n, 6] and W [n] in longdouble, accepted [n],
    visited [n].  Fault planting for the checker's own test, as field_list.replay: drop = (probe, k) leaves out the probe's
    k-th accepted term; wrong_mass = (probe, k) takes it with the mass of the next node in the array."""
    com = np.ascontiguousarray(tree["com_mass"])
    ft = com.dtype.type
    w = np.ascontiguousarray(tree["width"], ft)
    w2 = w * w
    skip = np.ascontiguousarray(tree["skip"], np.int64)
    m = len(w)
    p = rounded(points, ft)
    n = len(p)
    comL, pL = com.astype(LD), p.astype(LD)
    eps2 = LD(eps2_of(ft, g_soft))
    th, near = ft(theta2), ft(1e-10)
    S6, W = np.zeros((n, 6), LD), np.zeros(n, LD)
    acc, vis = np.zeros(n, np.int64), np.zeros(n, np.int64)
    body = np.arange(n)
    i = np.zeros(n, np.int64)
    if m == 0:
        body = body[:0]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while len(body):
            c = com[i]
            q = p[body]
            rx, ry, rz = c[:, 0] - q[:, 0], c[:, 1] - q[:, 1], c[:, 2] - q[:, 2]
            r2 = (rx * rx + ry * ry) + rz * rz
            sk = skip[i]
            vis[body] += 1
            skipped = r2 < near
            take = ~skipped & ((w2[i] < th * r2) | (sk == i + 1))
            if take.any():
                bt, it = body[take], i[take]
                d = comL[it, :3] - pL[bt]
                s2 = (d * d).sum(1) + eps2
                mass = comL[it, 3].copy()
                keep = np.ones(len(bt), bool)
                for fault, kind in ((drop, "drop"), (wrong_mass, "mass")):
                    if fault is not None:
                        hit = np.flatnonzero((bt == fault[0]) & (acc[bt] == fault[1]))
                        if len(hit) and kind == "drop":
                            keep[hit] = False
                        elif len(hit):
                            mass[hit] = comL[min(it[hit[0]] + 1, m - 1), 3]
                six, w4 = _terms(d, s2, np.where(keep, mass, 0))
                S6[bt] += six
                W[bt] += w4
                acc[bt] += 1
            i = np.where(skipped | take, sk, i + 1)
            live = i < m
            if not live.all():
                body, i = body[live], i[live]
    return dict(S6=S6, W=W, accepted=acc, visited=vis)


def pair_tidal(rec, points, g_soft) -> dict:
    """S6, W of every probe over ALL bodies of `rec` with r2 != 0, from the stored coordinates (longdouble); probes rounded to
    the records' precision, eps^2 as field_list.pair_field takes it; accepted = bodies summed per probe."""
    ft = rec["position"].dtype.type
    x = rec["position"].astype(LD)
    m = rec["mass"].astype(LD)
    p = rounded(points, ft).astype(LD)
    eps2 = LD(float(g_soft) ** 2 if ft is np.float64 else float(np.float64(ft(g_soft)) ** 2))
    n, nb = len(p), len(x)
    S6, W = np.zeros((n, 6), LD), np.zeros(n, LD)
    cnt = np.zeros(n, np.int64)
    if nb == 0:
        return dict(S6=S6, W=W, accepted=cnt, visited=cnt)
    step = max(1, (1 << 18) // nb)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(0, n, step):
            d = (x[None, :, :] - p[a:a + step, None, :]).reshape(-1, 3)
            r2 = (d * d).sum(1)
            on = r2 != 0
            six, w4 = _terms(d, np.where(on, r2 + eps2, 1), np.where(on, np.tile(m, len(d) // nb), 0))
            S6[a:a + step] = six.reshape(-1, nb, 6).sum(1)
            W[a:a + step] = w4.reshape(-1, nb).sum(1)
            cnt[a:a + step] = on.reshape(-1, nb).sum(1)
    return dict(S6=S6, W=W, accepted=cnt, visited=cnt)


def bound(ref, g, mode: str, f64: bool, n_bodies: int = 0) -> np.ndarray:
    """(C u + n_i 2^-53) g W per probe, in f64."""
    u = U64 if (f64 or mode == "pairs") else U32
    terms = ref["accepted"] if mode == "tree" else np.full(len(ref["W"]), int(n_bodies))
    return (C_TIDAL * u + terms * U64) * abs(float(g)) * ref["W"].astype(np.float64)


def ratios(t6, ref, g, mode: str, f64: bool, n_bodies: int = 0) -> np.ndarray:
    """Per probe, the worst component's |T_c - g S6_c| / bound; W = 0: 0 for exact zeros, inf otherwise; a non-finite result: inf."""
    t = np.asarray(t6, np.float64).reshape(-1, 6)
    err = np.abs(t.astype(LD) - LD(float(g)) * ref["S6"]).max(1).astype(np.float64)
    err = np.where(ref["W"] == 0, np.abs(t).max(1), err)
    err[~np.isfinite(t).all(1)] = np.inf
    return _ratio(err, bound(ref, g, mode, f64, n_bodies))


def check_tidal(t6, counts, ref, g, mode: str, f64: bool, n_bodies: int = 0, what="") -> float:
    """Counts exact (TREE; PAIRS: (0, 0)), every row of every probe within the bound; returns the worst ratio.  There is no
    way to leave a probe out: the rows must be exactly the reference's probes."""
    n = len(ref["W"])
    want = (int(ref["accepted"].sum()), int(ref["visited"].sum())) if mode == "tree" else (0, 0)
    if counts is not None:
        assert tuple(int(c) for c in counts) == want, f"{what}: counts {tuple(counts)}, expected {want}"
    t = np.asarray(t6, np.float64)
    assert t.shape == (n, 6), f"{what}: results of shape {t.shape} for {n} probes"
    r = ratios(t, ref, g, mode, f64, n_bodies)
    worst = float(r.max()) if n else 0.0
    if not worst <= 1.0:
        bad = np.flatnonzero(~(r <= 1.0))
        raise AssertionError(f"{what}: {len(bad)} of {n} probes beyond the bound, first {bad[:8].tolist()} at {r[bad[:8]].tolist()} x the bound")
    return worst
