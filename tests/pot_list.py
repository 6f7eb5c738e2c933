"""Checking nbody_potentials(NBODY_POTENTIAL_TREE) against the f64 sum of its own node list.

The potential walk makes the force walk's opening tests under the DIRECT leaf rule: r2 = (rx*rx + ry*ry) + rz*rz in the
tree's precision with no contraction, a node with r2 < 1e-10 is skipped whole, w2 < theta2 * r2 accepts a cell, a leaf that
fails the test is evaluated all the same.  `replay` walks an exported tree (Simulation.tree() / oracle.bh_build_tree) that
way for all bodies at once in numpy and sums the accepted terms m_j / sqrt(r^2 + eps^2) in f64 from the tree's values:
S_i, plus each body's accepted and visited counts.  The set of (body, node) terms is what
oracle.bh_walk_list(tree, pos, theta2, g, g_soft, leaf_mode=1) accepts (tests/test_pot_list_checker.py holds it to that).

The bound, per body, derived (not measured):

    |phi_i - (-g S_i)| <= R_i |g S_i|,   R_i = 8 u + n_i 2^-53,

u = unit roundoff of the handle's precision (2^-24 or 2^-53), n_i = the body's accepted count.  A coordinate difference is
within u; r2 + eps^2, a sum of positive terms, within about 5 u; sqrt, divide and the mass product bring a term within about
6 u; the terms have one sign, so their sum inherits the term bound, plus at most n_i f64 roundings from the accumulation (and
one for the product with g).

All terms have one sign, so a dropped or doubled term, or one taken with another node's mass, moves phi_i by its full
size: every term above 2 R_i |S_i| is individually detectable -- a share 2 R_i of |phi_i|, i.e. 9.6e-7 (f32 trees) or
(16 + 2 n_i) 1.1e-16 (f64 trees, 2.4e-13 at n_i = 1000).  The exact accepted / visited totals catch what is smaller.

Worst observed |phi_i + g S_i| / (R_i |g S_i|) on an MI355X (tests/test_potentials_gpu.py, pytest -s): see WORST_OBSERVED.

Plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
#: worst ratio to the bound seen on the device over the cases of tests/test_potentials_gpu.py: {precision: ratio}
WORST_OBSERVED = {"f32": 0.344, "f64": 0.194}   # (PAIRS against its own bound (n + 16) 2^-53: 0.058 on f32 handles, 0.086 on f64)


def replay(tree, pos, theta2, g_soft) -> dict:
    """DIRECT walk of every body over `tree`; returns S [n] f64, accepted [n], visited [n] (int64)."""
    com = np.ascontiguousarray(tree["com_mass"])
    ft = com.dtype.type
    w = np.ascontiguousarray(tree["width"], ft)
    w2 = w * w
    skip = np.ascontiguousarray(tree["skip"], np.int64)
    m = len(w)
    p = np.ascontiguousarray(np.asarray(pos).reshape(-1, 3), ft)
    n = len(p)
    com64, p64 = com.astype(np.float64), p.astype(np.float64)
    eps2 = float(ft(ft(g_soft) * ft(g_soft)))
    th = ft(theta2)
    near = ft(1e-10)
    S = np.zeros(n)
    acc = np.zeros(n, np.int64)
    vis = np.zeros(n, np.int64)
    body = np.arange(n)
    i = np.zeros(n, np.int64)
    if m == 0:
        body = body[:0]
    while len(body):
        c = com[i]
        q = p[body]
        rx, ry, rz = c[:, 0] - q[:, 0], c[:, 1] - q[:, 1], c[:, 2] - q[:, 2]
        r2 = (rx * rx + ry * ry) + rz * rz
        sk = skip[i]
        vis[body] += 1
        skipped = r2 < near
        with np.errstate(over="ignore"):
            take = ~skipped & ((w2[i] < th * r2) | (sk == i + 1))
        if take.any():
            d = com64[i[take], :3] - p64[body[take]]
            S[body[take]] += com64[i[take], 3] / np.sqrt((d * d).sum(1) + eps2)
            acc[body[take]] += 1
        i = np.where(skipped | take, sk, i + 1)
        live = i < m
        if not live.all():
            body, i = body[live], i[live]
    return dict(S=S, accepted=acc, visited=vis)


def bound(ref, f64: bool) -> np.ndarray:
    """R_i of the module docstring."""
    return 8.0 * (U64 if f64 else U32) + ref["accepted"] * U64


def ratios(phi, ref, g, f64: bool) -> np.ndarray:
    """|phi_i + g S_i| / (R_i |g S_i|) per body (0 where both sides are exactly 0, inf where S_i = 0 and phi_i is not, or phi_i is not finite)."""
    phi = np.asarray(phi, np.float64)
    want = -float(g) * ref["S"]
    num = np.abs(phi - want)
    den = bound(ref, f64) * np.abs(want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    r[~np.isfinite(phi)] = np.inf
    return r


def check_potentials(phi, counts, ref, g, f64: bool, what="") -> float:
    """Counts exact, every body within its bound; returns the worst ratio to the bound."""
    assert len(phi) == len(ref["S"]), f"{what}: {len(phi)} potentials for {len(ref['S'])} bodies"
    want = (int(ref["accepted"].sum()), int(ref["visited"].sum()))
    assert tuple(int(c) for c in counts) == want, f"{what}: counts {tuple(counts)}, the node list gives {want}"
    r = ratios(phi, ref, g, f64)
    worst = float(r.max()) if len(r) else 0.0
    if not worst <= 1.0:
        bad = np.flatnonzero(~(r <= 1.0))
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} bodies beyond R_i |g S_i|, first {bad[:8].tolist()} at {r[bad[:8]].tolist()} x the bound")
    return worst


def pair_sums(rec, g_soft) -> np.ndarray:
    """S_i = sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + g_soft^2) in f64 from the records' stored coordinates, all bodies (O(n^2) memory in rows of 512)."""
    return pair_sums_rows(rec, g_soft, np.arange(len(rec)))


def pair_sums_rows(rec, g_soft, rows) -> np.ndarray:
    x = rec["position"].astype(np.float64)
    m = rec["mass"].astype(np.float64)
    ft = rec["position"].dtype.type
    eps2 = float(g_soft) ** 2 if ft is np.float64 else float(np.float64(ft(g_soft)) ** 2)
    out = np.zeros(len(rows))
    for a in range(0, len(rows), 512):
        idx = np.asarray(rows[a:a + 512])
        d = x[None, :, :] - x[idx, None, :]
        inv = 1.0 / np.sqrt((d * d).sum(2) + eps2)
        inv[np.arange(len(idx)), idx] = 0.0
        out[a:a + 512] = (inv * m[None, :]).sum(1)
    return out
