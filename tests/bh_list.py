"""Checking a Barnes-Hut walk against the f64 sum of its own node list.

The fast walks (k_bh_walk, k_bh_walk_duo, k_bh_walk_fast64, with the walk split and the plane reductions) make their
opening tests with the oracle's f32 / f64 expressions, r2 = (rx*rx + ry*ry) + rz*rz, no contraction, w2 < theta2 * r2.
oracle.bh_walk_list replays those tests over the handle's OWN exported tree (Simulation.tree()), so it accepts exactly
the nodes the kernel accepts -- for the host and the device build alike, with no allowance for a flipped test -- and sums
the accepted terms t_ij in high precision: S_i = sum_j t_ij, T_i = sum_j |t_ij|.  The kernel's result differs from S_i by
its accumulation rounding only, which is bounded by a multiple of T_i (not of |a_i|, which cancellation makes small for
central bodies), so one bound holds for every body:

    |a_i - S_i| <= R T_i.

A node that is dropped, counted twice, applied with the wrong mass or taken from the wrong partial-sum plane moves a_i by
at least one term |t_ij|; every term above 2 R T_i is therefore individually detectable (about two thirds of all
(body, node) terms of a Plummer sphere at theta2 = 0.25 and R = LIST_RTOL_F32: tests/test_bh_list_checker.py measures the share).
The far-field rest is below any sum-based check.  The exact accepted / visited totals (stats()) catch what is left of a
wrong walk.

Which cases run (tests/test_bh_walk_list_gpu.py): `SIZES` x `THETA2S` x `G_SOFTS` for both tree builds and both leaf
rules, plus 2^20 at theta2 = 0.25; `KNOB_CASES` for the launch knobs, in which every value of every knob appears at least
once and bh_reduce_split runs at K >= 8 (`knob_coverage` checks the rule on the CPU).

This module is plain test infrastructure (no GPU): the CPU meta-test runs the checker on the oracle.
"""
from __future__ import annotations

import numpy as np

#: |a_i - S_i| <= R T_i for every body.  Worst measured on an MI355X over every case of test_bh_walk_list_gpu.py:
#: f32 fast walks 1.42e-6 (k_bh_walk in one segment, 30 011 bodies; a margin of 3.2x), f64 fast walk 3.15e-15 (a margin of 3.2x)
LIST_RTOL_F32 = 4.5e-6
LIST_RTOL_F64 = 1e-14

SIZES = (1, 2, 3, 9, 64, 65, 1001, 4097, 30011, 65536)
THETA2S = (0.25, 1.0)
G_SOFTS = (0.0, 0.01)
BIG = 1 << 20          # at theta2 = 0.25 only

#: (knobs, n): each knob value at least once; bh_walk_split pins K (k_bh_reduce_split runs at K >= 8 with bh_reduce_split = 1)
KNOB_CASES = (
    (dict(bh_walk_duo=0, bh_walk_split=1), 30011),
    (dict(bh_walk_duo=1, bh_walk_split=2), 30011),
    (dict(bh_walk_duo=2, bh_walk_split=7, bh_walk_order=0), 30011),
    (dict(bh_walk_duo=3, bh_walk_split=16, bh_reduce_split=0), 65536),
    (dict(bh_walk_duo=4, bh_walk_split=16, bh_reduce_split=1, bh_walk_xcd=0), 65536),
    (dict(bh_walk_duo=6, bh_walk_split=64, bh_walk_xcd=1), 65536),
    (dict(bh_walk_duo=8, bh_walk_split=64, bh_walk_order=1, bh_reduce_split=0), 4097),
    (dict(bh_walk_duo=8, bh_walk_split=8, bh_reduce_split=1, bh_walk_xcd=0, bh_walk_order=0), 4097),
    (dict(bh_walk_duo=0, bh_walk_split=16, bh_reduce_split=1), 1001),
    (dict(bh_walk_duo=3, bh_walk_split=7), 65),
)
KNOB_VALUES = dict(bh_walk_duo=(0, 1, 2, 3, 4, 6, 8), bh_walk_split=(1, 2, 7, 16, 64), bh_walk_xcd=(0, 1),
                   bh_walk_order=(0, 1), bh_reduce_split=(0, 1))


def knob_coverage(cases=KNOB_CASES) -> dict:
    """{knob: values that `cases` miss}; also raises if bh_reduce_split never runs at K >= 8 with either value."""
    seen = {k: set() for k in KNOB_VALUES}
    split_big = set()
    for knobs, _ in cases:
        for k, v in knobs.items():
            seen[k].add(v)
        if knobs.get("bh_walk_split", 0) >= 8:
            split_big.add(knobs.get("bh_reduce_split", 1))
    assert split_big == {0, 1}, f"bh_reduce_split at K >= 8: only {sorted(split_big)}"
    return {k: sorted(set(v) - seen[k]) for k, v in KNOB_VALUES.items() if set(v) - seen[k]}


def walk_errors(acc, ref) -> np.ndarray:
    """Per-body |a_i - S_i| / T_i (0 where both sides are exactly 0, inf where T_i = 0 and a_i is not exactly S_i, and
    inf for a non-finite a_i)."""
    a = np.asarray(acc, np.float64)[:, :3]
    num = np.linalg.norm(a - ref["S"], axis=1)
    T = ref["T"]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(T > 0, num / np.where(T > 0, T, 1.0), np.where(num == 0, 0.0, np.inf))
    err[~np.isfinite(a).all(1)] = np.inf
    return err


def check_walk(acc, ref, rtol=LIST_RTOL_F32, what="") -> float:
    """Assert |a_i - S_i| <= rtol T_i for every body; returns the worst ratio."""
    assert len(acc) == len(ref["T"]), f"{what}: {len(acc)} accelerations for {len(ref['T'])} bodies"
    err = walk_errors(acc, ref)
    worst = float(err.max()) if len(err) else 0.0
    if not worst <= rtol:
        bad = np.flatnonzero(~(err <= rtol))
        raise AssertionError(f"{what}: {len(bad)} of {len(err)} bodies beyond {rtol:g} T_i, first {bad[:8].tolist()} at "
                             f"{err[bad[:8]].tolist()}")
    return worst


def check_counts(stats, ref, what=""):
    """The handle's accepted / visited totals equal the reference walk's, exactly."""
    acc, vis = int(ref["accepted"].sum()), int(ref["visited"].sum())
    assert (stats.interactions, stats.node_visits) == (acc, vis), \
        f"{what}: accepted {stats.interactions} visited {stats.node_visits}, the node list gives {acc} and {vis}"


# ---------------------------------------------------------------------------------------------- node-list helpers
def terms(tree, p, nodes, g, g_soft) -> np.ndarray:
    """[len(nodes), 3] f64 terms g m_j (c_j - p) / (|c_j - p|^2 + eps^2)^(3/2) of the given nodes for a body at p, from the
    tree's values with g and eps^2 rounded to the tree's precision (as bh_walk_list sums them)."""
    ft = tree["com_mass"].dtype.type
    cm = tree["com_mass"][np.asarray(nodes, np.int64)].astype(np.float64)
    d = cm[:, :3] - np.asarray(p, ft).astype(np.float64)
    d2 = (d * d).sum(1) + float(ft(ft(g_soft) * ft(g_soft)))
    return d * (float(ft(g)) * cm[:, 3] / (d2 * np.sqrt(d2)))[:, None]


def split_first(n_nodes: int, K: int) -> list:
    """The split points of K segments of a host-listed node range (WalkSplitBuf::list_on_host)."""
    return [n_nodes * k // K for k in range(K + 1)]


def ancestors(skip, target: int) -> list:
    """The ancestors of node `target`, root first (what walk_entry replays for a segment that starts there)."""
    out, j = [], 0
    while j != target:
        out.append(j)
        c = j + 1
        while skip[c] <= target:
            c = skip[c]
        j = c
    return out


def parent(skip, j: int) -> int:
    """The parent of node j > 0."""
    return ancestors(skip, j)[-1]
