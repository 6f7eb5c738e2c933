"""Probe worlds for the brute-force kernels: every mass is 0 except body k's.

Each body i != k then receives exactly one non-zero term, g m_k (x_k - x_i) / (|x_k - x_i|^2 + eps^2)^(3/2), and body k
receives exactly nothing (its partners are massless; its self pair is excluded, which eps = 0 checks: the self pair
would give 0 * inf).  Massless bodies still receive forces, as in the reference loop (brute_force.rs:64-82).  A fast
kernel's result for body i is that one term with about ten f32 roundings and one v_rsq_f32, so a per-body bound of a
few 1e-6 is enough, while a dropped, doubled, wrong-side or wrong-mass pair is an O(1) error.  A full N-body sum
cannot see that: one pair is ~1/N of a body's acceleration, below the 1e-4 per-body tolerance above ~10 000 bodies.

Probing column k checks every pair (i, k) in the direction k -> i.  Columns are chosen by `probe_columns`:
  * below `every_below` bodies: every body;
  * otherwise, in each index block [lo, hi) (the whole world, or every shard's block): lo, lo+1, lo+63, lo+64, hi-2,
    hi-1; b-1 and b at every multiple b of each resident-set size (bodies counted from lo); the first and last body
    of the block's last set of each size; any extra block-relative offsets given (the cross-shard split); and
    `n_random` bodies drawn with a fixed seed.
Both ends of a set boundary are probed, so the pairs across it are checked in both directions.

This module is plain test infrastructure (no GPU): the CPU meta-test runs the checker on the oracle.
"""
from __future__ import annotations

import numpy as np

PROBE_G = 1.25
PROBE_MASS = 0.75
#: |a_i - a_ref_i| <= PROBE_RTOL |a_ref_i| for every body i != k; the worst seen on an MI355X over every form of
#: test_bf_pair_coverage_gpu.py is 5.9e-7 (a margin of 4x)
PROBE_RTOL = 2.5e-6


def probe_records(dtype, pos: np.ndarray) -> np.ndarray:
    """Records at `pos` ([n, 3]) with zero velocity, acceleration and mass."""
    rec = np.zeros(len(pos), dtype=dtype)
    rec["position"] = pos
    return rec


def set_probe(rec: np.ndarray, k: int, mass: float = PROBE_MASS) -> np.ndarray:
    """The same records with every mass 0 except body k's (in place; returned for chaining)."""
    rec["mass"] = 0.0
    rec["velocity"] = 0.0
    rec["acceleration"] = 0.0
    rec["mass"][k] = mass
    return rec


def probe_reference(pos: np.ndarray, k: int, g: float, eps: float, mass: float = PROBE_MASS) -> np.ndarray:
    """f64 accelerations of the probe world from the f32 positions, with g, eps and the mass rounded to f32 first (as
    the handle stores them).  Row k is exactly 0."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    g64, e64, m64 = (float(np.float32(v)) for v in (g, eps, mass))
    d = p[k] - p
    r2 = (d * d).sum(1) + e64 * e64
    r2[k] = 1.0
    a = (g64 * m64) * d / (r2 * np.sqrt(r2))[:, None]
    a[k] = 0.0
    return a


def probe_errors(acc: np.ndarray, pos: np.ndarray, k: int, g: float, eps: float, mass: float = PROBE_MASS) -> np.ndarray:
    """Per-body |a - a_ref| / |a_ref| (body k: 0 if its acceleration is exactly (0, 0, 0), else inf)."""
    acc = np.asarray(acc, np.float64)
    ref = probe_reference(pos, k, g, eps, mass)
    num = np.linalg.norm(acc - ref, axis=1)
    den = np.linalg.norm(ref, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    err[~np.isfinite(acc).all(1)] = np.inf
    err[k] = 0.0 if (np.isfinite(acc[k]).all() and (acc[k] == 0).all()) else np.inf
    return err


def check_probe(acc, pos, k, g, eps, mass=PROBE_MASS, rtol=PROBE_RTOL, what="") -> float:
    """Assert the probe world's accelerations; returns the worst per-body relative error."""
    assert len(acc) == len(pos), f"{what}: {len(acc)} accelerations for {len(pos)} bodies"
    err = probe_errors(acc, pos, k, g, eps, mass)
    worst = float(err.max()) if len(err) else 0.0
    if not worst <= rtol:
        bad = np.flatnonzero(~(err <= rtol))
        raise AssertionError(f"{what}: probe column k={k} of n={len(pos)} (eps={eps}): {len(bad)} bodies off, "
                             f"first {bad[:8].tolist()} with relative errors {err[bad[:8]].tolist()}")
    return worst


def probe_columns(n: int, blocks=None, set_sizes=(), offsets=(), n_random: int = 24, seed: int = 0,
                  every_below: int = 1100) -> list:
    """The probe columns of an n-body world (rule in the module docstring), sorted."""
    if n <= every_below:
        return list(range(n))
    cols = set()
    for lo, hi in (blocks if blocks is not None else [(0, n)]):
        if hi <= lo:
            continue
        cols.update(c for c in (lo, lo + 1, lo + 63, lo + 64, hi - 2, hi - 1) if lo <= c < hi)
        m = hi - lo
        for s in set_sizes:
            for b in range(s, m, s):
                cols.update((lo + b - 1, lo + b))
            last = (m - 1) // s * s
            cols.update((lo + last, hi - 1))
        for o in offsets:
            cols.update(c for c in (lo + o - 1, lo + o) if lo <= c < hi)
    rng = np.random.default_rng(seed if seed else n)
    cols.update(int(c) for c in rng.choice(n, size=min(n, n_random), replace=False))
    return sorted(cols)
