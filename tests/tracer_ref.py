"""References for the tracer tests (no GPU): tracers are massless particles in the bodies' field (include/nbody_hip.h).

Strict brute force.  A tracer gets the bits of a zero-mass body appended after the bodies: in the reference's loop
(brute_force.rs:64-82) such a body meets the bodies in ascending order, then the other appended bodies, whose terms are
(r f) * 0 = +-0 and change nothing as long as f is finite (no two tracers coincide).  `with_zero_mass` builds that world for
the oracle, `split_back` separates it again, `strict_tracer_acc` restates the per-tracer loop in numpy f32.

Fast brute force.  `pair_sums` gives, per tracer, S = sum_j m_j d_j / q_j^(3/2) (d_j = x_j - x_t, q_j = |d_j|^2 + eps^2) and
T = sum_j |m_j| |d_j| / q_j^(3/2) per component in longdouble from the stored f32 values.  The bound on a fast result a is

    |a_c - g S_c| <= (16 + n) u g T_c,    u = 2^-24,  n = number of bodies,

from counting roundings, the way tests/field_list.py does (u per rounding to nearest):
  * d_c = x_j - x_t: one rounding, u;  the squares inside the FMA chain are not rounded, so each d_c^2 carries 2 u;
  * r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, eps2))): three roundings of sums of non-negative terms, 3 u -> r2 within 5 u;
  * rinv = v_rsq_f32(r2): half of r2's error, 2.5 u, plus the instruction's own error of one unit in the last place (between
    u and 2 u relative) -> at most 4.5 u;
  * sc = (m rinv) (rinv rinv): three factors rinv, 13.5 u, and three rounded products -> 16.5 u;  times d_c (u) inside the
    FMA -> a term within 17.5 u if every rounding and the rsq's 2 u went the same way.  The bound's 16 u per term is the
    figure the feature was specified with, NOT this strict worst case: it is what the count gives with the rsq at one u, and
    it holds because the per-term roundings do not all align (the observed worst is a small fraction of it);
  * the n FMAs into a sum (over K slices and then K planes: n + K - 1 roundings, each of a partial sum no larger than T) and
    the final g * sum add about n u T.
The figure is a count, not a fit: the roundings are independent, so observed errors are a small fraction of it (see
WORST_OBSERVED), while a dropped or doubled pair is an error of a whole term, ~2^24 / (16 + n) times the bound's per-term
share.  T_c == 0 means the result must be exactly 0.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24

#: the largest |a_c - g S_c| / ((16 + n) u g T_c) seen on an MI355X over tests/test_tracers_gpu.py::test_fast_full_sums
#: (printed by the test under -s): at (3, 2^19), where the per-term share of the bound dominates
WORST_OBSERVED = 0.479


def with_zero_mass(bodies: np.ndarray, tracers: np.ndarray) -> np.ndarray:
    """The bodies followed by the tracers as records of mass 0 (every body must have mass > 0 for split_back)."""
    assert (bodies["mass"] > 0).all()
    t = tracers.astype(bodies.dtype).copy()
    t["mass"] = 0
    return np.concatenate([bodies, t])


def split_back(world: np.ndarray):
    """(bodies, tracers) of a world built by with_zero_mass, each in its order."""
    is_tracer = world["mass"] == 0
    return world[~is_tracer], world[is_tracer]


def strict_tracer_acc(bodies: np.ndarray, tracer_pos: np.ndarray, g: float, g_soft: float) -> np.ndarray:
    """The strict tracer pass in numpy f32: a = 0, then for bodies j ascending r = p_t - p_j,
    d = sqrt((rx rx + ry ry) + rz rz + eps2), f = g / ((d d) d), a_c -= (r_c f) m_j; every operation rounded on its own."""
    f32 = np.float32
    pt = np.asarray(tracer_pos, f32)
    pb = np.asarray(bodies["position"], f32)
    mb = np.asarray(bodies["mass"], f32)
    g, eps = f32(g), f32(g_soft)
    eps2 = f32(eps * eps)
    a = np.zeros((len(pt), 3), f32)
    with np.errstate(all="ignore"):
        for j in range(len(pb)):
            r = (pt - pb[j]).astype(f32)
            d = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(f32) + r[:, 2] * r[:, 2]).astype(f32) + eps2).astype(f32)
            f = (g / ((d * d).astype(f32) * d).astype(f32)).astype(f32)
            a -= ((r * f[:, None]).astype(f32) * mb[j]).astype(f32)
    return a


def pair_sums(bodies: np.ndarray, tracer_pos: np.ndarray, g: float, g_soft: float):
    """(S [m, 3], T [m, 3]) in longdouble from the stored f32 values; a body at zero distance with g_soft == 0 is not allowed."""
    ld = np.longdouble
    pt = np.asarray(tracer_pos, np.float32).astype(ld)
    pb = np.asarray(bodies["position"], np.float32).astype(ld)
    mb = np.asarray(bodies["mass"], np.float32).astype(ld)
    eps = ld(np.float32(g_soft))
    S = np.zeros((len(pt), 3), ld)
    T = np.zeros((len(pt), 3), ld)
    step = max(1, 4_000_000 // max(1, len(pb)))
    for lo in range(0, len(pt), step):
        d = pb[None, :, :] - pt[lo:lo + step, None, :]
        q = (d * d).sum(2) + eps * eps
        w = mb[None, :] / (q * np.sqrt(q))
        S[lo:lo + step] = (d * w[:, :, None]).sum(1)
        T[lo:lo + step] = (np.abs(d) * np.abs(w)[:, :, None]).sum(1)
    return S, T


def fast_bound(T: np.ndarray, n_bodies: int, g: float) -> np.ndarray:
    """(16 + n) u g T, per tracer and component."""
    return (16 + n_bodies) * U32 * abs(float(np.float32(g))) * np.asarray(T, np.longdouble)


def fast_ratio(acc: np.ndarray, S: np.ndarray, T: np.ndarray, n_bodies: int, g: float) -> np.ndarray:
    """Per tracer and component |a - g S| / bound; where the bound is 0 (T == 0): 0 if a is exactly 0, else inf.  A non-finite
    result is inf."""
    acc = np.asarray(acc, np.float32)
    a = acc.astype(np.longdouble)
    g_ = np.longdouble(np.float32(g))
    bound = fast_bound(T, n_bodies, g)
    err = np.abs(a - g_ * S)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(acc == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(acc), ratio, np.inf)
    return ratio.astype(np.float64)


def check_fast(acc, S, T, n_bodies, g, what="") -> float:
    """Assert every tracer within the bound (none left out); returns the worst ratio."""
    assert len(acc) == len(S), f"{what}: {len(acc)} accelerations for {len(S)} tracers"
    ratio = fast_ratio(acc, S, T, n_bodies, g)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        bad = np.flatnonzero(~(ratio <= 1.0).all(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(S)} tracers outside (16 + {n_bodies}) u g T, first {bad[:8].tolist()} "
                             f"with ratios {ratio[bad[:8]].max(1).tolist()}")
    return worst
