"""Checking nbody_field_at against the sums over its own node list (TREE) and over all bodies (PAIRS).

`replay(tree, points, theta2, g_soft)` is tests/pot_list.py's loop -- the potential walk's opening tests under the DIRECT leaf
rule, in the tree's precision, at the points rounded to the tree's precision -- extended to return, per probe,

    S = sum m_j / s_j,   A = sum m_j d_j / s_j^3 [3],   T = sum m_j |d_j| / s_j^3,   accepted, visited,

d_j = c_j - x, s_j^2 = |d_j|^2 + eps^2, over the accepted nodes; `pair_field(rec, points, g_soft)` is the same over all bodies
with r2 != 0.  Both evaluate and accumulate in np.longdouble from the stored values, so their own rounding (2^-64 per
operation where longdouble is the x87 format) is far below every bound here.

The bounds, derived by counting the roundings of the expressions the kernels implement (u = unit roundoff of the handle's
precision for TREE, 2^-53 for PAIRS; first order in u):

    d_c = fl(c_c - x_c)                                         1 u on each component
    r2 = fl(fl(dx dx + dy dy) + dz dz), q = fl(r2 + eps2)       3 u per square, 1 u per add: q within 6 u (positive terms)
    inv = fl(1 / fl(sqrt(q)))                                   3 u from q, sqrt 1 u, divide 1 u: 5 u
    scalar term  st = fl(m inv)                                 6 u
    k = fl(st / q)                                              6 u + 6 u + 1 u = 13 u
    vector term  fl(d_c k)                                      13 u + 1 u (d_c) + 1 u = 15 u of |d_c| m / s^3 <= m |d| / s^3

(The form d (m inv inv inv) would carry 3 x 5 u from inv and four products, 20 u with d: beyond the cap of 16, hence the divide.)
The terms are then added in f64, n_i additions, and multiplied by g once:

    TREE   |phi + g S|   <= (8 u + n_i 2^-53) |g S|          pot_list's bound as it stands (6 u per term derived above)
    TREE   |acc_c - g A_c| <= (16 u + n_i 2^-53) g T         c = 16: the 15 u of a term, and one for the product with g and second order
    PAIRS  |phi + g S|   <= (n + 16) 2^-53 |g S|             n = bodies of the world
    PAIRS  |acc_c - g A_c| <= (n + 17) 2^-53 g T             c' = 17: 15 per term, the product with g, one for second order

No probe is left out: a probe with T = 0 (S = 0) must return exactly 0.  The bounds are relative, so they hold inside the
handle's number range only: a finite probe so far away that r2 overflows (beyond ~1e19 from the bodies on an f32 handle) gets
inv = 1 / inf = 0 and exact zeros from the device, where the longdouble sums here are tiny and non-zero.

Worst observed ratios to these bounds on an MI355X (tests/test_field_gpu.py, pytest -s): see WORST_OBSERVED.

Plain test infrastructure (no GPU).
"""
from __future__ import annotations

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
C_TREE_PHI, C_TREE_ACC, C_PAIRS_PHI, C_PAIRS_ACC = 8.0, 16.0, 16.0, 17.0
LD = np.longdouble
#: worst ratio to the bound seen on the device over the cases of tests/test_field_gpu.py
WORST_OBSERVED = {"tree_phi_f32": 0.413, "tree_acc_f32": 0.432, "tree_phi_f64": 0.420, "tree_acc_f64": 0.372, "pairs_phi": 0.215, "pairs_acc": 0.243}


def rounded(points, ft) -> np.ndarray:
    """The probes as a handle of float type `ft` sees them: each coordinate rounded to the nearest `ft` once."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3).astype(ft))


def eps2_of(ft, g_soft) -> float:
    return float(ft(ft(g_soft) * ft(g_soft)))


def replay(tree, points, theta2, g_soft, drop=None, wrong_mass=None) -> dict:
    """DIRECT walk of every probe over `tree`; S [n], A [n, 3], T [n] (f64, accumulated in longdouble), accepted [n], visited [n].
    Fault planting for the checker's own test: drop = (probe, k) leaves out the probe's k-th accepted term; wrong_mass =
    (probe, k) takes it with the mass of the next node in the array."""
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
    S, A, T = np.zeros(n, LD), np.zeros((n, 3), LD), np.zeros(n, LD)
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
                k3 = np.where(keep, mass / (s2 * np.sqrt(s2)), 0)
                S[bt] += np.where(keep, mass / np.sqrt(s2), 0)
                A[bt] += d * k3[:, None]
                T[bt] += np.sqrt((d * d).sum(1)) * k3
                acc[bt] += 1
            i = np.where(skipped | take, sk, i + 1)
            live = i < m
            if not live.all():
                body, i = body[live], i[live]
    return dict(S=S.astype(np.float64), A=A.astype(np.float64), T=T.astype(np.float64), accepted=acc, visited=vis)


def pair_field(rec, points, g_soft) -> dict:
    """S, A, T of every probe over ALL bodies of `rec` with r2 != 0, from the stored coordinates (longdouble); probes rounded
    to the records' precision; accepted = bodies summed per probe."""
    ft = rec["position"].dtype.type
    x = rec["position"].astype(LD)
    m = rec["mass"].astype(LD)
    p = rounded(points, ft).astype(LD)
    eps2 = LD(float(g_soft) ** 2 if ft is np.float64 else float(np.float64(ft(g_soft)) ** 2))
    n = len(p)
    S, A, T = np.zeros(n, LD), np.zeros((n, 3), LD), np.zeros(n, LD)
    cnt = np.zeros(n, np.int64)
    step = max(1, (1 << 20) // max(len(x), 1))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(0, n, step):
            d = x[None, :, :] - p[a:a + step, None, :]
            r2 = (d * d).sum(2)
            s2 = r2 + eps2
            on = r2 != 0
            k3 = np.where(on, m[None, :] / (s2 * np.sqrt(s2)), 0)
            S[a:a + step] = np.where(on, m[None, :] / np.sqrt(s2), 0).sum(1)
            A[a:a + step] = (d * k3[:, :, None]).sum(1)
            T[a:a + step] = (np.sqrt(r2) * k3).sum(1)
            cnt[a:a + step] = on.sum(1)
    return dict(S=S.astype(np.float64), A=A.astype(np.float64), T=T.astype(np.float64), accepted=cnt, visited=cnt)


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    r[~np.isfinite(num)] = np.inf
    return r


def ratios(acc, phi, ref, g, mode: str, f64: bool, n_bodies: int = 0):
    """(per-probe worst component |acc_c - g A_c| / bound, |phi + g S| / bound); either input may be None (-> None)."""
    g = float(g)
    if mode == "tree":
        u = U64 if f64 else U32
        rp = C_TREE_PHI * u + ref["accepted"] * U64
        ra = C_TREE_ACC * u + ref["accepted"] * U64
    else:
        rp = np.full(len(ref["S"]), (n_bodies + C_PAIRS_PHI) * U64)
        ra = np.full(len(ref["S"]), (n_bodies + C_PAIRS_ACC) * U64)
    out_a = out_p = None
    if acc is not None:
        a = np.asarray(acc, np.float64).reshape(-1, 3)
        out_a = _ratio(np.abs(a - g * ref["A"]).max(1), ra * abs(g) * ref["T"])
    if phi is not None:
        ph = np.asarray(phi, np.float64)
        out_p = _ratio(np.abs(ph + g * ref["S"]), rp * np.abs(g * ref["S"]))
    return out_a, out_p


def check_field(acc, phi, counts, ref, g, mode: str, f64: bool, n_bodies: int = 0, what="") -> tuple:
    """Counts exact (TREE; PAIRS: (0, 0)), every probe within both bounds; returns the worst ratios (acc, phi)."""
    n = len(ref["S"])
    want = (int(ref["accepted"].sum()), int(ref["visited"].sum())) if mode == "tree" else (0, 0)
    if counts is not None:
        assert tuple(int(c) for c in counts) == want, f"{what}: counts {tuple(counts)}, expected {want}"
    ra, rp = ratios(acc, phi, ref, g, mode, f64, n_bodies)
    worst = []
    for name, r, got in (("acc", ra, acc), ("phi", rp, phi)):
        if r is None:
            worst.append(0.0)
            continue
        assert len(r) == n and len(got) == n, f"{what}: {len(got)} {name} results for {n} probes"
        w = float(r.max()) if n else 0.0
        if not w <= 1.0:
            bad = np.flatnonzero(~(r <= 1.0))
            raise AssertionError(f"{what}: {name} of {len(bad)} of {n} probes beyond the bound, first {bad[:8].tolist()} at {r[bad[:8]].tolist()} x the bound")
        worst.append(w)
    return tuple(worst)
