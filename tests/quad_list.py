"""Checking the quadrupole Barnes-Hut walk (nbody_set_multipole(h, 2)) against the f64 sum of its own node list.

The contract (include/nbody_hip.h), restated in numpy:

  * the quadrupole of a node, about its stored f32 centre of mass c, over the leaves l of its subtree -- the pre-order
    range (i, skip[i]) of the node array itself:  Q = sum_l m_l (3 d_l d_l^T - |d_l|^2 I),  d_l = c_l - c;  a leaf has Q = 0;
  * the term of an accepted internal node, with d = c - x, q = |d|^2 + g_soft^2, inv = 1 / sqrt(q):
        a += g [ M inv^3 d  -  inv^5 (Q d)  +  2.5 inv^7 (d^T Q d) d ];
    an accepted leaf contributes its monopole part alone;
  * the opening tests are the monopole walk's, in float32 exactly as tests/bh_list.py describes them.

`node_quadrupoles` gives the tensors in f64 (and A_i = sum_l m_l |d_l|^2, the scale their rounding is judged against:
|Q_ab| <= 2 A).  `walk_list_quad` replays the walk over an exported tree for many bodies at once and sums the terms in f64
from the f32 tensors it is GIVEN -- the device's own export in the GPU tests, so that the tensors' rounding (bound Rq A_i
per node) and the walk's (|a_i - S_i| <= R T_i per body, T_i = the sum of the magnitudes of the monopole and the two
quadrupole parts of every accepted term) are judged separately.

This module is plain test infrastructure (no GPU); tests/test_quad_list_checker.py checks it on the CPU.
"""
from __future__ import annotations

import numpy as np

#: |a_i - S_i| <= QUAD_RTOL T_i for every body.  NOT MEASURED on an MI355X yet (no GPU time was to be had when this was written):
#: derived instead.  LIST_RTOL_F32 = 4.5e-6 (tests/bh_list.py: 1.42e-6 measured, 3.2x margin) bounds a monopole walk: about 8
#: float32 roundings per term (difference, r2, v_rsq_f32, cube, products) and the running sums.  A quadrupole term takes about
#: ten more roundings (u = d inv, Q u, u^T Q u, the two coefficients, three FMAs per component) on parts whose magnitudes T
#: counts one by one, so a term's error at most doubles relative to its share of T: twice the monopole bound.  The issue's own
#: yardstick: a worst case above a few 1e-5 is a wrong term, not rounding.
QUAD_RTOL = 9e-6
#: |Q_device - Q_f64| <= QUAD_TENSOR_RTOL A_i per node and component.  NOT MEASURED either; derived: the device sums in f64
#: from exact differences and rounds once to float32, a component obeys |Q_ab| <= 2 A_i (Q_aa in [-A, 2 A], |Q_ab| <= 1.5 A),
#: so the error is at most 2^-24 * 2 A_i = 1.19e-7 A_i, plus f64 summation noise of ~1e-13 A_i.
QUAD_TENSOR_RTOL = 1.3e-7
#: GPU median error / CPU f64 median error on the accuracy case (n = 4097, theta2 = 1, g_soft = 0).  NOT MEASURED; derived: the
#: device result is within QUAD_RTOL T_i of the f64 list sum and T_i / |a_i| is a few units for the median body, so f32 rounding
#: moves a body's error of ~9e-3 |a| by < 1e-4 |a|, a ratio within 1.01; 1.05 leaves room for five times that (the cap is 1.25).
ACCURACY_MARGIN = 1.05

#: f64 walks (walk_list_quad; order 1 = the same with zero tensors) over the host-built tree of plummer_bodies(nb, 4097, seed=4097),
#: NBODY_LEAF_DIRECT, g_soft = 0, against the f64 direct sum: (median, 99th percentile) of |a - a_exact| / |a_exact|.
#: Measured 2026-10-17 by tests/test_quad_list_checker.py::test_f64_error_distributions, which recomputes and compares them.
F64_ERRORS = {
    # (order, theta2): (median, p99)
    (1, 0.25): (2.1847e-03, 1.4783e-02),
    (2, 0.25): (6.1675e-04, 3.2113e-03),
    (1, 1.0): (1.4252e-02, 1.1751e-01),
    (2, 1.0): (8.9782e-03, 6.6270e-02),
}
ACCURACY_N = 4097     # plummer_bodies(nb, ACCURACY_N, seed=ACCURACY_N)


def node_quadrupoles(com_mass, skip):
    """(Q6 [n, 6] f64 {xx, xy, xz, yy, yz, zz}, A [n] f64) of every node of a pre-order array, bottom-up: a node's full second
    moment N = sum m d d^T, first moment D = sum m d and leaf mass M about its own centre follow from its children's by the
    parallel-axis shift d -> d + delta, delta = c_child - c (exact algebra; every quantity is local to the cell, so nothing
    cancels); Q = 3 N - tr(N) I and A = tr(N)."""
    cm = np.asarray(com_mass, np.float64).reshape(-1, 4)
    skip = np.asarray(skip, np.int64)
    n = len(skip)
    N = np.zeros((n, 3, 3))
    D = np.zeros((n, 3))
    M = np.zeros(n)
    for i in range(n - 1, -1, -1):
        if skip[i] == i + 1:
            M[i] = cm[i, 3]
            continue
        j = i + 1
        while j < skip[i]:   # the children, in orthant order
            delta = cm[j, :3] - cm[i, :3]
            N[i] += N[j] + np.outer(D[j], delta) + np.outer(delta, D[j]) + M[j] * np.outer(delta, delta)
            D[i] += D[j] + M[j] * delta
            M[i] += M[j]
            j = skip[j]
    A = np.trace(N, axis1=1, axis2=2)
    Q = 3.0 * N - A[:, None, None] * np.eye(3)
    return np.stack([Q[:, 0, 0], Q[:, 0, 1], Q[:, 0, 2], Q[:, 1, 1], Q[:, 1, 2], Q[:, 2, 2]], axis=1), A


def q_matrix(q6):
    """[n, 3, 3] symmetric tensors from [n, 6] {xx, xy, xz, yy, yz, zz}."""
    q = np.asarray(q6, np.float64).reshape(-1, 6)
    return np.stack([q[:, [0, 1, 2]], q[:, [1, 3, 4]], q[:, [2, 4, 5]]], axis=1)


def plummer_bodies(nb, n, seed):
    """n Plummer records, all within 30 of the origin (well inside a box of width 64)."""
    rec = nb.plummer(2 * n + 64, seed=seed)
    rec = rec[np.abs(rec["position"]).max(1) < 30.0][:n]
    assert len(rec) == n
    return np.ascontiguousarray(rec)


def node_terms(cm_j, Q_j, internal, p, g, eps2, c2=2.5):
    """The three parts of node j's term for bodies at p [k, 3] (f64): monopole, -inv^5 Q d, 2.5 inv^7 (d^T Q d) d; the
    quadrupole parts are zero unless `internal`.  c2: the factor 2.5 (another value: a deliberately wrong walk)."""
    d = cm_j[:3] - p
    q = (d * d).sum(1) + eps2
    inv = 1.0 / np.sqrt(q)
    mono = d * (g * cm_j[3] * inv ** 3)[:, None]
    if not internal:
        return mono, np.zeros_like(mono), np.zeros_like(mono)
    Qd = d @ Q_j   # (Q symmetric)
    t1 = -g * Qd * (inv ** 5)[:, None]
    t2 = d * (c2 * g * (d * Qd).sum(1) * inv ** 7)[:, None]
    return mono, t1, t2


def walk_list_quad(points, tree, q6, g, g_soft, theta2, leaf, c2=2.5):
    """The quadrupole walk's decisions and f64 sums over an exported tree (com_mass [m, 4] f32, width [m] f32, skip [m]) for
    bodies at `points` [n, 3]; q6 [m, 6] = the tensors to use (as given: float32 from the device's export); leaf = 0 the
    reference rule, 1 NBODY_LEAF_DIRECT.  All bodies advance together: node i is handled for the bodies whose next node it
    is.  Returns dict(S [n, 3], T [n], accepted [n], visited [n], takers [m] = bodies that accepted each node)."""
    f32 = np.float32
    com = np.ascontiguousarray(tree["com_mass"], f32)
    w = np.ascontiguousarray(tree["width"], f32)
    w2 = w * w                                   # the node record's w^2 (float32 product)
    skip = np.asarray(tree["skip"], np.int64)
    p32 = np.ascontiguousarray(np.asarray(points).reshape(-1, 3), f32)
    p64 = p32.astype(np.float64)
    cm64 = com.astype(np.float64)
    Q = q_matrix(q6)
    m, n = len(skip), len(p32)
    g64 = float(f32(g))
    eps2 = float(f32(f32(g_soft) * f32(g_soft)))
    th = f32(theta2)
    S = np.zeros((n, 3))
    T = np.zeros(n)
    acc = np.zeros(n, np.uint64)
    vis = np.zeros(n, np.uint64)
    nxt = np.zeros(n, np.int64)
    takers = np.zeros(m, np.int64)
    with np.errstate(over="ignore"):
        for i in range(m):
            b = np.flatnonzero(nxt == i)
            if not len(b):
                continue
            r = com[i, :3] - p32[b]                              # float32, as the kernel
            r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            vis[b] += 1
            is_leaf = skip[i] == i + 1
            take = w2[i] < th * r2
            if leaf == 1:
                near = r2 < f32(1e-10)
                take = (take | is_leaf) & ~near
                jump = take | near
            else:
                jump = take
            nxt[b] = np.where(jump, skip[i], i + 1)
            t = b[take]
            if len(t):
                mono, t1, t2 = node_terms(cm64[i], Q[i], not is_leaf, p64[t], g64, eps2, c2)
                S[t] += mono + t1 + t2
                T[t] += np.linalg.norm(mono, axis=1) + np.linalg.norm(t1, axis=1) + np.linalg.norm(t2, axis=1)
                acc[t] += 1
                takers[i] = len(t)
    return dict(S=S, T=T, accepted=acc, visited=vis, takers=takers)


def direct_sum(points, pos, mass, g, g_soft):
    """[n, 3] f64 exact accelerations at `points` from bodies (pos, mass); a body at zero distance is skipped."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    y = np.asarray(pos, np.float64)
    mm = np.asarray(mass, np.float64)
    eps2 = float(g_soft) ** 2
    out = np.zeros_like(x)
    for k0 in range(0, len(x), 512):
        d = y[None, :, :] - x[k0:k0 + 512, None, :]
        r2 = (d * d).sum(2)
        with np.errstate(divide="ignore"):
            k = np.where(r2 > 0, mm[None, :] / ((r2 + eps2) * np.sqrt(r2 + eps2)), 0.0)
        out[k0:k0 + 512] = float(g) * (d * k[:, :, None]).sum(1)
    return out


def rel_errors(a, exact):
    """|a - a_exact| / |a_exact| per body."""
    a = np.asarray(a, np.float64)[:, :3]
    return np.linalg.norm(a - exact, axis=1) / np.linalg.norm(exact, axis=1)


def tensor_errors(q_dev, q_ref, A):
    """Per node max_ab |Q_dev - Q_ref| / A (0 where both are exactly 0, inf where A = 0 and they differ or Q_dev is not finite)."""
    num = np.abs(np.asarray(q_dev, np.float64) - q_ref).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(A > 0, num / np.where(A > 0, A, 1.0), np.where(num == 0, 0.0, np.inf))
    err[~np.isfinite(np.asarray(q_dev, np.float64)).all(1)] = np.inf
    return err
