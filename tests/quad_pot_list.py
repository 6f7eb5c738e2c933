"""Checking nbody_potentials / nbody_field_at in NBODY_POTENTIAL_TREE_QUADRUPOLE against the sums over their own node list.

`replay(tree, points, q6, theta2, g_soft)` is tests/field_list.py's loop -- the potential walk's opening tests under the DIRECT
leaf rule in float32, at the points rounded to float32 -- with the quadrupole term of every accepted INTERNAL node, from the
float32 tensors it is GIVEN (the device's own export in the GPU tests; their rounding is judged separately, by
quad_list.tensor_errors).  With d = c - x, s^2 = |d|^2 + eps^2, inv = 1 / s, u = d inv it returns, per point,

    S  = sum [ M inv + 1/2 (u^T Q u) inv^3 ]                                  (phi = -g S)
    A  = sum [ M d inv^3 - inv^4 (Q u) + 2.5 inv^4 (u^T Q u) u ]   [3]        (acc = g A = -grad phi)
    Ts = sum [ M inv + 1/2 N inv^3 ]            N   = sum_ab |u_a Q_ab u_b|
    Tv = sum [ M |d| inv^3 + inv^4 |n| + 2.5 inv^4 N |u| ]      n_a = sum_b |Q_ab u_b|, |.| the 2-norm
    accepted, visited, n_terms = accepted + accepted internal nodes (the f64 additions per sum)

Ts and Tv are the sums of the MAGNITUDES of the monopole part and of each quadrupole part of every accepted term, taken with
no cancellation inside a part (u^T Q u of a traceless tensor vanishes on a cone of directions; an f32 evaluation cannot be
relatively accurate there, only accurate relative to N).  An accepted leaf contributes the monopole part alone.  The sums are
accumulated in `dtype` (float64; np.longdouble gives field_list.replay's bits at theta2 = 0, float64 gives pot_list.replay's).

The bounds, per point, derived by counting the roundings of the expressions k_bh_pot_walk_quad / k_bh_field_walk_quad
(kernels_quad.hip, pot_quad_parts) are written in; u = 2^-24, first order in u, every fl() one rounding, fmaf one:

    d_c = fl(c_c - x_c)                                               1 u
    q   = fl(fl(fl(dx dx + dy dy) + dz dz) + eps2)                    6 u   (field_list.py)
    s   = fl(sqrt(q))      inv = fl(1 / s)                            4 u,  5 u
    st  = fl(M inv)                                                   6 u   monopole scalar part (a leaf in the potential walk: fl(M / s), 5 u)
    fl(d_c fl(st / q))                                                15 u  monopole vector part (field_list.py)
    u_c = fl(d_c inv)                                                 1 + 5 + 1 = 7 u
    p_c = fma(Q_c0, u_0, fma(Q_c1, u_1, fl(Q_c2 u_2)))                7 u from u and 3 roundings of partial sums: 10 u of n_c
    uqu = fma(u_0, p_0, fma(u_1, p_1, fl(u_2 p_2)))                   7 u (u_a) + 10 u (p_a) + 3 roundings: 20 u of N
    i2  = fl(inv inv)                                                 5 + 5 + 1 = 11 u
    P   = fl(fl(fl(0.5 uqu) i2) inv)                                  20 + 0 + (11 + 1) + (5 + 1) = 38 u of 1/2 N inv^3
    i4  = fl(i2 i2)                                                   11 + 11 + 1 = 23 u
    w   = fl(fl(2.5 uqu) i4)                                          (20 + 1) + 23 + 1 = 45 u
    b_c = fl(i4 p_c)                                                  23 + 10 + 1 = 34 u of inv^4 n_c
    V_c = fma(w, u_c, -b_c)                                           w u_c: 45 + 7 = 52 u; one rounding of at most |w u_c| + |b_c|:
                                                                      53 u of 2.5 inv^4 N |u_c|  and  35 u of inv^4 n_c

The worst part decides (every part's magnitude is in Ts / Tv with weight 1); one more u covers the product with g and second
order, as in field_list.py.  The f32 parts are widened and added in f64, n_terms additions per sum:

    |phi + g S|      <= (C_S u + n_terms 2^-53) g Ts        C_S = 38 + 1 = 39
    |acc_c - g A_c|  <= (C_V u + n_terms 2^-53) g Tv        C_V = 53 + 1 = 54

The bounds are relative, so they hold inside float32's range only: a point so far away that r2 overflows gets exact zeros from
the device (field_list.py), and a point from which inv^3 or inv^4 underflows (beyond ~1e9 from the bodies) is outside them.

Worst observed ratios to these bounds on an MI355X (tests/test_quadrupole_potentials_gpu.py, pytest -s): WORST_OBSERVED.

Plain test infrastructure (no GPU); tests/test_quad_pot_list_checker.py checks it on the CPU.
"""
from __future__ import annotations

import numpy as np

from quad_list import direct_sum, node_quadrupoles, plummer_bodies, q_matrix, walk_list_quad  # noqa: F401  (re-exported for the tests)
from field_list import eps2_of, rounded

U32, U64 = 2.0 ** -24, 2.0 ** -53
C_S, C_V = 39.0, 54.0
#: worst ratio to the bound seen on the device over the cases of tests/test_quadrupole_potentials_gpu.py.  None: NOT MEASURED on
#: an MI355X yet (no GPU time was to be had when this was written); the tests print them (pytest -s) and assert <= 1.
WORST_OBSERVED = {"potentials_phi": None, "field_phi": None, "field_acc": None}

#: f64 replays (order 1 = zero tensors, order 2 = node_quadrupoles' f64 tensors) over the host-built tree of
#: plummer_bodies(nb, 4097, seed=4097), g_soft = 0, against the f64 pair sum: (median, 99th percentile) of |phi - phi_exact| / |phi_exact|.
#: Measured by tests/test_quad_pot_list_checker.py::test_f64_error_distributions, which recomputes and compares them.
F64_POT_ERRORS = {
    # (order, theta2): (median, p99)
    (1, 0.25): (2.0249e-04, 7.7403e-04),
    (2, 0.25): (4.6497e-05, 1.9734e-04),
    (1, 1.0): (1.2220e-03, 4.6139e-03),
    (2, 1.0): (4.8436e-04, 2.4512e-03),
}
ACCURACY_N = 4097


def _q_apply(q, v):
    """(Q v) for q [k, 6] {xx, xy, xz, yy, yz, zz} and v [k, 3]."""
    return np.stack([q[:, 0] * v[:, 0] + q[:, 1] * v[:, 1] + q[:, 2] * v[:, 2],
                     q[:, 1] * v[:, 0] + q[:, 3] * v[:, 1] + q[:, 4] * v[:, 2],
                     q[:, 2] * v[:, 0] + q[:, 4] * v[:, 1] + q[:, 5] * v[:, 2]], axis=1)


def terms(cm, q, internal, x, eps2, c_half=0.5, c2=2.5, drop_qd=False):
    """The parts of the terms of nodes (cm [k, 4], q [k, 6], internal [k] bool) at points x [k, 3], all of one float type:
    (scalar monopole, scalar quadrupole, vector monopole [k, 3], vector quadrupole [k, 3], Ts share, Tv share).  c_half, c2,
    drop_qd: deliberately wrong walks (1/2 -> c_half, 2.5 -> c2, the Q d part left out)."""
    d = cm[:, :3] - x
    d2 = (d * d).sum(1)
    s2 = d2 + eps2
    mass = cm[:, 3]
    k3 = mass / (s2 * np.sqrt(s2))
    sm = mass / np.sqrt(s2)
    vm = d * k3[:, None]
    tv = np.sqrt(d2) * k3
    sq, vq, ts = np.zeros_like(sm), np.zeros_like(vm), np.abs(sm)
    if internal.any():   # the quadrupole parts, of the internal nodes alone
        di, qi = d[internal], q[internal]
        inv = 1 / np.sqrt(s2[internal])
        u = di * inv[:, None]
        p = _q_apply(qi, u)
        uqu = (u * p).sum(1)
        nvec = _q_apply(np.abs(qi), np.abs(u))
        N = (np.abs(u) * nvec).sum(1)
        inv3, inv4 = inv * inv * inv, (inv * inv) * (inv * inv)
        sq[internal] = c_half * uqu * inv3
        vq[internal] = u * (c2 * uqu * inv4)[:, None] - (0 if drop_qd else 1) * p * inv4[:, None]
        ts[internal] += 0.5 * N * inv3
        tv[internal] += inv4 * np.sqrt((nvec * nvec).sum(1)) + 2.5 * inv4 * N * np.sqrt((u * u).sum(1))
    return sm, sq, vm, vq, ts, tv


def replay(tree, points, q6, theta2, g_soft, dtype=np.float64, keep_lists=False, **wrong) -> dict:
    """DIRECT walk of every point over `tree` (float32 records) with the tensors q6 [m, 6]; S [n], A [n, 3], Ts [n], Tv [n]
    (f64, evaluated and accumulated in `dtype`), accepted, visited, n_terms [n]; keep_lists: lists = per point the accepted
    nodes in walk order.  **wrong: see `terms`."""
    f32 = np.float32
    com = np.ascontiguousarray(tree["com_mass"], f32)
    w = np.ascontiguousarray(tree["width"], f32)
    w2 = w * w
    skip = np.ascontiguousarray(tree["skip"], np.int64)
    m = len(w)
    p = rounded(points, f32)
    n = len(p)
    comX, pX = com.astype(dtype), p.astype(dtype)
    qX = np.asarray(q6).reshape(-1, 6).astype(dtype)
    eps2 = dtype(eps2_of(f32, g_soft))
    th, near = f32(theta2), f32(1e-10)
    S, A, Ts, Tv = np.zeros(n, dtype), np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    acc, vis, nt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    lists = [[] for _ in range(n)] if keep_lists else None
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
                internal = skip[it] != it + 1
                sm, sq, vm, vq, ts, tv = terms(comX[it], qX[it], internal, pX[bt], eps2, **wrong)
                S[bt] += sm
                A[bt] += vm
                bi = bt[internal]           # the quadrupole parts: an addition of their own, after the monopole part's
                S[bi] += sq[internal]
                A[bi] += vq[internal]
                Ts[bt] += ts
                Tv[bt] += tv
                acc[bt] += 1
                nt[bt] += 1
                nt[bi] += 1
                if keep_lists:
                    for b_, i_ in zip(bt.tolist(), it.tolist()):
                        lists[b_].append(i_)
            i = np.where(skipped | take, sk, i + 1)
            live = i < m
            if not live.all():
                body, i = body[live], i[live]
    out = dict(S=S.astype(np.float64), A=A.astype(np.float64), Ts=Ts.astype(np.float64), Tv=Tv.astype(np.float64), accepted=acc, visited=vis, n_terms=nt)
    if keep_lists:
        out["lists"] = lists
    return out


def eval_lists(tree, q6, x, lists, g_soft):
    """S [n] and A [n, 3] in f64 at the (unrounded) f64 points x over FIXED accepted-node lists: the function whose gradient A is."""
    com = np.asarray(tree["com_mass"], np.float64)
    skip = np.asarray(tree["skip"], np.int64)
    q = np.asarray(q6, np.float64).reshape(-1, 6)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    eps2 = eps2_of(np.float32, g_soft)
    S, A = np.zeros(len(x)), np.zeros((len(x), 3))
    for k, nodes in enumerate(lists):
        it = np.asarray(nodes, np.int64)
        if not len(it):
            continue
        sm, sq, vm, vq, _, _ = terms(com[it], q[it], skip[it] != it + 1, np.repeat(x[k:k + 1], len(it), 0), eps2)
        S[k] = (sm + sq).sum()
        A[k] = (vm + vq).sum(0)
    return S, A


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in f64 and the sum is rounded there first (a double rounding, 2^-29 u)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_f32(tree, q6, points, lists, g_soft):
    """The kernels' written-out f32 expressions (module docstring; kernels_quad.hip pot_quad_parts) in numpy float32 over
    FIXED accepted-node lists, the parts widened and added in f64: (S of k_bh_field_walk_quad, S of k_bh_pot_walk_quad -- a
    leaf there is fl(M / s) --, A [n, 3]).  numpy's float32 sqrt and divide are IEEE, as the device's are built to be."""
    f32 = np.float32
    com = np.ascontiguousarray(tree["com_mass"], f32)
    skip = np.asarray(tree["skip"], np.int64)
    q = np.asarray(q6, f32).reshape(-1, 6)
    p = rounded(points, f32)
    eps2 = f32(f32(g_soft) * f32(g_soft))
    S, Sp, A = np.zeros(len(p)), np.zeros(len(p)), np.zeros((len(p), 3))
    for k, nodes in enumerate(lists):
        it = np.asarray(nodes, np.int64)
        if not len(it):
            continue
        c, Q = com[it], q[it]
        r = [c[:, a] - p[k, a] for a in range(3)]
        r2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        qq = r2 + eps2
        s = np.sqrt(qq)
        inv = f32(1) / s
        internal = skip[it] != it + 1
        st = c[:, 3] * inv
        kk = st / qq
        u = [r[a] * inv for a in range(3)]
        row = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
        pq = [_fma32(Q[:, row[a][0]], u[0], _fma32(Q[:, row[a][1]], u[1], Q[:, row[a][2]] * u[2])) for a in range(3)]
        uqu = _fma32(u[0], pq[0], _fma32(u[1], pq[1], u[2] * pq[2]))
        i2 = inv * inv
        P = np.where(internal, ((f32(0.5) * uqu) * i2) * inv, f32(0))
        i4 = i2 * i2
        w = (f32(2.5) * uqu) * i4
        S[k] = st.astype(np.float64).sum() + P.astype(np.float64).sum()
        Sp[k] = np.where(internal, st, c[:, 3] / s).astype(np.float64).sum() + P.astype(np.float64).sum()
        for a in range(3):
            V = np.where(internal, _fma32(w, u[a], -(i4 * pq[a])), f32(0))
            A[k, a] = (r[a] * kk).astype(np.float64).sum() + V.astype(np.float64).sum()
    return S, Sp, A


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    r[~np.isfinite(num)] = np.inf
    return r


def ratios(acc, phi, ref, g):
    """(per-point worst component |acc_c - g A_c| / bound, |phi + g S| / bound); either input may be None (-> None)."""
    g = float(g)
    out_a = out_p = None
    if acc is not None:
        a = np.asarray(acc, np.float64).reshape(-1, 3)
        out_a = _ratio(np.abs(a - g * ref["A"]).max(1), (C_V * U32 + ref["n_terms"] * U64) * abs(g) * ref["Tv"])
    if phi is not None:
        ph = np.asarray(phi, np.float64)
        out_p = _ratio(np.abs(ph + g * ref["S"]), (C_S * U32 + ref["n_terms"] * U64) * abs(g) * ref["Ts"])
    return out_a, out_p


def check(acc, phi, counts, ref, g, what="") -> tuple:
    """Counts exact, every point within both bounds (a point with Ts = 0 must get exactly 0); returns the worst ratios (acc, phi)."""
    n = len(ref["S"])
    want = (int(ref["accepted"].sum()), int(ref["visited"].sum()))
    if counts is not None:
        assert tuple(int(c) for c in counts) == want, f"{what}: counts {tuple(counts)}, the node list gives {want}"
    ra, rp = ratios(acc, phi, ref, g)
    worst = []
    for name, r, got in (("acc", ra, acc), ("phi", rp, phi)):
        if r is None:
            worst.append(0.0)
            continue
        assert len(r) == n and len(got) == n, f"{what}: {len(got)} {name} results for {n} points"
        w = float(r.max()) if n else 0.0
        if not w <= 1.0:
            bad = np.flatnonzero(~(r <= 1.0))
            raise AssertionError(f"{what}: {name} of {len(bad)} of {n} points beyond the bound, first {bad[:8].tolist()} at {r[bad[:8]].tolist()} x the bound")
        worst.append(w)
    return tuple(worst)
