"""tests/tidal_list.py held to account without a GPU: pair_tidal against a central finite difference of field_list.pair_field's
acceleration (tolerance from the scheme's own error term), the tensor's symmetry and trace, replay_tidal's counts against
field_list.replay's and its sums against pair_tidal at theta2 = 0, planted faults, the W = 0 rule, and that check_tidal cannot
be made to skip a row.  Plus the ABI of nbody_tidal_at."""
import ctypes
import inspect

import numpy as np
import pytest

import field_list
import tidal_list

LD = np.longdouble
BOX = ((0.0, 0.0, 0.0), 64.0)
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # the rows' order


def world(nb, orc, n, f64, seed=5):
    rec = nb.plummer(2 * n + 64, seed=seed, f64=f64)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 30.0][:n])
    rec["mass"] *= np.random.default_rng(seed).uniform(0.5, 1.5, n).astype(rec["mass"].dtype)   # (no two neighbours of one mass)
    a = rec.astype(orc.P64 if f64 else orc.P32)
    return a, orc.bh_build_tree(a, *BOX)


def clear_probes(rec, n, seed, keep=0.05):
    """n points around the bodies, none within `keep` of one"""
    rng = np.random.default_rng(seed)
    x = rec["position"].astype(np.float64)
    out = np.zeros((0, 3))
    while len(out) < n:
        p = rng.uniform(-3.0, 3.0, (4 * n, 3))
        d = np.sqrt(((p[:, None, :] - x[None, :, :]) ** 2).sum(2)).min(1)
        out = np.concatenate([out, p[d > keep]])
    return np.ascontiguousarray(out[:n])


@pytest.mark.parametrize("g_soft", [0.0, 0.01])
def test_pair_tidal_is_the_gradient_of_the_pair_acceleration(nb, g_soft):
    """T_ab against [a_a(x + h e_b) - a_a(x - h e_b)] / (2 h), h = 1e-4.  The scheme's error is h^2 / 6 times the third derivative
    of a_a along e_b somewhere within h of x.  Along any straight line m / sqrt(|d|^2 + eps^2) is the Newtonian m / r of a point
    off that line, so its n-th derivative along a unit vector is n! P_n m / s^(n + 1), at most n! m / s^(n + 1), and a mixed
    derivative of a symmetric form is no larger than the largest one along a single direction: the fourth derivative of the
    potential is at most 24 m / s^5, with s taken 2 h nearer than it is at x.  The acceleration comes back in f64, half an ulp
    per value, and x +- h are f64 too, so the step is taken as it came out and the midpoint's shift (an ulp of x) costs the
    third derivative of the potential, 6 m / s^4, times it."""
    rec = np.ascontiguousarray(nb.plummer(200, seed=3, f64=True))
    pts = clear_probes(rec, 50, seed=4)
    h = 1e-4
    got = tidal_list.pair_tidal(rec, pts, g_soft)
    assert (got["accepted"] == 200).all()
    x, m = rec["position"].astype(LD), rec["mass"].astype(LD)
    r = np.sqrt(((x[None, :, :] - pts.astype(LD)[:, None, :]) ** 2).sum(2))
    assert float(r.min()) > 0.05
    s_near = np.sqrt((r - LD(2 * h)) ** 2 + LD(g_soft) ** 2)
    d4 = (24 * m[None, :] / s_near ** 5).sum(1)
    d3 = (6 * m[None, :] / s_near ** 4).sum(1)
    worst = 0.0
    for b in range(3):
        e = np.zeros(3)
        e[b] = h
        hi, lo = pts + e, pts - e
        step = (hi[:, b].astype(LD) - lo[:, b].astype(LD))           # ~2 h, as f64 made it
        shift = np.abs((hi[:, b].astype(LD) + lo[:, b].astype(LD)) / 2 - pts[:, b].astype(LD))
        fp, fm = field_list.pair_field(rec, hi, g_soft), field_list.pair_field(rec, lo, g_soft)
        for a in range(3):
            fd = (fp["A"][:, a].astype(LD) - fm["A"][:, a].astype(LD)) / step
            tol = (step / 2) ** 2 / 6 * d4 + shift * d3 + field_list.U64 * (np.abs(fp["A"][:, a]) + np.abs(fm["A"][:, a])) / step
            c = SIX.index((min(a, b), max(a, b)))
            err = np.abs(fd - got["S6"][:, c])
            assert (err <= tol).all(), (a, b, float((err / tol).max()))
            worst = max(worst, float((err / tol).max()))
            assert float((tol / got["W"]).max()) < 1e-5   # the tolerance is a statement: seven digits of the tensor's scale
    print(f"\n[tidal_list] finite difference, g_soft={g_soft}: worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("g_soft", [0.0, 0.01])
def test_symmetry_and_trace(nb, g_soft):
    """tidal_matrices of the six rows is symmetric by construction, and the trace is -3 eps^2 sum m / q^(5/2): zero without
    softening.  Tolerance: a term's three diagonal entries carry a handful of longdouble roundings each, of at most its share
    of W, and the n additions one each: (64 + 2 n) 2^-64 W."""
    rec = np.ascontiguousarray(nb.plummer(200, seed=3, f64=True))
    pts = clear_probes(rec, 50, seed=6)
    got = tidal_list.pair_tidal(rec, pts, g_soft)
    mats = nb.tidal_matrices(got["S6"].astype(np.float64))
    assert mats.shape == (50, 3, 3) and np.array_equal(mats, mats.transpose(0, 2, 1))
    for c, (a, b) in enumerate(SIX):
        assert np.array_equal(mats[:, a, b], got["S6"][:, c].astype(np.float64))
    x, m = rec["position"].astype(LD), rec["mass"].astype(LD)
    q = ((x[None, :, :] - pts.astype(LD)[:, None, :]) ** 2).sum(2) + LD(g_soft) ** 2
    want = -3 * LD(g_soft) ** 2 * (m[None, :] / (q * q * np.sqrt(q))).sum(1)
    trace = got["S6"][:, 0] + got["S6"][:, 3] + got["S6"][:, 5]
    tol = (64 + 2 * len(rec)) * LD(2.0) ** -64 * got["W"]
    assert (np.abs(trace - want) <= tol).all()
    if g_soft == 0.0:
        assert (want == 0).all()
    else:
        assert (want < 0).all() and (np.abs(want) > 1e3 * tol).all()   # the softening's trace is seen, not lost in the tolerance


@pytest.mark.parametrize("f64", [False, True])
def test_replay_tidal_walks_as_field_list_replay_and_sums_as_pair_tidal(nb, orc, f64):
    a, tree = world(nb, orc, 300, f64)
    rng = np.random.default_rng(2)
    pts = np.concatenate([a["position"][:40].astype(np.float64), rng.uniform(-32, 32, (100, 3)), rng.uniform(-100, 100, (60, 3))])
    for theta2, g_soft in ((0.25, 0.0), (1.0, 0.01), (0.0, 0.0)):
        got = tidal_list.replay_tidal(tree, pts, theta2, g_soft)
        ref = field_list.replay(tree, pts, theta2, g_soft)
        assert np.array_equal(got["accepted"], ref["accepted"]) and np.array_equal(got["visited"], ref["visited"])
    # theta2 = 0, no softening (an f32 tree squares g_soft in f32, the pair sum in f64): every other leaf, the pair sum
    pair = tidal_list.pair_tidal(a, pts, 0.0)
    assert np.array_equal(got["accepted"], pair["accepted"])
    assert (np.abs(got["S6"] - pair["S6"]).max(1) <= 1e-15 * pair["W"]).all()
    assert (np.abs(got["W"] - pair["W"]) <= 1e-15 * pair["W"]).all()


@pytest.mark.parametrize("f64", [False, True])
def test_planted_faults_are_caught(nb, orc, f64):
    n, theta2, g_soft, g = 300, 0.25, 0.01, 1.25
    a, tree = world(nb, orc, n, f64)
    pts = np.random.default_rng(1).uniform(-32, 32, (120, 3))
    ref = tidal_list.replay_tidal(tree, pts, theta2, g_soft)
    counts = (int(ref["accepted"].sum()), int(ref["visited"].sum()))
    exact = (LD(g) * ref["S6"]).astype(np.float64)
    assert tidal_list.check_tidal(exact, counts, ref, g, "tree", f64) <= 0.05   # (the conversion to f64 alone)
    i = 77
    # a term whose neighbour in the array has another mass (an only child has its parent's, the array's last node has no neighbour)
    k = next(k for k in range(int(ref["accepted"][i]))
             if not np.array_equal(tidal_list.replay_tidal(tree, pts[i:i + 1], theta2, g_soft, wrong_mass=(0, k))["S6"], ref["S6"][i:i + 1]))
    for fault in (dict(drop=(i, k)), dict(wrong_mass=(i, k))):
        bad = tidal_list.replay_tidal(tree, pts, theta2, g_soft, **fault)
        assert np.array_equal(bad["accepted"], ref["accepted"])
        assert np.array_equal(np.flatnonzero((bad["S6"] != ref["S6"]).any(1)), [i])
        with pytest.raises(AssertionError, match="beyond the bound"):
            tidal_list.check_tidal((LD(g) * bad["S6"]).astype(np.float64), counts, ref, g, "tree", f64, what=str(fault))
    swapped = exact.copy()
    swapped[i, [1, 2]] = swapped[i, [2, 1]]   # xy and xz in each other's place
    with pytest.raises(AssertionError, match="beyond the bound"):
        tidal_list.check_tidal(swapped, counts, ref, g, "tree", f64)
    with pytest.raises(AssertionError, match="counts"):
        tidal_list.check_tidal(exact, (counts[0] - 1, counts[1]), ref, g, "tree", f64)
    # PAIRS: the same against the pair sums
    pref = tidal_list.pair_tidal(a, pts, g_soft)
    pexact = (LD(g) * pref["S6"]).astype(np.float64)
    assert tidal_list.check_tidal(pexact, (0, 0), pref, g, "pairs", f64, n) <= 0.05
    worse = pexact.copy()
    worse[i] *= 1.0 + 1e-9
    with pytest.raises(AssertionError, match="beyond the bound"):
        tidal_list.check_tidal(worse, (0, 0), pref, g, "pairs", f64, n)
    nan = pexact.copy()
    nan[i, 4] = np.nan
    with pytest.raises(AssertionError, match="beyond the bound"):
        tidal_list.check_tidal(nan, (0, 0), pref, g, "pairs", f64, n)


def test_a_row_without_terms_must_be_exactly_zero_and_no_row_can_be_skipped(nb):
    rec = np.ascontiguousarray(nb.plummer(1, seed=1, f64=True))
    pts = np.concatenate([rec["position"].astype(np.float64), [[1.0, 2.0, 3.0]]])   # on the only body: no term at all
    ref = tidal_list.pair_tidal(rec, pts, 0.0)
    assert ref["W"][0] == 0 and ref["accepted"].tolist() == [0, 1]
    good = (LD(1.0) * ref["S6"]).astype(np.float64)
    assert tidal_list.check_tidal(good, (0, 0), ref, 1.0, "pairs", True, 1) <= 0.05
    bad = good.copy()
    bad[0, 3] = 1e-300
    with pytest.raises(AssertionError, match="beyond the bound"):
        tidal_list.check_tidal(bad, (0, 0), ref, 1.0, "pairs", True, 1)
    # no mask, no subset: fewer rows than probes, or more, are refused
    assert list(inspect.signature(tidal_list.check_tidal).parameters) == ["t6", "counts", "ref", "g", "mode", "f64", "n_bodies", "what"]
    assert list(inspect.signature(tidal_list.ratios).parameters) == ["t6", "ref", "g", "mode", "f64", "n_bodies"]
    for rows in (good[:1], np.concatenate([good, good])):
        with pytest.raises(AssertionError, match="shape"):
            tidal_list.check_tidal(rows, (0, 0), ref, 1.0, "pairs", True, 1)


def test_abi_of_nbody_tidal_at(nb):
    assert "nbody_tidal_at" in nb.DECLARED_SYMBOLS
    assert nb.lib.nbody_abi_version() == 4
    fn = nb.lib.nbody_tidal_at
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    assert fn(None, 0, None, 0, None, None) == nb.NBODY_ERR_INVALID   # a null handle is refused without touching a device
    assert list(inspect.signature(nb.Simulation.tidal_at).parameters) == ["self", "points", "mode", "counts"]
    header = open(nb.LIB_PATH.replace("nbody-llm_amd/libnbody_hip.so", "include/nbody_hip.h")).read()
    assert "int nbody_tidal_at(NbodyHandle* h, int mode, const double* xyz, size_t n_points, double* tidal6, uint64_t counts[2]);" in header
