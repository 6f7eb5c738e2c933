"""The checker of tests/quad_pot_list.py, on the CPU (trees from nb.host_build_tree): the term reproduces the two-mass
expansion, A is the gradient of S, at theta2 = 0 the replay gives the bits of pot_list.replay and field_list.replay and its
counts equal theirs at every theta2, the mistakes a quadrupole potential walk could make break the derived bounds, and the
f64 error distributions of the monopole and the quadrupole potential against the pair sum are measured and pinned."""
import numpy as np
import pytest

import field_list
import pot_list
import quad_pot_list as qp
from quad_pot_list import node_quadrupoles, plummer_bodies

BOX = ((0.0, 0.0, 0.0), 64.0)
_cache = {}


def world(nb, n, seed):
    """(records, host-built tree, f64 tensors)."""
    if (n, seed) not in _cache:
        rec = plummer_bodies(nb, n, seed)
        tree = nb.host_build_tree(np.concatenate([rec["position"], rec["mass"][:, None]], axis=1), *BOX)
        _cache[(n, seed)] = (rec, tree, node_quadrupoles(tree["com_mass"], tree["skip"])[0])
    return _cache[(n, seed)]


def test_two_masses_on_an_axis():
    """Masses m at +-s on the x axis seen from R on it: the root's term gives phi = -g (2 m / R)(1 + s^2 / R^2), the exact
    -g m [1 / (R - s) + 1 / (R + s)] up to O((s / R)^4)."""
    m, s, R, g = 0.75, 0.5, 8.0, 1.5
    tree = dict(com_mass=np.array([[0, 0, 0, 2 * m], [-s, 0, 0, m], [s, 0, 0, m]], np.float32), width=np.array([64, 32, 32], np.float32),
                skip=np.array([3, 2, 3], np.int32))
    q6, _ = node_quadrupoles(tree["com_mass"], tree["skip"])
    ref = qp.replay(tree, [[R, 0, 0]], q6, 1e30, 0.0)
    assert ref["accepted"][0] == 1 and ref["visited"][0] == 1 and ref["n_terms"][0] == 2
    phi = -g * ref["S"][0]
    assert abs(phi + g * (2 * m / R) * (1 + s * s / (R * R))) <= 1e-15 * abs(phi)
    exact = -g * m * (1 / (R - s) + 1 / (R + s))
    assert abs(phi - exact) <= 1.1 * abs(exact) * (s / R) ** 4 and abs(phi - exact) > 0.5 * abs(exact) * (s / R) ** 4
    # the vector sum is the force walk's term (quad_list's two-mass pin): 2 m / R^2 (1 + 3 s^2 / R^2), towards the masses
    assert np.allclose(ref["A"][0], [-(2 * m / R ** 2) * (1 + 3 * s * s / R ** 2), 0, 0], rtol=1e-15, atol=0)
    # the magnitudes: no cancellation on the axis, so Ts = S
    assert ref["Ts"][0] == pytest.approx(ref["S"][0], rel=1e-15)
    mono = qp.replay(tree, [[R, 0, 0]], q6, 0.0, 0.0)   # both leaves
    assert mono["accepted"][0] == 2 and mono["n_terms"][0] == 2 and abs(-g * mono["S"][0] - exact) <= 1e-15 * abs(exact)


def test_the_vector_sum_is_the_gradient_of_the_scalar_sum(nb):
    """Central differences of S over fixed accepted-node lists, in f64: dS/dx_k = A_k (acc = g A = -grad phi, phi = -g S)."""
    rec, tree, q6 = world(nb, 65, 65)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rec["position"].astype(np.float64), rng.uniform(-30, 30, (40, 3))])
    for theta2 in (0.25, 1.0):
        ref = qp.replay(tree, pts, q6, theta2, 0.01, keep_lists=True)
        assert (ref["n_terms"] > ref["accepted"]).any()   # internal nodes among the accepted
        x = field_list.rounded(pts, np.float32).astype(np.float64)
        S0, A0 = qp.eval_lists(tree, q6, x, ref["lists"], 0.01)
        assert np.allclose(S0, ref["S"], rtol=1e-13, atol=0) and np.allclose(A0, ref["A"], rtol=1e-9, atol=1e-13)
        h = 1e-5
        grad = np.zeros_like(A0)
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            grad[:, k] = (qp.eval_lists(tree, q6, x + e, ref["lists"], 0.01)[0] - qp.eval_lists(tree, q6, x - e, ref["lists"], 0.01)[0]) / (2 * h)
        err = np.linalg.norm(grad - A0, axis=1) / np.linalg.norm(A0, axis=1)
        print(f"\n[quad pot list] theta2={theta2}: worst |grad S - A| / |A| {err.max():.2e}")
        assert err.max() <= 1e-6


@pytest.mark.parametrize("n", [9, 65, 1001])
def test_bits_at_theta2_zero_and_counts_everywhere(nb, n):
    rec, tree, q6 = world(nb, n, n)
    rng = np.random.default_rng(n)
    pts = np.concatenate([rec["position"].astype(np.float64), rng.uniform(-40, 40, (50, 3))])
    for theta2 in (0.0, 0.25, 1.0, 1e30):
        for g_soft in (0.0, 0.01):
            ours = qp.replay(tree, rec["position"], q6, theta2, g_soft)
            pot = pot_list.replay(tree, rec["position"], theta2, g_soft)
            oursL = qp.replay(tree, pts, q6, theta2, g_soft, dtype=np.longdouble)
            fld = field_list.replay(tree, pts, theta2, g_soft)
            for k in ("accepted", "visited"):
                assert np.array_equal(ours[k], pot[k]) and np.array_equal(oursL[k], fld[k])
            if theta2 == 0.0:
                assert np.array_equal(ours["S"], pot["S"]) and np.array_equal(ours["n_terms"], ours["accepted"])
                assert np.array_equal(oursL["S"], fld["S"]) and np.array_equal(oursL["A"], fld["A"]) and np.array_equal(oursL["Tv"], fld["T"])
                assert np.array_equal(oursL["Ts"], fld["S"])
            elif n > 9:
                assert not np.array_equal(ours["S"], pot["S"])


def test_the_checker_sees_a_wrong_walk(nb):
    """n = 4097, theta2 = 0.25: coefficient 1 for 1/2 in S, 2 for 2.5 in A, the Q d part dropped -- each beyond the derived
    bound around the correct replay for more than half of the bodies (a bound that let them pass would be no test)."""
    rec, tree, q6 = world(nb, 4097, 4097)
    q32 = q6.astype(np.float32)
    good = qp.replay(tree, rec["position"], q32, 0.25, 0.0)
    ra, rp = qp.ratios(good["A"], -good["S"], good, 1.0)
    assert ra.max() == 0.0 and rp.max() == 0.0
    for wrong, which in ((dict(c_half=1.0), "phi"), (dict(c2=2.0), "acc"), (dict(drop_qd=True), "acc")):
        bad = qp.replay(tree, rec["position"], q32, 0.25, 0.0, **wrong)
        ra, rp = qp.ratios(bad["A"], -bad["S"], good, 1.0)
        share = float(((rp if which == "phi" else ra) > 1.0).mean())
        print(f"\n[quad pot list] {wrong}: {share:.3f} of the bodies beyond the {which} bound")
        assert share > 0.5
        with pytest.raises(AssertionError):
            qp.check(bad["A"], -bad["S"], None, good, 1.0)


@pytest.mark.parametrize("case", ["plummer", "clump"])
def test_the_written_out_f32_expressions_keep_the_derived_bounds(nb, case):
    """The kernels' expressions, operation by operation in numpy float32 (quad_pot_list.emulate_f32), stay within the bounds
    counted from them -- on a Plummer sphere and in the clump world, whose cells 1e-5 wide are accepted from 1e-5 away."""
    rng = np.random.default_rng(5)
    if case == "plummer":
        rec, tree, q6 = world(nb, 1001, 1001)
        pts = np.concatenate([rec["position"][::3].astype(np.float64), rng.uniform(-40, 40, (200, 3))])
    else:
        rec = plummer_bodies(nb, 1000, 11)
        c = np.array([1.3, -0.7, 0.4])
        rec["position"][300:] = (c + np.random.default_rng(11).uniform(-0.5e-5, 0.5e-5, size=(700, 3))).astype(np.float32)
        tree = nb.host_build_tree(np.concatenate([rec["position"], rec["mass"][:, None]], axis=1), *BOX)
        q6 = node_quadrupoles(tree["com_mass"], tree["skip"])[0]
        pts = np.concatenate([rec["position"][::5].astype(np.float64), c + rng.uniform(-1e-4, 1e-4, (200, 3))])
    q32 = q6.astype(np.float32)
    for theta2, g_soft in ((0.25, 0.0), (1.0, 0.01), (1e30, 0.0)):
        ref = qp.replay(tree, pts, q32, theta2, g_soft, keep_lists=True)
        S, Sp, A = qp.emulate_f32(tree, q32, pts, ref["lists"], g_soft)
        wa, wp = qp.check(A, -S, None, ref, 1.0, f"{case} theta2={theta2} field walk")
        _, wpp = qp.check(None, -Sp, None, ref, 1.0, f"{case} theta2={theta2} potential walk")
        print(f"\n[quad pot list] f32 emulation {case} theta2={theta2} g_soft={g_soft}: error / bound acc {wa:.3f} phi {wp:.3f} (potential walk {wpp:.3f})")
        assert wp > 0 and wa > 0   # (an f32 evaluation, not the f64 replay again)


def test_f64_error_distributions(nb):
    """The figures of quad_pot_list.F64_POT_ERRORS, recomputed; order 2 beats order 1 in the median and the 99th percentile at
    both opening angles."""
    n = qp.ACCURACY_N
    rec, tree, q6 = world(nb, n, n)
    with np.errstate(divide="ignore"):
        exact = -pot_list.pair_sums(rec, 0.0)
    got = {}
    for theta2 in (0.25, 1.0):
        for order, q in ((1, np.zeros_like(q6)), (2, q6)):
            e = np.abs(-qp.replay(tree, rec["position"], q, theta2, 0.0)["S"] - exact) / np.abs(exact)
            got[(order, theta2)] = (float(np.median(e)), float(np.percentile(e, 99)))
            print(f"\n[quad pot list] order {order} theta2 {theta2}: median {got[(order, theta2)][0]:.4e} p99 {got[(order, theta2)][1]:.4e}")
    for key, want in qp.F64_POT_ERRORS.items():
        assert np.allclose(got[key], want, rtol=1e-3, atol=0), (key, got[key], want)
    assert set(got) == set(qp.F64_POT_ERRORS)
    for theta2 in (0.25, 1.0):
        assert got[(2, theta2)][0] < got[(1, theta2)][0] and got[(2, theta2)][1] < got[(1, theta2)][1]
