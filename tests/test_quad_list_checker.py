"""The quadrupole checker of tests/quad_list.py, on the CPU (trees from nb.host_build_tree): the bottom-up tensors equal the
sums over each node's member bodies, the term reproduces the two-mass expansion, at theta2 = 0 the list sum is the direct
sum, the mistakes a quadrupole walk could make are reported as violations of |a - S| <= R T, and the f64 error distributions
of the monopole and the quadrupole walk against the direct sum are measured and pinned."""
import numpy as np

from quad_list import (ACCURACY_N, F64_ERRORS, QUAD_RTOL, direct_sum, node_quadrupoles, plummer_bodies, q_matrix, rel_errors, walk_list_quad)

BOX = ((0.0, 0.0, 0.0), 64.0)
G = 1.0
N_ACC = ACCURACY_N
_cache = {}

def world(nb, n=N_ACC, seed=N_ACC):
    """(records, host-built tree, f64 tensors, A, exact accelerations at g_soft = 0)."""
    key = (n, seed)
    if key not in _cache:
        rec = plummer_bodies(nb, n, seed)
        pos4 = np.concatenate([rec["position"], rec["mass"][:, None]], axis=1)
        tree = nb.host_build_tree(pos4, *BOX)
        q6, A = node_quadrupoles(tree["com_mass"], tree["skip"])
        exact = direct_sum(rec["position"], rec["position"], rec["mass"], G, 0.0)
        _cache[key] = (rec, tree, q6, A, exact)
    return _cache[key]


def test_tensors_equal_the_sums_over_member_bodies(nb):
    rec, tree, q6, A, _ = world(nb, 1001, 7)
    skip, order = tree["skip"], tree["order"]
    leaf = skip == np.arange(len(skip)) + 1
    before = np.concatenate([[0], np.cumsum(leaf)])       # leaves before node i = its first member's place in `order`
    x = rec["position"].astype(np.float64)
    m = rec["mass"].astype(np.float64)
    Q = q_matrix(q6)
    worst = 0.0
    for i in range(len(skip)):
        members = order[before[i]:before[skip[i]]]
        if leaf[i]:
            assert len(members) == 1 and not q6[i].any() and A[i] == 0.0
            continue
        d = x[members] - tree["com_mass"][i, :3].astype(np.float64)
        d2 = (d * d).sum(1)
        want = 3.0 * np.einsum("k,ka,kb->ab", m[members], d, d) - (m[members] * d2).sum() * np.eye(3)
        a_want = (m[members] * d2).sum()
        assert abs(A[i] - a_want) <= 1e-12 * a_want
        worst = max(worst, np.abs(Q[i] - want).max() / a_want)
        assert abs(np.trace(Q[i])) <= 1e-12 * a_want
    print(f"\n[quad list] bottom-up tensors against member sums: worst {worst:.2e} A")
    assert worst < 1e-12


def test_two_masses_on_an_axis():
    """Masses m at +-s on the x axis seen from distance R on it: the root's term is 2 g m / R^2 (1 + 3 s^2 / R^2), towards them."""
    m, s, R, g = 0.75, 0.5, 8.0, 1.5
    tree = dict(com_mass=np.array([[0, 0, 0, 2 * m], [-s, 0, 0, m], [s, 0, 0, m]], np.float32), width=np.array([64, 32, 32], np.float32),
                skip=np.array([3, 2, 3], np.int32))
    q6, A = node_quadrupoles(tree["com_mass"], tree["skip"])
    assert np.allclose(q6[0], [4 * m * s * s, 0, 0, -2 * m * s * s, 0, -2 * m * s * s], rtol=1e-15) and A[0] == 2 * m * s * s
    assert not q6[1:].any()
    for leaf in (0, 1):
        ref = walk_list_quad([[R, 0, 0]], tree, q6.astype(np.float32), g, 0.0, 100.0, leaf)   # w^2 = 4096 < 100 * 64: the root is accepted
        assert ref["accepted"][0] == 1 and ref["visited"][0] == 1
        want = 2 * g * m / R ** 2 * (1 + 3 * s * s / R ** 2)
        assert np.allclose(ref["S"][0], [-want, 0, 0], rtol=1e-14, atol=0)
        assert np.isclose(ref["T"][0], 2 * g * m / R ** 2 * (1 + 2 * s * s / R ** 2 + 5 * s * s / R ** 2), rtol=1e-14)


def test_theta2_zero_direct_is_the_direct_sum(nb):
    rec, tree, q6, _, _ = world(nb, 1001, 7)
    ref = walk_list_quad(rec["position"], tree, q6, G, 0.01, 0.0, 1)
    exact = direct_sum(rec["position"], rec["position"], rec["mass"], G, float(np.float32(np.float32(0.01) * np.float32(0.01))) ** 0.5)
    assert np.abs(ref["S"] - exact).max() <= 1e-12 * np.abs(exact).max()
    assert (ref["accepted"] == len(rec) - 1).all() and (ref["visited"] == len(tree["skip"])).all()


def violations(ref, a):
    return np.linalg.norm(a - ref["S"], axis=1) > QUAD_RTOL * ref["T"]


def test_wrong_quadrupole_walks_are_reported(nb):
    """A walk that negates Q, drops the factor 2.5, swaps xy and xz, or zeroes one accepted node's Q, seen through
    |a - S| <= R T: the share of bodies each mistake moves beyond the bound."""
    rec, tree, q6, _, _ = world(nb)
    q32 = q6.astype(np.float32)
    pos = rec["position"]
    for theta2 in (0.25, 1.0):
        ref = walk_list_quad(pos, tree, q32, G, 0.0, theta2, 1)
        assert not violations(ref, ref["S"]).any()
        wrong = {
            "Q negated": walk_list_quad(pos, tree, -q32, G, 0.0, theta2, 1)["S"],
            "2.5 dropped": walk_list_quad(pos, tree, q32, G, 0.0, theta2, 1, c2=1.0)["S"],
            "xy and xz swapped": walk_list_quad(pos, tree, q32[:, [0, 2, 1, 3, 4, 5]], G, 0.0, theta2, 1)["S"],
        }
        for name, a in wrong.items():
            share = violations(ref, a).mean()
            print(f"\n[quad list] theta2={theta2}: {name} -> {share:.1%} of bodies beyond R T")
            # every body accepts cells a few widths away: their quadrupole parts are ~1e-2 .. 1e-4 of T, far above R = QUAD_RTOL
            assert share > 0.99, name
        # one node: the internal node most bodies accept loses its tensor; the bodies that accept it are the ones that can tell
        internal = tree["skip"] != np.arange(len(tree["skip"])) + 1
        j = int(np.argmax(np.where(internal, ref["takers"], -1)))
        z = q32.copy()
        z[j] = 0
        bad = violations(ref, walk_list_quad(pos, tree, z, G, 0.0, theta2, 1)["S"])
        print(f"\n[quad list] theta2={theta2}: Q of node {j} zeroed -> {bad.sum()} of its {ref['takers'][j]} accepting bodies beyond R T")
        assert 0 < bad.sum() <= ref["takers"][j]


def test_f64_error_distributions(nb):
    """Monopole and quadrupole sums in f64 against the direct sum: the figures the GPU accuracy test compares with."""
    rec, tree, q6, _, exact = world(nb)
    zero = np.zeros_like(q6)
    got = {}
    for theta2 in (0.25, 1.0):
        for order, q in ((1, zero), (2, q6.astype(np.float32))):
            e = rel_errors(walk_list_quad(rec["position"], tree, q, G, 0.0, theta2, 1)["S"], exact)
            got[(order, theta2)] = (float(np.median(e)), float(np.percentile(e, 99)))
            print(f"\n[quad list] f64 order {order} theta2={theta2}: median {got[(order, theta2)][0]:.4e} p99 {got[(order, theta2)][1]:.4e}")
    for key, (med, p99) in got.items():
        assert np.isclose(med, F64_ERRORS[key][0], rtol=1e-3) and np.isclose(p99, F64_ERRORS[key][1], rtol=1e-3), (key, med, p99)
    for theta2 in (0.25, 1.0):   # (one more order in w / r: a factor 3.5 in the median at theta2 = 0.25, 1.6 at theta2 = 1 where w / r reaches 1)
        assert got[(2, theta2)][0] < got[(1, theta2)][0] and got[(2, theta2)][1] < got[(1, theta2)][1]
