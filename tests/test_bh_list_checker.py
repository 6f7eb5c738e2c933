"""The node-list checker of tests/bh_list.py, on the CPU: the reference walk (oracle.bh_walk_list) makes the oracle's own
opening tests (its accepted and visited totals equal bh_update_forces'), the oracle's f32 accelerations pass
check_walk, and the errors a fast walk could make for ONE body -- a node dropped, doubled or applied with its parent's
mass, a segment's share lost, two bodies' results swapped -- fail it.  The share of (body, node) terms that are
individually detectable (|t_ij| > 2 R T_i) at 65 536 bodies is printed (pytest -s) and bounded below."""
import numpy as np
import pytest

from bh_list import (LIST_RTOL_F32, check_walk, knob_coverage, parent, split_first, terms, walk_errors)

BOX = ((0.0, 0.0, 0.0), 64.0)
G, EPS = 1.0, 0.01
_cache = {}


def world(nb, orc, n, leaf, theta2=0.25, seed=20250523):
    """(records with the oracle's f32 accelerations, the oracle's tree, the reference walk, oracle counts)."""
    key = (n, leaf, theta2, seed)
    if key not in _cache:
        rec = nb.plummer(n, seed=seed).astype(orc.P32)
        counts = orc.bh_update_forces(rec, dict(g=G, g_soft=EPS, dt=1e-3, theta2=theta2), *BOX, threads=16, leaf_mode=leaf)
        tree = orc.bh_build_tree(rec, *BOX)
        ref = orc.bh_walk_list(tree, rec["position"], theta2, G, EPS, leaf, 16)
        _cache[key] = (rec, tree, ref, counts)
    return _cache[key]


def body_terms(orc, tree, p, theta2, leaf):
    """(accepted node indices, their f64 terms) of one body at p."""
    nodes = orc.bh_walk_list(tree, np.asarray(p).reshape(1, 3), theta2, G, EPS, leaf, 1, list_body=0)["list"]
    return nodes, terms(tree, p, nodes, G, EPS)


@pytest.mark.parametrize("leaf", [0, 1])
@pytest.mark.parametrize("n,theta2", [(1, 0.25), (2, 0.25), (3, 1.0), (64, 0.25), (1001, 1.0), (1001, 0.0), (20000, 0.25),
                                      (20000, 4.0), (65536, 0.25)])
def test_reference_walk_makes_the_oracles_decisions(nb, orc, n, theta2, leaf):
    _, tree, ref, (acc_n, vis_n) = world(nb, orc, n, leaf, theta2)
    assert (int(ref["accepted"].sum()), int(ref["visited"].sum())) == (acc_n, vis_n)
    if theta2 == 0.0 and leaf == 0:
        assert acc_n == 0 and not ref["S"].any() and not ref["T"].any()


@pytest.mark.parametrize("leaf", [0, 1])
@pytest.mark.parametrize("n,theta2", [(3, 1.0), (1001, 0.25), (20000, 4.0), (65536, 0.25), (65536, 1.0)])
def test_oracle_accelerations_pass(nb, orc, n, theta2, leaf):
    rec, _, ref, _ = world(nb, orc, n, leaf, theta2)
    worst = check_walk(rec["acceleration"], ref, what="oracle")
    print(f"\n[node list] oracle f32 n={n} theta2={theta2} leaf={leaf}: worst |a - S| / T {worst:.2e}")
    assert worst < LIST_RTOL_F32 / 2


def one_body(acc, i, delta):
    a = np.asarray(acc, np.float64).copy()
    a[i] += delta
    return a


@pytest.mark.parametrize("leaf", [0, 1])
def test_single_corruptions_fail(nb, orc, leaf):
    n, theta2 = 65536, 0.25
    rec, tree, ref, _ = world(nb, orc, n, leaf, theta2)
    acc = rec["acceleration"]
    pos = rec["position"]
    r = np.linalg.norm(pos.astype(np.float64), axis=1)
    # a central body (most cancellation), a median one and a halo body
    for i in (int(np.argmin(r)), int(np.argsort(r)[n // 2]), int(np.argmax(r))):
        nodes, t = body_terms(orc, tree, pos[i], theta2, leaf)
        mag = np.linalg.norm(t, axis=1)
        T = ref["T"][i]
        assert np.isclose(mag.sum(), T, rtol=1e-12) and np.allclose(t.sum(0), ref["S"][i], rtol=0, atol=1e-12 * T)
        above = np.flatnonzero(mag > 2 * LIST_RTOL_F32 * T)
        assert len(above), "no detectable term"
        j_big = int(np.argmax(mag))
        j_edge = int(above[np.argmin(mag[above])])   # just above the threshold: the weakest term the check must see
        k = int(nodes[j_edge])
        m_par = float(tree["com_mass"][parent(tree["skip"], k), 3]) if k > 0 else None
        cases = [("largest dropped", -t[j_big]), ("threshold term dropped", -t[j_edge]), ("threshold term doubled", t[j_edge])]
        if m_par is not None:
            cases.append(("parent's mass", t[j_edge] * (m_par / float(tree["com_mass"][k, 3]) - 1.0)))
        for name, d in cases:
            bad = one_body(acc, i, d)
            err = walk_errors(bad, ref)
            assert np.count_nonzero(err > LIST_RTOL_F32) == 1, name
            with pytest.raises(AssertionError):
                check_walk(bad, ref, what=name)
            print(f"\n[node list] leaf={leaf} body {i}: {name} -> {err[i] / LIST_RTOL_F32:.1f} R")
    # two bodies' results swapped
    bad = np.asarray(acc, np.float64).copy()
    bad[[5, 6]] = bad[[6, 5]]
    with pytest.raises(AssertionError):
        check_walk(bad, ref, what="swap")


@pytest.mark.parametrize("K", [8, 16])
def test_dropped_segment_share_fails(nb, orc, K):
    """A body group of 64 neighbours in space (one wave of the tree order) loses what one of K segments added."""
    n, theta2, leaf = 65536, 0.25, 0
    rec, tree, ref, _ = world(nb, orc, n, leaf, theta2)
    pos = rec["position"].astype(np.float64)
    group = np.argsort(np.linalg.norm(pos - pos[123], axis=1))[:64]
    first = split_first(len(tree["width"]), K)
    bad = np.asarray(rec["acceleration"], np.float64).copy()
    seg = K // 2
    for i in group:
        nodes, t = body_terms(orc, tree, rec["position"][i], theta2, leaf)
        bad[i] -= t[(nodes >= first[seg]) & (nodes < first[seg + 1])].sum(0)
    err = walk_errors(bad, ref)
    hit = int(np.count_nonzero(err[group] > LIST_RTOL_F32))
    print(f"\n[node list] segment {seg} of {K} dropped for 64 bodies: {hit} fail")
    assert hit >= 32
    with pytest.raises(AssertionError):
        check_walk(bad, ref, what="segment")


def test_detectable_share(nb, orc):
    """The share of accepted (body, node) terms above 2 R T_i at 65 536 bodies (a random sample of 400 bodies)."""
    n, theta2 = 65536, 0.25
    for leaf in (0, 1):
        rec, tree, ref, _ = world(nb, orc, n, leaf, theta2)
        tot = det = 0
        for i in np.random.default_rng(1).choice(n, 400, replace=False):
            _, t = body_terms(orc, tree, rec["position"][i], theta2, leaf)
            mag = np.linalg.norm(t, axis=1)
            det += int(np.count_nonzero(mag > 2 * LIST_RTOL_F32 * ref["T"][i]))
            tot += len(mag)
        share = det / tot
        print(f"\n[node list] leaf={leaf}: {share:.1%} of {tot} terms individually detectable at R = {LIST_RTOL_F32:g}")
        assert share > 0.65


def test_knob_cases_cover_every_value():
    assert knob_coverage() == {}
