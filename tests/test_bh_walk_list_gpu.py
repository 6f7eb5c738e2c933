"""The fast Barnes-Hut walks against the f64 sum of their own node list (tests/bh_list.py).

After every force pass the handle's tree is exported (Simulation.tree()) and oracle.bh_walk_list replays the walk's
opening tests over it for every body.  Asserted: (a) stats() accepted and visited totals equal the reference walk's
exactly; (b) |a_i - S_i| <= R T_i for every body; (c) the worst ratio is printed (pytest -s).  Covered, for f32 fast math on
host- and device-built trees and both leaf rules: k_bh_walk and k_bh_walk_duo (1 to 8 bodies per lane), the node-range
split (K = 1 .. 64, K above the node count, split points inside a deep chain of ancestors), k_bh_reduce and
k_bh_reduce_split, the kick fused into the reduction after compaction and unsynchronised steps, re-planning on one handle,
and the f64 fast walk (k_bh_walk_fast64 + k_bh_reduce64)."""
import numpy as np
import pytest

from bh_list import (BIG, G_SOFTS, KNOB_CASES, LIST_RTOL_F32, LIST_RTOL_F64, SIZES, THETA2S, ancestors, check_counts,
                     check_walk, split_first)

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
G = 1.0
LEAVES = ("reference", "direct")


def bodies(nb, n, seed, f64=False):
    """n Plummer records, all well inside BOX."""
    rec = nb.plummer(2 * n + 64, seed=seed, f64=f64)
    rec = rec[np.abs(rec["position"]).max(1) < 30.0][:n]
    assert len(rec) == n
    return np.ascontiguousarray(rec)


def fast_sim(nb, rec, tree, leaf, box=BOX, **tuning):
    return nb.Simulation(rec, *box, method=nb.BARNES_HUT, math_mode=nb.FAST,
                         tree_build=nb.TREE_DEVICE if tree == "device" else nb.TREE_HOST,
                         leaf_mode=nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE, tuning=tuning)


def report(what, worst):
    print(f"\n[node list] {what}: worst |a - S| / T {worst:.3e}")


def checked_forces(nb, orc, sim, leaf, theta2, g_soft, what):
    """One update_forces, checked against the node list of the tree it built; returns (worst, records, reference)."""
    sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
    sim.reset_stats()
    sim.update_forces()
    pts = sim.get_points()
    ref = orc.bh_walk_list(sim.tree(), pts["position"], theta2, G, g_soft, LEAVES.index(leaf), 16)
    check_counts(sim.stats(), ref, what)
    worst = check_walk(pts["acceleration"], ref, LIST_RTOL_F64 if sim.f64 else LIST_RTOL_F32, what)
    return worst, pts, ref


# ---------------------------------------------------------------------------------------------- update_forces
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_update_forces(gpu, orc, n, leaf, tree):
    nb = gpu
    with fast_sim(nb, bodies(nb, n, seed=n), tree, leaf) as sim:
        worst = 0.0
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                what = f"n={n} {tree} {leaf} theta2={theta2} g_soft={g_soft}"
                worst = max(worst, checked_forces(nb, orc, sim, leaf, theta2, g_soft, what)[0])
    report(f"update_forces n={n} {tree} {leaf}", worst)


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_update_forces_2p20(gpu, orc, leaf, tree):
    nb = gpu
    with fast_sim(nb, bodies(nb, BIG, seed=20250523), tree, leaf) as sim:
        worst = checked_forces(nb, orc, sim, leaf, 0.25, 0.01, f"2^20 {tree} {leaf}")[0]
    report(f"update_forces n=2^20 {tree} {leaf}", worst)


@pytest.mark.parametrize("case", range(len(KNOB_CASES)))
@pytest.mark.parametrize("tree", ["host", "device"])
def test_walk_knobs(gpu, orc, case, tree):
    """bh_walk_duo / bh_walk_split / bh_walk_xcd / bh_walk_order / bh_reduce_split (every value at least once: bh_list)."""
    nb = gpu
    knobs, n = KNOB_CASES[case]
    leaf = LEAVES[case % 2]
    with fast_sim(nb, bodies(nb, n, seed=7 + case), tree, leaf, **knobs) as sim:
        worst = max(checked_forces(nb, orc, sim, leaf, t2, 0.01, f"{knobs} n={n} {tree} {leaf} theta2={t2}")[0] for t2 in THETA2S)
    report(f"{knobs} n={n} {tree} {leaf}", worst)


# ---------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("duo", [0, 4])
@pytest.mark.parametrize("n", [2, 9, 20])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_more_segments_than_nodes(gpu, orc, n, tree, duo):
    """K = 64 pinned on a tree of fewer than 64 nodes: most segments are empty."""
    nb = gpu
    worst = 0.0
    for leaf in LEAVES:
        with fast_sim(nb, bodies(nb, n, seed=3), tree, leaf, bh_walk_split=64, bh_walk_duo=duo) as sim:
            for t2 in (0.25, 1.0):
                worst = max(worst, checked_forces(nb, orc, sim, leaf, t2, 0.0, f"K=64 n={n} {tree} {leaf}")[0])
            assert len(sim.tree()["width"]) < 64
    report(f"K=64 n={n} {tree} duo={duo}", worst)


def clump_world(nb, seed=11):
    """300 Plummer bodies and 700 in a cube of side 1e-5 around (1.3, -0.7, 0.4): they share ~22 levels of the tree."""
    rec = bodies(nb, 1000, seed=seed)
    rng = np.random.default_rng(seed)
    c = np.array([1.3, -0.7, 0.4])
    rec["position"][300:] = (c + rng.uniform(-0.5e-5, 0.5e-5, size=(700, 3))).astype(np.float32)
    rec["velocity"][300:] = 0.0
    return rec


@pytest.mark.parametrize("K", [7, 16, 64])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_split_points_inside_a_deep_chain(gpu, orc, K, tree):
    """Split points fall inside the clump's subtree: a segment's entry replays more than 21 ancestors (walk_entry)."""
    nb = gpu
    worst = 0.0
    for leaf in LEAVES:
        with fast_sim(nb, clump_world(nb), tree, leaf, bh_walk_split=K) as sim:
            for t2 in (0.25, 1.0):
                worst = max(worst, checked_forces(nb, orc, sim, leaf, t2, 0.0, f"clump K={K} {tree} {leaf}")[0])
            skip = sim.tree()["skip"]
            if tree == "host":   # the host lists the split points itself (equal parts of the node range)
                deepest = max(len(ancestors(skip, f)) for f in split_first(len(skip), K)[:-1])
                assert deepest > 21, deepest
    report(f"clump K={K} {tree}", worst)


@pytest.mark.parametrize("tree", ["host", "device"])
def test_nearly_coincident_bodies(gpu, orc, tree):
    """Pairs 3e-6 apart (r2 < 1e-10): DIRECT skips the partner's leaf whole, REFERENCE sees it fail the opening test."""
    nb = gpu
    rec = bodies(nb, 400, seed=5)
    rec["position"][200:] = rec["position"][:200] + np.float32(3e-6)
    worst = 0.0
    for leaf in LEAVES:
        with fast_sim(nb, rec, tree, leaf, bh_walk_split=16) as sim:
            for t2 in (0.25, 1.0):
                worst = max(worst, checked_forces(nb, orc, sim, leaf, t2, 0.01, f"pairs {tree} {leaf}")[0])
    report(f"nearly coincident pairs {tree}", worst)


@pytest.mark.parametrize("tree", ["host", "device"])
def test_theta2_zero(gpu, orc, tree):
    """theta2 = 0 accepts nothing: REFERENCE gives exactly zero; DIRECT is the sum over every other leaf, visiting every node."""
    nb = gpu
    n = 1001
    for leaf in LEAVES:
        with fast_sim(nb, bodies(nb, n, seed=9), tree, leaf) as sim:
            worst, pts, ref = checked_forces(nb, orc, sim, leaf, 0.0, 0.01, f"theta2=0 {tree} {leaf}")
            m = len(sim.tree()["width"])
            s = sim.stats()
            if leaf == "reference":
                assert s.interactions == 0 and not pts["acceleration"].any()
            else:
                # no centre of mass of a cell lies within 1e-5 of a body here: every body visits every node
                assert s.node_visits == n * m and s.interactions == n * (n - 1)
        report(f"theta2=0 {tree} {leaf}", worst)


@pytest.mark.parametrize("tree", ["host", "device"])
def test_huge_theta2_accepts_the_root(gpu, orc, tree):
    nb = gpu
    n = 4097
    for leaf in LEAVES:
        with fast_sim(nb, bodies(nb, n, seed=13), tree, leaf, bh_walk_split=7) as sim:
            worst, _, ref = checked_forces(nb, orc, sim, leaf, 1e30, 0.01, f"theta2=1e30 {tree} {leaf}")
            assert (ref["accepted"] == 1).all() and (ref["visited"] == 1).all()
        report(f"theta2=1e30 {tree} {leaf}", worst)


# ---------------------------------------------------------------------------------------------- steps
@pytest.mark.parametrize("plan", [dict(bh_walk_split=1), dict(bh_walk_split=8, bh_reduce_split=0),
                                  dict(bh_walk_split=16, bh_reduce_split=1), dict(bh_walk_split=8, bh_reduce_split=1, bh_walk_duo=3)])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_one_step_through_the_fused_kick(gpu, orc, tree, leaf, plan):
    """A few steps in a tight box (bodies escape: compaction; the device build runs them unsynchronised), then one more step:
    its walk positions are oracle.pre_force(records) retained in the box, bit for bit; the acceleration is checked against the
    node list of the tree that step built, and velocity and position equal oracle.after_force with that acceleration."""
    nb = gpu
    rec = nb.plummer(6000, seed=17)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 1.45])
    box = ((0.0, 0.0, 0.0), 2.92)   # (about 20 of 5 129 bodies leave it in 6 steps)
    dt = 0.05
    with fast_sim(nb, rec, tree, leaf, box=box, **plan) as sim:
        sim.settings = nb.Settings(G, 0.01, dt, 0.25)
        sim.steps(5)
        before = sim.get_points()
        assert len(before) < len(rec)   # bodies left the box
        walk = before.copy()
        orc.pre_force(walk, dt)
        walk = orc.retain(walk, *box).copy()
        sim.reset_stats()
        sim.step()
        after = sim.get_points()
        assert len(after) == len(walk)
        ref = orc.bh_walk_list(sim.tree(), walk["position"], 0.25, G, 0.01, LEAVES.index(leaf), 16)
        what = f"step {tree} {leaf} {plan}"
        check_counts(sim.stats(), ref, what)
        worst = check_walk(after["acceleration"], ref, what=what)
        want = walk.copy()
        want["acceleration"] = after["acceleration"]
        orc.after_force(want, dt)
        for k in ("velocity", "position", "mass"):
            assert np.array_equal(after[k].view(np.uint32), want[k].view(np.uint32)), f"{what}: {k}"
    report(what, worst)


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_replanning_on_one_handle(gpu, orc, tree, leaf):
    """K = 64 at 30 011 bodies, then K = 7 at 9 001 on the same handle (planes of the first pass stay in the buffer):
    checked, and bit-equal to a fresh handle."""
    nb = gpu
    big, small = bodies(nb, 30011, seed=21), bodies(nb, 9001, seed=22)
    with fast_sim(nb, big, tree, leaf, bh_walk_split=64, bh_walk_duo=2) as sim:
        w1 = checked_forces(nb, orc, sim, leaf, 0.25, 0.01, f"replan K=64 {tree} {leaf}")[0]
        sim.set_tuning("bh_walk_split", 7)
        sim.upload(small)
        w2, pts, _ = checked_forces(nb, orc, sim, leaf, 0.25, 0.01, f"replan K=7 {tree} {leaf}")
    with fast_sim(nb, small, tree, leaf, bh_walk_split=7, bh_walk_duo=2) as fresh:
        fresh.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        fresh.update_forces()
        assert np.array_equal(fresh.get_points()["acceleration"].view(np.uint32), pts["acceleration"].view(np.uint32))
    report(f"replan {tree} {leaf}", max(w1, w2))


# ---------------------------------------------------------------------------------------------- f64
@pytest.mark.parametrize("n", [1, 3, 65, 4097, 65536])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_f64_update_forces(gpu, orc, n, leaf, tree):
    nb = gpu
    with fast_sim(nb, bodies(nb, n, seed=n, f64=True), tree, leaf) as sim:
        assert sim.f64
        worst = 0.0
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                worst = max(worst, checked_forces(nb, orc, sim, leaf, theta2, g_soft, f"f64 n={n} {tree} {leaf} {theta2} {g_soft}")[0])
    report(f"f64 update_forces n={n} {tree} {leaf}", worst)


@pytest.mark.parametrize("knobs", [dict(bh_walk_split=1, bh_walk_duo=0), dict(bh_walk_split=7, bh_walk_duo=2),
                                   dict(bh_walk_split=16, bh_walk_duo=3, bh_walk_xcd=0), dict(bh_walk_split=64, bh_walk_duo=8)])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_f64_walk_knobs(gpu, orc, knobs, tree):
    nb = gpu
    worst = 0.0
    for leaf in LEAVES:
        with fast_sim(nb, bodies(nb, 30011, seed=31, f64=True), tree, leaf, **knobs) as sim:
            worst = max(worst, checked_forces(nb, orc, sim, leaf, 0.25, 0.01, f"f64 {knobs} {tree} {leaf}")[0])
    report(f"f64 {knobs} {tree}", worst)


@pytest.mark.parametrize("tree", ["host", "device"])
def test_f64_edges(gpu, orc, tree):
    """f64: K = 64 on a 20-node tree, theta2 = 0 and a huge theta2."""
    nb = gpu
    worst = 0.0
    for leaf in LEAVES:
        with fast_sim(nb, bodies(nb, 9, seed=3, f64=True), tree, leaf, bh_walk_split=64) as sim:
            worst = max(worst, checked_forces(nb, orc, sim, leaf, 0.25, 0.0, f"f64 K=64 {tree} {leaf}")[0])
        with fast_sim(nb, bodies(nb, 1001, seed=9, f64=True), tree, leaf) as sim:
            for t2 in (0.0, 1e30):
                w, pts, ref = checked_forces(nb, orc, sim, leaf, t2, 0.01, f"f64 theta2={t2} {tree} {leaf}")
                worst = max(worst, w)
                if t2 == 0.0 and leaf == "reference":
                    assert not pts["acceleration"].any()
                if t2 == 1e30:
                    assert (ref["accepted"] == 1).all()
    report(f"f64 edges {tree}", worst)
