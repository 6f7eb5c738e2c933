"""The quadrupole force walk (nbody_set_multipole(h, 2): k_tree_quad + k_bh_walk_quad) against tests/quad_list.py.

After a force pass the handle's tree and tensors are exported.  Asserted, for both tree builds and both leaf rules:
(1) every exported tensor is within Rq A_i of node_quadrupoles on the exported tree, leaves exactly zero; (2) |a_i - S_i| <=
R T_i for every body, S and T from walk_list_quad over the exported tree and tensors; (3) stats() accepted and visited totals
equal the checker's, and those of a monopole handle on the same points with the same build (the host build makes the same
tree bit for bit every time; the device build is compared with a device-built monopole handle, because its centres of mass
differ from the host build's in the last bits and with them a few opening tests: include/nbody_hip.h NBODY_TREE_DEVICE);
(4) the node-range split and both plane reductions; (5) one step through the fused kick; (6) enqueued steps; (7) the errors
against the f64 direct sum; (8) the setting leaves no trace, is cloned, and is refused where it does not apply.
Every worst figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from quad_list import (ACCURACY_MARGIN, ACCURACY_N, F64_ERRORS, QUAD_RTOL, QUAD_TENSOR_RTOL, direct_sum, node_quadrupoles,
                       plummer_bodies, rel_errors, tensor_errors, walk_list_quad)

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
G = 1.0
LEAVES = ("reference", "direct")
SIZES = (1, 2, 3, 9, 65, 1001, 4097)
THETA2S = (0.25, 1.0)
G_SOFTS = (0.0, 0.01)


def fast_sim(nb, rec, tree, leaf, box=BOX, multipole=2, **tuning):
    sim = nb.Simulation(rec, *box, method=nb.BARNES_HUT, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if tree == "device" else nb.TREE_HOST,
                        leaf_mode=nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE, tuning=tuning)
    sim.multipole = multipole
    return sim


def check_tensors(tree, q6, what):
    """(1): returns the worst |Q_dev - Q| / A."""
    want, A = node_quadrupoles(tree["com_mass"], tree["skip"])
    leaf = tree["skip"] == np.arange(len(A)) + 1
    err = tensor_errors(q6, want, A)
    worst = float(err.max()) if len(err) else 0.0
    print(f"\n[quadrupole] {what}: worst |Q_dev - Q| / A {worst:.3e}")
    assert not q6[leaf].any(), f"{what}: a leaf with a tensor"
    assert worst <= QUAD_TENSOR_RTOL, f"{what}: {np.count_nonzero(~(err <= QUAD_TENSOR_RTOL))} nodes beyond {QUAD_TENSOR_RTOL:g} A"
    return worst


def check_bodies(acc, ref, what):
    """(2): returns the worst |a - S| / T."""
    a = np.asarray(acc, np.float64)
    num = np.linalg.norm(a - ref["S"], axis=1)
    T = ref["T"]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(T > 0, num / np.where(T > 0, T, 1.0), np.where(num == 0, 0.0, np.inf))
    err[~np.isfinite(a).all(1)] = np.inf
    worst = float(err.max()) if len(err) else 0.0
    print(f"\n[quadrupole] {what}: worst |a - S| / T {worst:.3e}")
    assert worst <= QUAD_RTOL, f"{what}: {np.count_nonzero(~(err <= QUAD_RTOL))} of {len(err)} bodies beyond {QUAD_RTOL:g} T"
    return worst


def checked_forces(nb, sim, leaf, theta2, g_soft, what, ref=None):
    """One update_forces with quadrupoles, checks (1) (2) and the checker's counts; returns (records, reference, counts)."""
    sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
    sim.reset_stats()
    sim.update_forces()
    pts = sim.get_points()
    tree, q6 = sim.tree(), sim.tree_quadrupoles()
    assert q6.shape == (len(tree["skip"]), 6)
    if ref is None:
        check_tensors(tree, q6, what)
        ref = walk_list_quad(pts["position"], tree, q6, G, g_soft, theta2, LEAVES.index(leaf))
        ref["tree"], ref["q6"] = tree, q6
    else:   # a reference shared between handles: they must have built the same tree and tensors
        assert all(np.array_equal(tree[k].view(np.uint32), ref["tree"][k].view(np.uint32)) for k in tree) and np.array_equal(q6.view(np.uint32), ref["q6"].view(np.uint32))
    s = sim.stats()
    counts = (s.interactions, s.node_visits)
    assert counts == (int(ref["accepted"].sum()), int(ref["visited"].sum())), f"{what}: counters {counts} against the checker's"
    check_bodies(pts["acceleration"], ref, what)
    return pts, ref, counts


def monopole_counts(nb, sim, theta2, g_soft):
    sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
    sim.reset_stats()
    sim.update_forces()
    s = sim.stats()
    return (s.interactions, s.node_visits)


# ---------------------------------------------------------------------------------------------- (1) (2) (3)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_update_forces(gpu, n, leaf, tree):
    nb = gpu
    rec = plummer_bodies(nb, n, seed=n)
    with fast_sim(nb, rec, tree, leaf) as sim, fast_sim(nb, rec, tree, leaf, multipole=1) as mono:
        assert sim.multipole == nb.MULTIPOLE_QUADRUPOLE and mono.multipole == nb.MULTIPOLE_MONOPOLE
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                what = f"n={n} {tree} {leaf} theta2={theta2} g_soft={g_soft}"
                _, _, counts = checked_forces(nb, sim, leaf, theta2, g_soft, what)
                assert counts == monopole_counts(nb, mono, theta2, g_soft), f"{what}: counters differ from the monopole handle's"


def clump_world(nb, seed=11):
    """tests/test_bh_walk_list_gpu.py's: 300 Plummer bodies and 700 in a cube of side 1e-5 around (1.3, -0.7, 0.4)."""
    rec = plummer_bodies(nb, 1000, seed=seed)
    rng = np.random.default_rng(seed)
    c = np.array([1.3, -0.7, 0.4])
    rec["position"][300:] = (c + rng.uniform(-0.5e-5, 0.5e-5, size=(700, 3))).astype(np.float32)
    rec["velocity"][300:] = 0.0
    return rec


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_clump(gpu, leaf, tree):
    """Cells 1e-5 wide inside a box of 64: tensors of ~1e-13 beside ones of ~1, accepted from 1e-5 away."""
    nb = gpu
    rec = clump_world(nb)
    with fast_sim(nb, rec, tree, leaf) as sim, fast_sim(nb, rec, tree, leaf, multipole=1) as mono:
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                what = f"clump {tree} {leaf} theta2={theta2} g_soft={g_soft}"
                _, _, counts = checked_forces(nb, sim, leaf, theta2, g_soft, what)
                assert counts == monopole_counts(nb, mono, theta2, g_soft), what


# ---------------------------------------------------------------------------------------------- (4)
@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_segments(gpu, n, tree):
    """bh_walk_split 1, 7, 16, 64 (at n = 65 more segments than nodes would allow equal parts of 16) x bh_reduce_split 0, 1:
    the same tree and tensors, so one reference serves all eight handles."""
    nb = gpu
    rec = plummer_bodies(nb, n, seed=n + 1)
    for leaf in LEAVES:
        ref = None
        for K in (1, 7, 16, 64):
            for rs in (0, 1):
                with fast_sim(nb, rec, tree, leaf, bh_walk_split=K, bh_reduce_split=rs) as sim:
                    _, ref, _ = checked_forces(nb, sim, leaf, 0.25, 0.01, f"n={n} {tree} {leaf} K={K} reduce_split={rs}", ref)


# ---------------------------------------------------------------------------------------------- (5)
@pytest.mark.parametrize("plan", [dict(bh_walk_split=1), dict(bh_walk_split=8, bh_reduce_split=0), dict(bh_walk_split=16, bh_reduce_split=1)])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_one_step_through_the_fused_kick(gpu, orc, tree, leaf, plan):
    """As tests/test_bh_walk_list_gpu.py: a few steps in a tight box (bodies escape; the device build runs them without
    read-back), then one more step: it walks oracle.pre_force(records) retained in the box; its acceleration is checked against
    the node list of the tree that step built, and velocity and position equal oracle.after_force with that acceleration."""
    nb = gpu
    rec = nb.plummer(6000, seed=17)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 1.45])
    box = ((0.0, 0.0, 0.0), 2.92)
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
        tree_, q6 = sim.tree(), sim.tree_quadrupoles()
        what = f"step {tree} {leaf} {plan}"
        check_tensors(tree_, q6, what)
        ref = walk_list_quad(walk["position"], tree_, q6, G, 0.01, 0.25, LEAVES.index(leaf))
        s = sim.stats()
        assert (s.interactions, s.node_visits) == (int(ref["accepted"].sum()), int(ref["visited"].sum())), what
        check_bodies(after["acceleration"], ref, what)
        want = walk.copy()
        want["acceleration"] = after["acceleration"]
        orc.after_force(want, dt)
        for k in ("velocity", "position", "mass"):
            assert np.array_equal(after[k].view(np.uint32), want[k].view(np.uint32)), f"{what}: {k}"


# ---------------------------------------------------------------------------------------------- (6)
@pytest.mark.parametrize("leaf", LEAVES)
def test_enqueued_steps_equal_single_steps(gpu, leaf):
    nb = gpu
    rec = plummer_bodies(nb, 4097, seed=23)
    out = []
    for enqueue in (True, False):
        with fast_sim(nb, rec, "device", leaf) as sim:
            sim.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
            if enqueue:
                sim.steps(3)
            else:
                for _ in range(3):
                    sim.step_by(1e-3)
            out.append(sim.get_points())
            assert sim.stats().steps == 3
    for k in ("position", "velocity", "acceleration"):
        assert np.array_equal(out[0][k].view(np.uint32), out[1][k].view(np.uint32)), k
    assert out[0]["acceleration"].any()


# ---------------------------------------------------------------------------------------------- (7)
def test_accuracy_against_the_direct_sum(gpu):
    """n = 4097, theta2 = 1, g_soft = 0, NBODY_LEAF_DIRECT, host build (the tree of tests/test_quad_list_checker.py): order 2
    beats order 1 on the same handle in the median and the 99th percentile, and its median is the CPU f64 walk's up to the f32
    rounding of the terms."""
    nb = gpu
    rec = plummer_bodies(nb, ACCURACY_N, seed=ACCURACY_N)
    exact = direct_sum(rec["position"], rec["position"], rec["mass"], G, 0.0)
    got = {}
    with fast_sim(nb, rec, "host", "direct") as sim:
        sim.settings = nb.Settings(G, 0.0, 1e-3, 1.0)
        for order in (2, 1):
            sim.multipole = order
            sim.update_forces()
            e = rel_errors(sim.get_points()["acceleration"], exact)
            got[order] = (float(np.median(e)), float(np.percentile(e, 99)))
            print(f"\n[quadrupole] order {order}: median {got[order][0]:.4e} p99 {got[order][1]:.4e}")
    cpu = F64_ERRORS[(2, 1.0)][0]
    print(f"\n[quadrupole] GPU median / CPU f64 median {got[2][0] / cpu:.5f}")
    assert got[2][0] < got[1][0] and got[2][1] < got[1][1]
    assert got[2][0] <= ACCURACY_MARGIN * cpu


# ---------------------------------------------------------------------------------------------- (8)
@pytest.mark.parametrize("tree", ["host", "device"])
def test_back_to_monopole_leaves_no_trace(gpu, tree):
    nb = gpu
    rec = plummer_bodies(nb, 4097, seed=29)
    with fast_sim(nb, rec, tree, "direct", multipole=1) as plain, fast_sim(nb, rec, tree, "direct") as sim:
        for s in (plain, sim):
            s.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        plain.update_forces()
        sim.update_forces()
        a2 = sim.get_points()["acceleration"]
        sim.tree_quadrupoles()
        sim.multipole = 1
        sim.update_forces()
        a1 = sim.get_points()["acceleration"]
        want = plain.get_points()["acceleration"]
        assert np.array_equal(a1.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(a2.view(np.uint32), want.view(np.uint32))
        with pytest.raises(nb.NbodyError) as e:   # the last pass was a monopole pass
            sim.tree_quadrupoles()
        assert e.value.code == nb.NBODY_ERR_INVALID
        sim.steps(2)
        plain.steps(2)
        for k in ("position", "velocity", "acceleration"):
            assert np.array_equal(sim.get_points()[k].view(np.uint32), plain.get_points()[k].view(np.uint32)), k


def test_clone_carries_the_order(gpu):
    nb = gpu
    rec = plummer_bodies(nb, 1001, seed=31)
    with fast_sim(nb, rec, "device", "direct") as sim:
        sim.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        sim.step()
        with sim.clone() as twin:
            assert twin.multipole == nb.MULTIPOLE_QUADRUPOLE
            sim.step()
            twin.step()
            for k in ("position", "velocity", "acceleration"):
                assert np.array_equal(sim.get_points()[k].view(np.uint32), twin.get_points()[k].view(np.uint32)), k
            assert twin.tree_quadrupoles().any()


def test_refusals(gpu):
    nb = gpu
    rec = plummer_bodies(nb, 65, seed=37)
    kw = dict(method=nb.BARNES_HUT, math_mode=nb.FAST)
    refused = {
        "brute force": lambda: nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST),
        "f64": lambda: nb.Simulation(rec.astype(nb.PARTICLE_DTYPE64), *BOX, **kw),
        "strict math": lambda: nb.Simulation(rec, *BOX, method=nb.BARNES_HUT, math_mode=nb.STRICT),
        "sharded": lambda: nb.Simulation(rec, *BOX, rank=0, world_size=2, **kw),
        "spatial": lambda: nb.Simulation(rec, *BOX, shard_mode=nb.SHARD_SPATIAL, **kw),
    }
    for name, make in refused.items():
        with make() as sim:
            with pytest.raises(nb.NbodyError) as e:
                sim.multipole = nb.MULTIPOLE_QUADRUPOLE
            assert e.value.code == nb.NBODY_ERR_INVALID, name
            assert "nbody_set_multipole" in str(e.value), name
            assert sim.multipole == nb.MULTIPOLE_MONOPOLE
            sim.multipole = nb.MULTIPOLE_MONOPOLE   # (the default is accepted everywhere)
    with nb.Simulation(rec, *BOX, **kw) as sim:
        for order in (0, 3, -1):
            with pytest.raises(nb.NbodyError) as e:
                sim.multipole = order
            assert e.value.code == nb.NBODY_ERR_INVALID
        with pytest.raises(nb.NbodyError) as e:   # no force pass yet
            sim.tree_quadrupoles()
        assert e.value.code == nb.NBODY_ERR_INVALID
        sim.update_forces()
        with pytest.raises(nb.NbodyError):        # a monopole pass
            sim.tree_quadrupoles()
