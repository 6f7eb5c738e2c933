"""nbody_potentials / nbody_field_at / nbody_energy_world in NBODY_POTENTIAL_TREE_QUADRUPOLE (k_bh_pot_walk_quad,
k_bh_field_walk_quad) against tests/quad_pot_list.py: the replay of the DIRECT walk over the tree and the tensors the call
itself built.  Counts exact and equal to mode TREE's, every body and probe within the derived bounds, the tensors within
quad_list's bound; mode TREE's bits at theta2 = 0; nbody_field_at's contracts; the clump world; consistency with the quadrupole
force walk; accuracy against PAIRS; the energy; no trace in later steps; refusals.  Worst ratios are printed (pytest -s) and
recorded in quad_pot_list.WORST_OBSERVED."""
import numpy as np
import pytest

import quad_pot_list as qp
from quad_list import ACCURACY_MARGIN, QUAD_RTOL, QUAD_TENSOR_RTOL, node_quadrupoles, plummer_bodies, tensor_errors, walk_list_quad

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
G = 1.0
SIZES = (1, 2, 3, 9, 65, 1001, 4097)
THETA2S = (0.25, 1.0)
G_SOFTS = (0.0, 0.01)
BATCH = 65536   # probes per batch (nbody_handle.h kFieldBatch)
TREES = ("host", "device")


def bh_sim(nb, rec, tree, math="fast", leaf="reference", box=BOX, **tuning):
    return nb.Simulation(rec, *box, method=nb.BARNES_HUT, math_mode=nb.FAST if math == "fast" else nb.STRICT,
                         tree_build=nb.TREE_DEVICE if tree == "device" else nb.TREE_HOST,
                         leaf_mode=nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE, tuning=tuning)


def probe_mix(rec, seed, n_own=1001, n_random=1000, n_outside=200):
    """tests/test_field_gpu.py's kinds of probes: body positions | a 10^3 grid over the box | uniform random points | points outside the box"""
    rng = np.random.default_rng(seed)
    g = (np.arange(10) + 0.5) * 6.4 - 32.0
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out = rng.uniform(33.0, 300.0, (n_outside, 3)) * rng.choice([-1.0, 1.0], (n_outside, 3))
    return np.concatenate([rec["position"][:n_own].astype(np.float64), grid, rng.uniform(-32, 32, (n_random, 3)), out])


def clump_world(nb, seed=11):
    """tests/test_bh_quadrupole_gpu.py's: 300 Plummer bodies and 700 in a cube of side 1e-5 around (1.3, -0.7, 0.4)."""
    rec = plummer_bodies(nb, 1000, seed=seed)
    rng = np.random.default_rng(seed)
    c = np.array([1.3, -0.7, 0.4])
    rec["position"][300:] = (c + rng.uniform(-0.5e-5, 0.5e-5, size=(700, 3))).astype(np.float32)
    rec["velocity"][300:] = 0.0
    return rec


def same_tree(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("com_mass", "width", "skip"))


def check_tensors(tree, q6, what):
    want, A = node_quadrupoles(tree["com_mass"], tree["skip"])
    leaf = tree["skip"] == np.arange(len(A)) + 1
    err = tensor_errors(q6, want, A)
    worst = float(err.max()) if len(err) else 0.0
    assert not q6[leaf].any(), f"{what}: a leaf with a tensor"
    assert worst <= QUAD_TENSOR_RTOL, f"{what}: worst |Q_dev - Q| / A {worst:.3e}"


def potentials_checked(nb, sim, theta2, g_soft, what, Ks=(1, 7, 64)):
    """potentials(2) with the split pinned to each K (0: automatic) against the replay of the tree and tensors the call built;
    counts also against potentials(TREE) on the same handle.  Returns (worst ratio, phi of the last K, reference)."""
    sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
    pos = sim.get_points()["position"]
    ref, first, worst = None, None, 0.0
    for K in Ks:
        sim.set_tuning("bh_walk_split", K)
        phi, counts = sim.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)
        tree, q6 = sim.tree(), sim.tree_quadrupoles()
        if ref is None:
            check_tensors(tree, q6, what)
            ref, first = qp.replay(tree, pos, q6, theta2, g_soft), (tree, q6)
        else:
            assert same_tree(tree, first[0]) and np.array_equal(q6.view(np.uint32), first[1].view(np.uint32))
        worst = max(worst, qp.check(None, phi, counts, ref, G, f"{what} K={K}")[1])
        _, mono_counts = sim.potentials(nb.POTENTIAL_TREE)
        assert counts == mono_counts, f"{what} K={K}: counts {counts}, mode TREE's {mono_counts}"
    return worst, phi, ref


def field_checked(nb, sim, pts, theta2, g_soft, what, Ks=(7, 0)):
    sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
    ref, worst = None, (0.0, 0.0)
    for K in Ks:
        sim.set_tuning("bh_walk_split", K)
        acc, phi, counts = sim.field_at(pts, nb.POTENTIAL_TREE_QUADRUPOLE)
        tree, q6 = sim.tree(), sim.tree_quadrupoles()
        if ref is None:
            check_tensors(tree, q6, what)
            ref = qp.replay(tree, pts, q6, theta2, g_soft)
        w = qp.check(acc, phi, counts, ref, G, f"{what} K={K}")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        assert sim.field_at(pts, nb.POTENTIAL_TREE, acc=False, phi=False)[2] == counts, f"{what} K={K}: counts differ from mode TREE's"
    return worst, (acc, phi, counts), ref


def report(what, worst):
    print(f"\n[quadrupole potentials] {what}: worst error / bound {worst}")


# ---------------------------------------------------------------------------------------------- 1. potentials(2)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tree", TREES)
def test_potentials_against_the_node_list(gpu, tree, n):
    nb = gpu
    rec = plummer_bodies(nb, n, seed=n)
    worst = 0.0
    with bh_sim(nb, rec, tree, leaf="reference") as a, bh_sim(nb, rec, tree, leaf="direct", bh_walk_split=7) as b:
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                w, phi, _ = potentials_checked(nb, a, theta2, g_soft, f"n={n} {tree} theta2={theta2} g_soft={g_soft}", (1, 64, 7))
                worst = max(worst, w)
                b.settings = nb.Settings(G, g_soft, 1e-3, theta2)
                phi_b, _ = b.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)   # the handle's leaf_mode makes no difference (K = 7 on both)
                assert np.array_equal(phi, phi_b)
    report(f"potentials n={n} {tree}", f"phi {worst:.3e}")


@pytest.mark.parametrize("tree", TREES)
def test_potentials_on_a_strict_math_handle(gpu, tree):
    nb = gpu
    rec = plummer_bodies(nb, 4097, seed=2)
    with bh_sim(nb, rec, tree, math="strict") as sim, bh_sim(nb, rec, tree, math="fast") as fast:
        worst, phi, _ = potentials_checked(nb, sim, 0.25, 0.01, f"strict {tree}", (0,))   # (0: the automatic split)
        fast.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        assert np.array_equal(fast.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)[0], phi)     # math_mode has no influence
    report(f"potentials strict {tree}", f"phi {worst:.3e}")


# ---------------------------------------------------------------------------------------------- 2. field_at(points, 2)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tree", TREES)
def test_field_against_the_node_list(gpu, tree, n):
    nb = gpu
    rec = plummer_bodies(nb, n, seed=n)
    pts = probe_mix(rec, seed=n)
    worst = (0.0, 0.0)
    with bh_sim(nb, rec, tree) as sim:
        for theta2 in THETA2S:
            for g_soft in G_SOFTS:
                w, _, _ = field_checked(nb, sim, pts, theta2, g_soft, f"n={n} {tree} theta2={theta2} g_soft={g_soft}")
                worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    report(f"field_at n={n} {tree}", f"acc {worst[0]:.3e} phi {worst[1]:.3e}")


@pytest.mark.parametrize("tree", TREES)
def test_field_contracts(gpu, tree):
    """acc-only and phi-only calls, repetition, permutation, a non-finite probe, a probe beyond the number range, no probes."""
    nb = gpu
    md = nb.POTENTIAL_TREE_QUADRUPOLE
    rec = plummer_bodies(nb, 1001, seed=6)
    rng = np.random.default_rng(8)
    pts = probe_mix(rec, seed=1)
    with bh_sim(nb, rec, tree) as sim:
        sim.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        acc, phi, counts = sim.field_at(pts, md)
        a2, p2, c2 = sim.field_at(pts, md)
        assert np.array_equal(acc, a2) and np.array_equal(phi, p2) and counts == c2
        perm = rng.permutation(len(pts))
        a3, p3, c3 = sim.field_at(pts[perm], md)
        assert np.array_equal(a3, acc[perm]) and np.array_equal(p3, phi[perm]) and c3 == counts
        a4, none, c4 = sim.field_at(pts, md, phi=False)
        assert none is None and np.array_equal(a4, acc) and c4 == counts
        none, p5, c5 = sim.field_at(pts, md, acc=False)
        assert none is None and np.array_equal(p5, phi) and c5 == counts
        none, none2, c6 = sim.field_at(pts, md, acc=False, phi=False)
        assert none is None and none2 is None and c6 == counts
        # a non-finite probe gets NaN, its neighbours keep their bits
        bad = pts.copy()
        where = [5, 77, 300]
        bad[5, 1], bad[77, 0], bad[300] = np.nan, np.inf, (-np.inf, np.nan, 1e300)
        a7, p7, _ = sim.field_at(bad, md)
        ok = np.ones(len(pts), bool)
        ok[where] = False
        assert np.array_equal(a7[ok], acc[ok]) and np.array_equal(p7[ok], phi[ok])
        assert np.isnan(a7[where]).all() and np.isnan(p7[where]).all()
        # a finite probe from which r2 overflows: exact zeros, its neighbours keep their bits
        far = pts.copy()
        far[40] = (1e30, -1e30, 1e30)
        far[41] = (1e30, 0.0, 0.0)
        a8, p8, _ = sim.field_at(far, md)
        assert not a8[40:42].any() and not p8[40:42].any()
        ok = np.ones(len(pts), bool)
        ok[40:42] = False
        assert np.array_equal(a8[ok], acc[ok]) and np.array_equal(p8[ok], phi[ok])
        # no probes: valid, the tree is built all the same
        a9, p9, c9 = sim.field_at(np.zeros((0, 3)), md)
        assert a9.shape == (0, 3) and p9.shape == (0,) and c9 == (0, 0) and len(sim.tree_quadrupoles()) == len(sim.tree()["skip"]) > 0


def test_field_in_two_batches(gpu):
    """65 536 + 100 probes against 1001 bodies: the bits of the same probes sent in two calls (the split pinned: a call draws
    its segment count from its first batch), and within the bounds."""
    nb = gpu
    md = nb.POTENTIAL_TREE_QUADRUPOLE
    rec = plummer_bodies(nb, 1001, seed=12)
    rng = np.random.default_rng(13)
    pts = np.concatenate([probe_mix(rec, seed=2), rng.uniform(-40, 40, (BATCH + 100 - 3201, 3))])
    assert len(pts) == BATCH + 100
    with bh_sim(nb, rec, "device", bh_walk_split=7) as sim:
        sim.settings = nb.Settings(G, 0.01, 1e-3, 1.0)
        acc, phi, counts = sim.field_at(pts, md)
        a1, p1, c1 = sim.field_at(pts[:BATCH], md)
        a2, p2, c2 = sim.field_at(pts[BATCH:], md)
        assert np.array_equal(acc, np.concatenate([a1, a2])) and np.array_equal(phi, np.concatenate([p1, p2]))
        assert counts == (c1[0] + c2[0], c1[1] + c2[1])
        ref = qp.replay(sim.tree(), pts, sim.tree_quadrupoles(), 1.0, 0.01)
        worst = qp.check(acc, phi, counts, ref, G, "two batches")
    report("field_at two batches", f"acc {worst[0]:.3e} phi {worst[1]:.3e}")


# ---------------------------------------------------------------------------------------------- 3. 4. the ends of theta2
@pytest.mark.parametrize("tree", TREES)
def test_theta2_zero_gives_mode_tree_bit_for_bit(gpu, tree):
    nb = gpu
    rec = plummer_bodies(nb, 1001, seed=9)
    pts = probe_mix(rec, seed=9)
    with bh_sim(nb, rec, tree, bh_walk_split=7) as sim:
        sim.settings = nb.Settings(G, 0.01, 1e-3, 0.0)
        phi2, c2 = sim.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)
        phi1, c1 = sim.potentials(nb.POTENTIAL_TREE)
        assert np.array_equal(phi2, phi1) and c2 == c1 and c1[0] == 1001 * 1000
        f2, f1 = sim.field_at(pts, nb.POTENTIAL_TREE_QUADRUPOLE), sim.field_at(pts, nb.POTENTIAL_TREE)
        assert np.array_equal(f2[0], f1[0]) and np.array_equal(f2[1], f1[1]) and f2[2] == f1[2]


@pytest.mark.parametrize("tree", TREES)
def test_theta2_huge_accepts_the_root_alone(gpu, tree):
    nb = gpu
    n = 1001
    rec = plummer_bodies(nb, n, seed=9)
    with bh_sim(nb, rec, tree) as sim:
        w, phi, ref = potentials_checked(nb, sim, 1e30, 0.01, f"theta2=1e30 {tree}")
        assert (ref["accepted"] == 1).all() and (ref["visited"] == 1).all() and (ref["n_terms"] == 2).all()
        own = rec["position"].astype(np.float64)
        wf, got, fref = field_checked(nb, sim, own, 1e30, 0.01, f"theta2=1e30 {tree} field")
        assert got[2] == (n, n)
        assert (np.abs(got[1] - phi) <= 2 * (qp.C_S * qp.U32 + 2 * qp.U64) * G * ref["Ts"]).all()
    report(f"theta2=1e30 {tree}", f"potentials phi {w:.3e} field acc {wf[0]:.3e} phi {wf[1]:.3e}")


# ---------------------------------------------------------------------------------------------- 5. the clump world
@pytest.mark.parametrize("tree", TREES)
def test_clump(gpu, tree):
    """Cells 1e-5 wide inside a box of 64: tensors of ~1e-13 beside ones of ~1, accepted from 1e-5 away."""
    nb = gpu
    rec = clump_world(nb)
    pts = np.concatenate([rec["position"][::3].astype(np.float64), probe_mix(rec, seed=5, n_own=0, n_random=300, n_outside=50),
                          np.array([1.3, -0.7, 0.4]) + np.random.default_rng(5).uniform(-1e-4, 1e-4, (300, 3))])
    with bh_sim(nb, rec, tree) as sim:
        w, _, ref = potentials_checked(nb, sim, 0.25, 0.0, f"clump {tree}", (7, 64))
        assert (ref["n_terms"] > ref["accepted"]).all()
        wf, _, _ = field_checked(nb, sim, pts, 0.25, 0.0, f"clump {tree} field", (7, 64))
    report(f"clump {tree}", f"potentials phi {w:.3e} field acc {wf[0]:.3e} phi {wf[1]:.3e}")


# ---------------------------------------------------------------------------------------------- 6. the force walk's field
def test_consistency_with_the_quadrupole_force_walk(gpu):
    """update_forces with multipole = 2 and field_at(own positions, 2) sum the same terms over the same nodes: they differ by
    the two walks' roundings at most; potentials(2) and field_at's phi likewise."""
    nb = gpu
    theta2, g_soft = 0.25, 0.01
    rec = plummer_bodies(nb, 4097, seed=41)
    with bh_sim(nb, rec, "host", leaf="direct") as sim:
        sim.multipole = nb.MULTIPOLE_QUADRUPOLE
        sim.settings = nb.Settings(G, g_soft, 1e-3, theta2)
        sim.update_forces()
        pts = sim.get_points()
        tree_f, q6_f = sim.tree(), sim.tree_quadrupoles()
        fref = walk_list_quad(pts["position"], tree_f, q6_f, G, g_soft, theta2, 1)
        own = pts["position"].astype(np.float64)
        acc, phi, counts = sim.field_at(own, nb.POTENTIAL_TREE_QUADRUPOLE)
        tree, q6 = sim.tree(), sim.tree_quadrupoles()
        assert same_tree(tree, tree_f) and np.array_equal(q6.view(np.uint32), q6_f.view(np.uint32))
        ref = qp.replay(tree, own, q6, theta2, g_soft)
        qp.check(acc, phi, counts, ref, G, "field at the own positions")
        assert counts == (int(fref["accepted"].sum()), int(fref["visited"].sum()))
        bound_a = (qp.C_V * qp.U32 + ref["n_terms"] * qp.U64) * G * ref["Tv"]
        diff = np.abs(pts["acceleration"].astype(np.float64) - acc).max(1)
        ratio = diff / (QUAD_RTOL * fref["T"] + bound_a)
        print(f"\n[quadrupole potentials] force walk against field_at: worst {ratio.max():.3e} x (QUAD_RTOL T + the field bound)")
        assert ratio.max() <= 1.0
        pot, pcounts = sim.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)
        assert pcounts == counts
        bound_p = (qp.C_S * qp.U32 + ref["n_terms"] * qp.U64) * G * ref["Ts"]
        assert (np.abs(pot - phi) <= 2 * bound_p).all()


# ---------------------------------------------------------------------------------------------- 7. accuracy
def test_accuracy_against_the_pair_sum(gpu):
    """n = 4097, host build, g_soft = 0, theta2 = 0.25 (the tree of tests/test_quad_pot_list_checker.py): the median error of
    mode 2 is below mode TREE's and is the CPU f64 replay's up to the f32 rounding of the terms."""
    nb = gpu
    rec = plummer_bodies(nb, qp.ACCURACY_N, seed=qp.ACCURACY_N)
    with bh_sim(nb, rec, "host") as sim:
        sim.settings = nb.Settings(G, 0.0, 1e-3, 0.25)
        exact, _ = sim.potentials(nb.POTENTIAL_PAIRS)
        med = {}
        for mode in (nb.POTENTIAL_TREE, nb.POTENTIAL_TREE_QUADRUPOLE):
            phi, _ = sim.potentials(mode)
            e = np.abs(phi - exact) / np.abs(exact)
            med[mode] = float(np.median(e))
            print(f"\n[quadrupole potentials] mode {mode}: median |phi - phi_PAIRS| / |phi_PAIRS| {med[mode]:.4e} p99 {np.percentile(e, 99):.4e}")
    cpu = qp.F64_POT_ERRORS[(2, 0.25)][0]
    print(f"\n[quadrupole potentials] GPU median / CPU f64 median {med[2] / cpu:.5f}")
    assert med[2] < med[1]
    assert med[2] <= ACCURACY_MARGIN * cpu


# ---------------------------------------------------------------------------------------------- 8. the energy
@pytest.mark.parametrize("tree", TREES)
def test_energy_world(gpu, tree):
    nb = gpu
    rec = plummer_bodies(nb, 4097, seed=43)
    with bh_sim(nb, rec, tree) as sim:
        sim.settings = nb.Settings(G, 0.01, 1e-3, 0.25)
        ke, pe = sim.energy_world(nb.POTENTIAL_TREE_QUADRUPOLE)
        phi, _ = sim.potentials(nb.POTENTIAL_TREE_QUADRUPOLE)
        want = 0.5 * float((rec["mass"].astype(np.float64) * phi).sum())
        assert abs(pe - want) <= 1e-13 * abs(want)
        kp, pp = sim.energy_world(nb.POTENTIAL_PAIRS)
        k1, p1 = sim.energy_world(nb.POTENTIAL_TREE)
        assert ke == kp == k1
        print(f"\n[quadrupole potentials] {tree}: |E - E_PAIRS| mode TREE {abs(p1 - pp):.3e}, mode TREE_QUADRUPOLE {abs(pe - pp):.3e} (E_PAIRS {kp + pp:.6e})")


# ---------------------------------------------------------------------------------------------- 9. the calls leave no trace
@pytest.mark.parametrize("multipole", [1, 2])
def test_calls_leave_no_trace_in_later_steps(gpu, multipole):
    """A device-build handle stepping without read-back in a box bodies leave: steps after calls in mode 2 give the bits of a
    handle that never called, and stats() is unchanged by the calls."""
    nb = gpu
    md = nb.POTENTIAL_TREE_QUADRUPOLE
    rec = nb.plummer(6000, seed=17)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 1.45])
    box = ((0.0, 0.0, 0.0), 2.92)
    probes = np.random.default_rng(1).uniform(-3, 3, (3000, 3))
    with bh_sim(nb, rec, "device", leaf="direct", box=box) as a, bh_sim(nb, rec, "device", leaf="direct", box=box) as b:
        for s in (a, b):
            s.multipole = multipole
            s.settings = nb.Settings(G, 0.01, 0.05, 0.25)
            s.init()
        a.steps(3)
        before = a.stats()
        phi, _ = a.potentials(md)
        acc, fphi, _ = a.field_at(probes, md)
        a.energy_world(md)
        assert len(a.tree_quadrupoles()) == len(a.tree()["skip"])
        after = a.stats()
        assert (before.steps, before.interactions, before.node_visits) == (after.steps, after.interactions, after.node_visits)
        a.steps(2)
        b.steps(5)
        pa, pb = a.get_points(), b.get_points()
        assert len(pa) == len(pb) < len(rec)
        sa, sb = a.stats(), b.stats()
        assert (sa.steps, sa.interactions, sa.node_visits) == (sb.steps, sb.interactions, sb.node_visits)
        for f in ("position", "velocity", "acceleration", "mass"):
            assert np.array_equal(np.ascontiguousarray(pa[f]).view(np.uint8), np.ascontiguousarray(pb[f]).view(np.uint8)), f
        assert a.elapsed() == b.elapsed()
        assert (phi < 0).all() and np.isfinite(acc).all() and (fphi < 0).all()


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_refusals(gpu):
    nb = gpu
    md = nb.POTENTIAL_TREE_QUADRUPOLE
    rec = plummer_bodies(nb, 65, seed=37)
    pts = np.zeros((4, 3))
    kw = dict(method=nb.BARNES_HUT, math_mode=nb.FAST)
    refused = {
        "brute force": lambda: nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST),
        "f64": lambda: nb.Simulation(rec.astype(nb.PARTICLE_DTYPE64), *BOX, **kw),
        "sharded": lambda: nb.Simulation(rec, *BOX, rank=0, world_size=2, **kw),
        "spatial": lambda: nb.Simulation(rec, *BOX, shard_mode=nb.SHARD_SPATIAL, **kw),
    }
    for name, make in refused.items():
        with make() as sim:
            for call in (lambda: sim.potentials(md), lambda: sim.field_at(pts, md), lambda: sim.energy_world(md)):
                with pytest.raises(nb.NbodyError) as e:
                    call()
                assert e.value.code == nb.NBODY_ERR_INVALID, name
                assert "mode" in str(e.value) and "NBODY_POTENTIAL_TREE_QUADRUPOLE" in str(e.value), name
    with nb.Simulation(rec, *BOX, **kw) as sim:
        for mode in (3, -1):
            with pytest.raises(nb.NbodyError) as e:
                sim.potentials(mode)
            assert e.value.code == nb.NBODY_ERR_INVALID and "mode" in str(e.value)

        def export_refused():
            with pytest.raises(nb.NbodyError) as e:
                sim.tree_quadrupoles()
            assert e.value.code == nb.NBODY_ERR_INVALID

        sim.update_forces()                      # a monopole force pass
        export_refused()
        sim.potentials(md)
        assert sim.tree_quadrupoles().shape == (len(sim.tree()["skip"]), 6)
        sim.potentials(nb.POTENTIAL_TREE)        # the tree of a monopole call
        export_refused()
        sim.field_at(pts, md)
        assert sim.tree_quadrupoles().any()
        sim.field_at(pts, nb.POTENTIAL_TREE)
        export_refused()
        sim.energy_world(md)
        assert sim.tree_quadrupoles().any()
        sim.update_forces()
        export_refused()
        assert sim.multipole == nb.MULTIPOLE_MONOPOLE   # the mode is per call: the setting is untouched
