"""tests/pot_list.py held to the oracle (no GPU): its replay accepts and visits exactly what oracle.bh_walk_list does under
the DIRECT leaf rule, its sums are the sums over that list, and check_potentials catches a dropped term, a doubled term and
a wrong mass.  Plus the ABI of the two entry points the checker serves."""
import ctypes
import inspect

import numpy as np
import pytest

import pot_list

BOX = ((0.0, 0.0, 0.0), 64.0)


def world(nb, orc, n, f64, seed=5):
    rec = nb.plummer(2 * n + 64, seed=seed, f64=f64)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 30.0][:n])
    a = rec.astype(orc.P64 if f64 else orc.P32)
    return a, orc.bh_build_tree(a, *BOX)


def list_sum(tree, p, nodes, g_soft):
    ft = tree["com_mass"].dtype.type
    cm = tree["com_mass"][np.asarray(nodes, np.int64)].astype(np.float64)
    d = cm[:, :3] - np.asarray(p, ft).astype(np.float64)
    return float((cm[:, 3] / np.sqrt((d * d).sum(1) + float(ft(ft(g_soft) * ft(g_soft))))).sum())


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("n", [1, 2, 65, 1001])
@pytest.mark.parametrize("theta2,g_soft", [(0.25, 0.0), (1.0, 0.01), (0.0, 0.01), (1e30, 0.0)])
def test_replay_is_the_oracles_direct_walk(nb, orc, n, f64, theta2, g_soft):
    a, tree = world(nb, orc, n, f64)
    got = pot_list.replay(tree, a["position"], theta2, g_soft)
    ref = orc.bh_walk_list(tree, a["position"], theta2, 1.0, g_soft, leaf_mode=1)
    assert np.array_equal(got["accepted"], ref["accepted"].astype(np.int64))
    assert np.array_equal(got["visited"], ref["visited"].astype(np.int64))
    for i in sorted({0, n // 3, n - 1}):
        nodes = orc.bh_walk_list(tree, a["position"], theta2, 1.0, g_soft, leaf_mode=1, list_body=i)["list"]
        assert len(nodes) == got["accepted"][i]
        assert got["S"][i] == pytest.approx(list_sum(tree, a["position"][i], nodes, g_soft), rel=1e-13, abs=0.0)
    if theta2 == 1e30 and n > 1:   # the root alone, the body's own mass included
        assert (got["accepted"] == 1).all() and (got["visited"] == 1).all()
    if theta2 == 0.0:              # every other leaf (no two bodies of this set within 1e-5)
        assert (got["accepted"] == n - 1).all()


@pytest.mark.parametrize("f64", [False, True])
def test_planted_faults_are_caught(nb, orc, f64):
    n, theta2, g_soft, g = 1001, 0.25, 0.01, 1.0
    a, tree = world(nb, orc, n, f64)
    ref = pot_list.replay(tree, a["position"], theta2, g_soft)
    counts = (int(ref["accepted"].sum()), int(ref["visited"].sum()))
    phi = -g * ref["S"]
    assert pot_list.check_potentials(phi, counts, ref, g, f64) == 0.0
    i = 400
    nodes = orc.bh_walk_list(tree, a["position"], theta2, g, g_soft, leaf_mode=1, list_body=i)["list"]
    each = np.array([list_sum(tree, a["position"][i], [j], g_soft) for j in nodes])
    share = each / ref["S"][i]
    detectable = share > 2 * pot_list.bound(ref, f64)[i]
    # the smallest detectable term is 2 R_i of |phi_i|: on this body every single term is far above it
    assert detectable.all(), (share.min(), 2 * pot_list.bound(ref, f64)[i])
    k = int(np.argmin(each))   # the smallest term of the body: the hardest one to see
    for what, delta in (("dropped", -each[k]), ("doubled", each[k]), ("mass of a node half as heavy", -0.5 * each[k])):
        bad = phi.copy()
        bad[i] -= g * delta
        with pytest.raises(AssertionError):
            pot_list.check_potentials(bad, counts, ref, g, f64, what)
    with pytest.raises(AssertionError):
        pot_list.check_potentials(phi, (counts[0] - 1, counts[1]), ref, g, f64)
    with pytest.raises(AssertionError):
        pot_list.check_potentials(phi, (counts[0], counts[1] + 1), ref, g, f64)


def test_pair_sums_are_the_oracles_energy(nb, orc):
    rec = nb.plummer(700, seed=3)
    S = pot_list.pair_sums(rec, 0.01)
    ke, pe = orc.energy(rec.astype(orc.P32), 1.0, float(np.float32(0.01)))   # (an f32 handle holds g_soft as f32)
    assert -0.5 * float((rec["mass"].astype(np.float64) * S).sum()) == pytest.approx(pe, rel=1e-12)


def test_abi_of_the_new_entry_points(nb):
    assert {"nbody_potentials", "nbody_energy_world"} <= set(nb.DECLARED_SYMBOLS)
    assert nb.lib.nbody_abi_version() == 4
    assert (nb.POTENTIAL_PAIRS, nb.POTENTIAL_TREE) == (0, 1)
    pot, en = nb.lib.nbody_potentials, nb.lib.nbody_energy_world
    assert pot.restype is ctypes.c_int and en.restype is ctypes.c_int
    assert pot.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                            ctypes.POINTER(ctypes.c_uint64)]
    assert en.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    # a null handle is refused without touching a device
    assert pot(None, 0, None, 0, None, None) == nb.NBODY_ERR_INVALID
    assert en(None, 1, None, None) == nb.NBODY_ERR_INVALID
    assert list(inspect.signature(nb.Simulation.potentials).parameters) == ["self", "mode"]
    assert list(inspect.signature(nb.Simulation.energy_world).parameters) == ["self", "mode"]
    header = open(nb.LIB_PATH.replace("nbody-llm_amd/libnbody_hip.so", "include/nbody_hip.h")).read()
    assert "int nbody_potentials(NbodyHandle* h, int mode, double* phi, size_t cap, size_t* n_out, uint64_t counts[2]);" in header
    assert "int nbody_energy_world(NbodyHandle* h, int mode, double* kinetic, double* potential);" in header
