"""The spatial ranks' Barnes-Hut walks against the f64 sums of their own node lists (tests/let_list.py).

The one-GPU rehearsal of tests/test_spatial_gpu.py: G handles play ranks 0..G-1, nb.spatial_step makes a force pass with the
exchanges done as device-to-device copies.  After the pass every rank's held node array is copied out
(Simulation.let_held(): nbody_debug_let_export_held) and, with the single-handle device tree of the same bodies, goes
through let_list.check_world: walk (|a_i - S_i| <= R T_i for every own body), counts (stats() equal the replay's sums
exactly), structure, closure and partition.  No check has an allowance for a flipped opening test.  The worst
|a - S| / T of every case is printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from let_list import check_world, one_tree_facts, rank_input

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
G_NEWTON = 1.0
LEAVES = ("reference", "direct")
FIELDS = ("position", "velocity", "acceleration", "mass")
_one = {}


def make_world(nb, ics, G, box, st, leaf, prune=True):
    lm = nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE
    sims = [nb.Simulation(ics, *box, method=nb.BARNES_HUT, math_mode=nb.FAST, rank=r, world_size=G, capacity=max(len(ics), 1),
                          shard_mode=nb.SHARD_SPATIAL, leaf_mode=lm) for r in range(G)]
    for s in sims:
        s.settings = st
        s.set_prune(prune)
        s.init()
    return sims


def close(sims):
    for s in sims:
        s.close()


def single_tree(nb, key, bodies, box):
    """(tree, let_list facts) of the single-handle device build of `bodies`: built once per world (the tree does not depend on
    theta2, g_soft or the leaf rule)."""
    if key not in _one:
        with nb.Simulation(bodies, *box, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as one:
            one.settings = nb.Settings(G_NEWTON, 0.01, 1e-3, 0.25)
            one.update_forces()
            tree = one.tree()
        _one[key] = (tree, one_tree_facts(tree))
    return _one[key]


def rank_inputs(sims):
    """rank_input of every rank after a force pass whose statistics started at zero"""
    out = []
    for s in sims:
        pts, st, ls = s.get_points(), s.stats(), s.let_stats()
        out.append(rank_input(s.let_held(), pts["position"], pts["acceleration"], st.interactions, st.node_visits, ls.nodes_local,
                              ls.nodes_received))
    return out


def checked_pass(nb, orc, sims, tree, facts, leaf, what):
    """One force pass of the world, checked; returns let_list's info."""
    for s in sims:
        s.reset_stats()
    nb.spatial_step(sims, forces_only=True)
    st = sims[0].settings
    info = check_world(orc, rank_inputs(sims), tree, st.theta2, st.g, st.g_soft, LEAVES.index(leaf), facts, what=what)
    print(f"\n[let list] {what}: worst |a - S| / T {info['worst']:.3e}, moments {info['moments'][0]:.3f} u / {info['moments'][1]:.3f} u, "
          f"held {[len(s.let_held()['width']) for s in sims]} of {len(tree['width'])}")
    return info


# ---------------------------------------------------------------------------------------------- one force pass
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("G,n", [(2, 300), (3, 1001), (5, 64), (8, 300), (4, 4097)])
def test_one_force_pass(gpu, orc, G, n, leaf, prune):
    nb = gpu
    ics = nb.plummer(n, seed=700 + n)
    tree, facts = single_tree(nb, ("plummer", n), ics, BOX)
    for theta2 in (0.25, 1.0):
        for g_soft in (0.0, 0.01):
            sims = make_world(nb, ics, G, BOX, nb.Settings(G_NEWTON, g_soft, 1e-3, theta2), leaf, prune)
            try:
                checked_pass(nb, orc, sims, tree, facts, leaf, f"G={G} n={n} {leaf} prune={prune} theta2={theta2} g_soft={g_soft}")
                assert sum(len(s) for s in sims) == n
            finally:
                close(sims)


def test_one_force_pass_8_ranks_20000_bodies(gpu, orc):
    nb = gpu
    G, n = 8, 20000
    ics = nb.plummer(n, seed=62)
    tree, facts = single_tree(nb, ("plummer", n), ics, BOX)
    sims = make_world(nb, ics, G, BOX, nb.Settings(G_NEWTON, 0.01, 1e-3, 0.25), "direct", True)
    try:
        checked_pass(nb, orc, sims, tree, facts, "direct", f"G={G} n={n} direct pruned")
    finally:
        close(sims)


@pytest.mark.parametrize("leaf", LEAVES)
def test_more_ranks_than_bodies(gpu, orc, leaf):
    """8 ranks, 5 bodies: the ranks that own nothing export, import and count consistently."""
    nb = gpu
    G, n = 8, 5
    ics = nb.plummer(n, seed=705)
    tree, facts = single_tree(nb, ("plummer", n), ics, BOX)
    for prune in (True, False):
        sims = make_world(nb, ics, G, BOX, nb.Settings(G_NEWTON, 0.01, 1e-3, 0.25), leaf, prune)
        try:
            checked_pass(nb, orc, sims, tree, facts, leaf, f"G={G} n={n} {leaf} prune={prune}")
            owned = [len(s) for s in sims]
            assert sum(owned) == n and owned.count(0) >= G - n
            for s, k in zip(sims, owned):
                if k == 0:
                    assert (s.stats().interactions, s.stats().node_visits) == (0, 0)
        finally:
            close(sims)


@pytest.mark.parametrize("leaf", LEAVES)
def test_after_migration(gpu, orc, leaf):
    """3 ranks, 3 000 bodies in the width-2.5 box: three full steps (bodies leave the box and change ranks, the bounds are
    redrawn), then a force pass, checked against the single-handle tree of the bodies that are left, where they are."""
    nb = gpu
    G, n = 3, 3000
    box = ((0.0, 0.0, 0.0), 2.5)
    ics = nb.plummer(n, seed=64)
    sims = make_world(nb, ics, G, box, nb.Settings(G_NEWTON, 0.01, 5e-3, 0.25), leaf)
    try:
        owners = []
        for _ in range(3):
            nb.spatial_step(sims)
            owners.append([set(s.download_ids().tolist()) for s in sims])
        rec, idx = nb.spatial_gather(sims, n)
        assert len(rec) < n and sum(s.let_stats().bodies_migrated for s in sims) > 0
        assert any(a != b for a, b in zip(owners[0], owners[-1]))
        tree, facts = single_tree(nb, ("migrated", leaf), np.ascontiguousarray(rec), box)
        checked_pass(nb, orc, sims, tree, facts, leaf, f"after 3 steps G={G} n={len(rec)} {leaf}")
        again, idx2 = nb.spatial_gather(sims, n)
        assert np.array_equal(idx, idx2) and np.array_equal(again["position"].view(np.uint32), rec["position"].view(np.uint32))
    finally:
        close(sims)


# ---------------------------------------------------------------------------------------------- special worlds
def deep_world(nb):
    """test_spatial_shards_with_bodies_that_share_all_21_levels' bodies: groups a few 1.2e-7 apart (equal 63-bit keys)"""
    n = 6000
    ics = nb.plummer(n, seed=66)
    rng = np.random.default_rng(1)
    for dst, src in ((1, 0), (7, 3), (11, 3), (n - 1, n // 2), (100, 99), (101, 99), (102, 99), (103, 99)):
        ics["position"][dst] = ics["position"][src] + rng.integers(1, 12, 3).astype(np.float32) * np.float32(1.2e-7)
    return ics


def clump_world(nb):
    """test_spatial_ranks_with_a_clump_inside_one_level_16_cell's bodies: 1 500 of 7 500 inside one level-16 cell"""
    rng = np.random.default_rng(7)
    clump = 1500
    ics = nb.plummer(6000 + clump, seed=92)
    w16 = np.float64(BOX[1]) / 65536.0
    ics["position"][6000:] = (-32.0 + 36000 * w16 + w16 * (0.1 + 0.5 * rng.random((clump, 3)))).astype(np.float32)
    ics["velocity"][6000:] = 0.0
    return ics


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name,g_soft", [("deep", 0.01), ("clump", 1e-3)])
def test_special_worlds(gpu, orc, name, g_soft, leaf):
    nb = gpu
    ics = deep_world(nb) if name == "deep" else clump_world(nb)
    tree, facts = single_tree(nb, (name,), ics, BOX)
    if name == "deep":
        assert np.log2(BOX[1] / np.float64(tree["width"].min())) > 22
    sims = make_world(nb, ics, 3, BOX, nb.Settings(G_NEWTON, g_soft, 1e-3, 0.25), leaf)
    try:
        checked_pass(nb, orc, sims, tree, facts, leaf, f"{name} world G=3 n={len(ics)} {leaf}")
    finally:
        close(sims)


# ---------------------------------------------------------------------------------------------- the hook itself
def snapshot(nb, sims, n):
    rec, idx = nb.spatial_gather(sims, n)
    stats = [(s.stats().interactions, s.stats().node_visits, s.stats().tree_nodes, s.stats().steps) for s in sims]
    ls = []
    for s in sims:
        l = s.let_stats()
        ls.append(tuple(getattr(l, k) for k in ("steps", "bodies_migrated", "nodes_local", "nodes_global", "nodes_sent", "nodes_received",
                                                "bytes_sent", "bytes_allgather_equivalent", "host_syncs", "migrant_respills",
                                                "node_array_peak_bytes", "node_array_bytes")))
    return rec, idx, stats, ls


def test_an_export_leaves_no_trace(gpu):
    """A step, a force pass and two more steps, with and without exports in between: the same bits, NbodyStats and NbodyLetStats; two
    exports in a row return the same arrays."""
    nb = gpu
    G, n = 3, 3000
    box = ((0.0, 0.0, 0.0), 2.5)
    ics = nb.plummer(n, seed=64)
    out = {}
    for export in (False, True):
        sims = make_world(nb, ics, G, box, nb.Settings(G_NEWTON, 0.01, 5e-3, 0.25), "direct")
        try:
            nb.spatial_step(sims)      # (the retain of a step puts every body inside the box)
            nb.spatial_step(sims, forces_only=True)
            if export:
                first = [s.let_held() for s in sims]
                second = [s.let_held() for s in sims]
                for a, b in zip(first, second):
                    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and len(a["width"]) > 0
            nb.spatial_step(sims)
            if export:
                for s in sims:
                    s.let_held()        # (after a step: the array that step walked)
            nb.spatial_step(sims)
            out[export] = snapshot(nb, sims, n)
        finally:
            close(sims)
    a, b = out[False], out[True]
    assert np.array_equal(a[1], b[1]) and len(a[1]) <= n
    for f in FIELDS:
        assert np.array_equal(a[0][f].view(np.uint32), b[0][f].view(np.uint32)), f
    assert a[2] == b[2] and a[3] == b[3]


def test_refusals_name_the_call(gpu):
    nb = gpu
    ics = nb.plummer(300, seed=3)
    st = nb.Settings(G_NEWTON, 0.01, 1e-3, 0.25)
    with nb.Simulation(ics, *BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as one:
        one.settings = st
        one.update_forces()
        with pytest.raises(nb.NbodyError) as e:      # not a spatial handle
            one.let_held()
        assert e.value.code == nb.NBODY_ERR_INVALID and "nbody_debug_let_export_held" in str(e.value)
    sims = make_world(nb, ics, 2, BOX, st, "reference")
    try:
        for s in sims:                               # no force pass yet
            with pytest.raises(nb.NbodyError) as e:
                s.let_held()
            assert e.value.code == nb.NBODY_ERR_INVALID and "nbody_debug_let_export_held" in str(e.value)
        nb.spatial_step(sims, forces_only=True)
        s = sims[1]
        n = C.c_size_t(0)
        assert nb.lib.nbody_debug_let_export_held(s._h, None, None, None, None, None, None, 0, C.byref(n)) == nb.NBODY_OK   # NULL arrays: the count
        m = n.value
        assert m == len(s.let_held()["width"]) > 0
        width = np.full(m, -1.0, np.float32)
        rc = nb.lib.nbody_debug_let_export_held(s._h, None, width.ctypes.data, None, None, None, None, m - 1, C.byref(n))
        assert rc == nb.NBODY_ERR_CAPACITY and n.value == m and (width == -1.0).all()
        assert "nbody_debug_let_export_held" in nb.lib.nbody_last_error(s._h).decode()
        assert nb.lib.nbody_debug_let_export_held(s._h, None, width.ctypes.data, None, None, None, None, m, C.byref(n)) == nb.NBODY_OK   # one array alone
        assert np.array_equal(width, s.let_held()["width"])
        assert nb.lib.nbody_debug_let_export_held(None, None, None, None, None, None, None, 0, C.byref(n)) == nb.NBODY_ERR_INVALID
        s.upload(ics)                                # a new upload: the array of the old bodies is no longer offered
        with pytest.raises(nb.NbodyError) as e:
            s.let_held()
        assert e.value.code == nb.NBODY_ERR_INVALID and "nbody_debug_let_export_held" in str(e.value)
    finally:
        close(sims)
