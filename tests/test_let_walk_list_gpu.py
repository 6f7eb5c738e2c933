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

import tree_moments as tm
from bh_list import LIST_RTOL_F32, check_walk
from let_list import LET_MOMENT_R, check_world, one_tree_facts, rank_input

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


# ---------------------------------------------------------------------------------------------- light and massless cells on a rank boundary
# tree_moments' boundary worlds: a rank that holds a sun and then dust up to its bound, so that the cells that span the bound
# are dust only and a difference of the rank's prefix sums cancels to a few bodies of 1e-12 or 1e-15 behind a mass of 1; and a
# cell across a bound whose bodies (or whose owner's bodies) are massless.  tests/test_let_list_checker.py shows on the CPU
# that spanning cells formed from the high parts of the prefixes alone miss LET_MOMENT_R by more than 10x on every dust case.
ST_DUST = (G_NEWTON, 0.01, 1e-3, 0.25)


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("dust", tm.LET_DUST_MASSES)
@pytest.mark.parametrize("G,n", tm.LET_DUST_CASES)
def test_dust_across_the_boundaries(gpu, orc, G, n, dust, leaf):
    """Two suns in dust on G ranks, one pruned force pass, all five checks.  With the spanning cells' own parts taken from the high
    parts of the prefixes alone these cases gave held spanning cells 4 to 1.4e6 u from their exact moments."""
    nb = gpu
    ics = tm.dust_world(nb, n, dust)
    tree, facts = single_tree(nb, ("dust", n, dust), ics, BOX)
    sims = make_world(nb, ics, G, BOX, nb.Settings(*ST_DUST), leaf)
    try:
        checked_pass(nb, orc, sims, tree, facts, leaf, f"dust {dust:g} G={G} n={n} {leaf}")
        assert sum(len(s) for s in sims) == n
        assert all(np.isfinite(s.get_points()["acceleration"]).all() for s in sims)
    finally:
        close(sims)


@pytest.mark.parametrize("own_side_only", [False, True])
@pytest.mark.parametrize("G,n,r", tm.LET_MASSLESS_CASES)
def test_massless_cells_across_a_boundary(gpu, orc, G, n, r, own_side_only):
    """control_world with every body of the deepest cell across boundary r massless (or only the owner's part of it): the cell is
    held by both neighbours as a spanning cell and -- with exact M = 0 -- has the single-handle tree's bits, mass +0 and that
    tree's NaN centre, which every walk opens; no acceleration is non-finite."""
    nb = gpu
    base = tm.control_world(nb, n)
    tree0, _ = single_tree(nb, ("control", n), base, BOX)
    ics, node = tm.massless_boundary(base, tree0, G, r, own_side_only)
    tree, facts = single_tree(nb, ("massless", n, G, r, own_side_only), ics, BOX)
    assert np.array_equal(tree["skip"], tree0["skip"])
    M = facts["exact"]["M"][facts["row"][node]]
    assert (M != 0) == own_side_only
    for leaf in LEAVES:
        sims = make_world(nb, ics, G, BOX, nb.Settings(*ST_DUST), leaf)
        try:
            checked_pass(nb, orc, sims, tree, facts, leaf, f"massless {'own part' if own_side_only else 'cell'} G={G} n={n} {leaf}")
            for q, s in enumerate(sims):
                h = s.let_held()
                at = np.flatnonzero(h["global_index"] == node)
                if q in (r - 1, r):
                    assert len(at) == 1 and h["origin"][at[0]] == (2 if q == r - 1 else 3), (q, at, h["origin"][at])
                for p in at:
                    assert h["origin"][p] >= 2
                    got, want = h["com_mass"][p].view(np.uint32), tree["com_mass"][node].view(np.uint32)
                    print(f"[let list] rank {q}: cell {node} holds {[hex(v) for v in got.tolist()]}, the single tree {[hex(v) for v in want.tolist()]}")
                    if not own_side_only:
                        assert np.array_equal(got, want) and got[3] == 0 and np.isnan(h["com_mass"][p, :3]).all()
                assert np.isfinite(s.get_points()["acceleration"]).all()
        finally:
            close(sims)


@pytest.mark.parametrize("leaf", LEAVES)
def test_dust_after_migration(gpu, orc, leaf):
    """The 1e-12 dust in the width-8 box on 3 ranks: three full steps (bodies leave, the bounds are redrawn at the work quantiles
    and move into different dust), then a checked force pass against the single tree of the survivors; both suns are there."""
    nb = gpu
    G, n = 3, 5000
    box = ((0.0, 0.0, 0.0), 8.0)
    ics = tm.dust_world(nb, n, 1e-12)
    sims = make_world(nb, ics, G, box, nb.Settings(G_NEWTON, 0.05, 2e-2, 0.5), leaf)
    try:
        for _ in range(3):
            nb.spatial_step(sims)
        rec, idx = nb.spatial_gather(sims, n)
        assert 2 < len(rec) < n and np.count_nonzero(rec["mass"] == 1.0) == 2
        tree, facts = single_tree(nb, ("dust migrated", leaf), np.ascontiguousarray(rec), box)
        checked_pass(nb, orc, sims, tree, facts, leaf, f"dust 1e-12 after 3 steps G={G} n={len(rec)} {leaf}")
        assert all(np.isfinite(s.get_points()["acceleration"]).all() for s in sims)
    finally:
        close(sims)


def test_dust_accelerations_of_the_ranks_against_the_single_handle(gpu, orc):
    """End to end on the 1e-12 dust, 2 ranks, n = 1 025, theta2 = 0.25, the reference's leaf rule: every rank's accelerations
    against the single-handle device-tree handle's, by the derivation of
    test_tree_moments_gpu.test_dust_accelerations_device_tree_against_host_tree:

        |a_rank - a_one| <= LIST_RTOL_F32 (T_rank + T_one) + D_i,

    D_i summed over the internal cells body i accepts with b_j = SCHEME_R + LET_MOMENT_R: the single tree's stored moments lie
    within SCHEME_R u of the exact ones (tests/test_tree_moments_gpu.py), a held cell's -- spanning or private -- within
    LET_MOMENT_R u (the structure check of the pass, made here), so the two differ by at most their sum; LET_MOMENT_R stands
    where the host build's n_j + 2 stood.  Both walks accept the same nodes for every body (asserted, by global index): with this
    seed (dust_world: 400 + n) no opening test flips."""
    nb = gpu
    G, n = 2, 1025
    ics = tm.dust_world(nb, n, 1e-12)
    st = nb.Settings(*ST_DUST)
    with nb.Simulation(ics, *BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as one:
        one.settings = st
        one.update_forces()
        t1, a1 = one.tree(), one.get_points()["acceleration"].astype(np.float64)
    ref1 = orc.bh_walk_list(t1, ics["position"], st.theta2, st.g, st.g_soft)
    check_walk(a1, ref1, LIST_RTOL_F32, what="single handle")
    facts = one_tree_facts(t1)
    ex = facts["exact"]
    u = tm.U[np.dtype(np.float32)]
    b = np.zeros(len(t1["skip"]))
    absA = np.zeros(len(t1["skip"]))
    b[ex["cell"]] = tm.SCHEME_R[np.dtype(np.float32)] + LET_MOMENT_R
    absA[ex["cell"]] = np.sqrt((np.asarray(ex["A"], np.float64) ** 2).sum(axis=1))
    eps2 = float(np.float32(st.g_soft) * np.float32(st.g_soft))
    sims = make_world(nb, ics, G, BOX, st, "reference")
    worst = 0.0
    try:
        info = checked_pass(nb, orc, sims, t1, facts, "reference", f"dust 1e-12 end to end G={G} n={n}")
        seen = 0
        for r, s in enumerate(sims):
            h, pts, ids = s.let_held(), s.get_points(), s.download_ids()
            assert np.array_equal(pts["position"].view(np.uint32), ics["position"][ids].view(np.uint32))
            held_tree = dict(com_mass=np.ascontiguousarray(h["com_mass"], np.float32), width=h["width"], skip=h["skip"])
            gi = h["global_index"].astype(np.int64)
            ref_r = info["refs"][r]
            for k, i in enumerate(ids.tolist()):
                p = ics["position"][i:i + 1]
                lst = orc.bh_walk_list(t1, p, st.theta2, st.g, st.g_soft, list_body=0)["list"]
                mine = orc.bh_walk_list(held_tree, p, st.theta2, st.g, st.g_soft, list_body=0)["list"]
                assert np.array_equal(gi[mine], lst), f"rank {r} body {i}: the walks accept different nodes"
                cm = t1["com_mass"][lst].astype(np.float64)
                d = cm[:, :3] - p.astype(np.float64)
                dc = b[lst] * u * absA[lst]
                s_ = np.sqrt((d * d).sum(axis=1) + eps2)
                tmag = st.g * cm[:, 3] * np.sqrt((d * d).sum(axis=1)) / s_ ** 3
                s_short = np.maximum(s_ - dc, 0.0)
                with np.errstate(divide="ignore"):
                    D = float((tmag * b[lst] * u + 2.0 * st.g * cm[:, 3] * (1.0 + b[lst] * u) * dc / s_short ** 3)[b[lst] > 0].sum())
                bound = LIST_RTOL_F32 * (ref_r["T"][k] + ref1["T"][i]) + D
                diff = float(np.linalg.norm(pts["acceleration"][k].astype(np.float64) - a1[i]))
                assert diff <= bound, f"rank {r} body {i}: |a_rank - a_one| = {diff:.3e} beyond {bound:.3e} (moment term {D:.3e})"
                worst = max(worst, diff / bound if bound > 0 else 0.0)
                seen += 1
        assert seen == n
    finally:
        close(sims)
    print(f"dust 1e-12 end to end on {G} ranks: worst |a_rank - a_one| / bound = {worst:.3g}")
