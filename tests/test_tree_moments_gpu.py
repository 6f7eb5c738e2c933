"""The device build's masses and centres of mass, cell by cell, against exact sums over each cell's own bodies
(tests/tree_moments.py: the bounds, the count behind SCHEME_R and the worlds).  Every test builds on the device, exports the
tree, asserts the host build's structure (skip links and widths exactly, leaves bit copies of the bodies) and runs the
checker under both bounds.  `pytest -s` prints the worst ratio to each bound."""
import numpy as np
import pytest

import bh_list
import tree_moments as tm
from test_bh_device_tree_gpu import close_pairs, lattice_pairs
from test_tree_moments_checker import host_tree

pytestmark = pytest.mark.gpu
SD = dict(g=1.0, g_soft=0.02, dt=1e-3, theta2=0.25)
KINDS = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])


def bodies_of(points):
    return np.concatenate([points["position"], points["mass"][:, None]], axis=1)


def check_tree(nb, orc, sim, box, what, massless=0):
    """The handle's tree after a force pass: the host build's structure over the handle's own bodies, then the checker."""
    pts = sim.get_points()
    t = sim.tree()
    ht = host_tree(nb, orc, pts, box)
    assert sim.stats().tree_nodes == len(t["skip"]) == len(ht["skip"]), what
    assert np.array_equal(t["skip"], ht["skip"]), f"{what}: skip links differ"
    assert np.array_equal(t["width"], ht["width"]), f"{what}: cell widths differ"
    leaf = np.flatnonzero(ht["skip"] == np.arange(len(ht["skip"])) + 1)
    if len(pts):
        it = np.uint64 if t["com_mass"].dtype == np.float64 else np.uint32
        want = bodies_of(pts)[ht["leaf_body"][leaf]]
        assert np.array_equal(t["com_mass"][leaf].view(it), np.ascontiguousarray(want).view(it)), f"{what}: leaves are copies of the bodies"
    r = tm.check_moments(t, scheme=True, host_tree=ht, what=what)
    assert r["massless"] == massless, f"{what}: {r['massless']} massless cells"
    print(f"{what}: {r['cells']} cells; mass / centre worst {r['reference'][0]:.3g} / {r['reference'][1]:.3g} of (n_c + 2) u, "
          f"{r['scheme'][0]:.3g} / {r['scheme'][1]:.3g} of R u")
    return t, ht, pts


def build(nb, orc, ics, box, what, massless=0, math_mode=None, sd=SD):
    with nb.Simulation(ics, *box, method=nb.BARNES_HUT, math_mode=nb.FAST if math_mode is None else math_mode, tree_build=nb.TREE_DEVICE) as sim:
        sim.settings = nb.Settings(**sd)
        sim.update_forces()
        return check_tree(nb, orc, sim, box, what, massless)


@KINDS
@pytest.mark.parametrize("n", tm.SIZES)
def test_control(gpu, orc, n, f64):
    build(gpu, orc, tm.control_world(gpu, n, f64), tm.BOX, f"control {n}")


@pytest.mark.parametrize("first", [True, False], ids=["sun-first", "sun-last"])
@pytest.mark.parametrize("f64,dust", [(k == "f64", m) for k in ("f32", "f64") for m in tm.DUST_MASSES[k]],
                         ids=[f"{k}-{m:g}" for k in ("f32", "f64") for m in tm.DUST_MASSES[k]])
@pytest.mark.parametrize("n", tm.DUST_SIZES)
def test_two_suns_and_dust(gpu, orc, n, dust, first, f64):
    build(gpu, orc, tm.dust_world(gpu, n, dust, first, f64), tm.BOX, f"dust {dust:g} {n}")


@KINDS
@pytest.mark.parametrize("n", tm.SIZES)
def test_far_box(gpu, orc, n, f64):
    build(gpu, orc, tm.far_world(gpu, n, f64), tm.FAR_BOX, f"far box {n}")


@KINDS
def test_massless_clump(gpu, orc, f64):
    """Eight massless bodies alone in one cell: its mass is exactly 0 and its centre the host build's NaN, so every walk opens
    it and finds eight leaves that add nothing.  The world's sums are exact in f32 (tree_moments.massless_world), so the two
    builds store the same moments and after the first force pass a host-tree handle has counted exactly the same visits
    and accepted nodes.  Then both handles take two steps and their stats() are compared again: steps, accepted nodes, visits,
    tree nodes and body counts are equal.  (Nothing forces that once the bodies are off the grid -- the two builds then round
    their centres differently and an opening test on its threshold could fall either way -- but on these 309 bodies none
    does: measured (2, 84 547, 153 770, 498) on both handles in both precisions, and every kernel involved is
    deterministic.)  Every acceleration stays finite."""
    nb = gpu
    ics = tm.massless_world(nb, f64=f64)
    out = {}
    for tb in (nb.TREE_DEVICE, nb.TREE_HOST):
        with nb.Simulation(ics, *tm.BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=tb) as sim:
            sim.settings = nb.Settings(**SD)
            sim.update_forces()
            if tb == nb.TREE_DEVICE:
                t, ht, _ = check_tree(nb, orc, sim, tm.BOX, "massless clump", massless=tm.MASSLESS_CELLS)
                assert np.array_equal(t["com_mass"], ht["com_mass"].astype(t["com_mass"].dtype), equal_nan=True)   # (exact sums)
            s = sim.stats()
            first = (int(s.interactions), int(s.node_visits), int(s.tree_nodes))
            acc0 = sim.get_points()["acceleration"]
            sim.reset_stats()
            sim.init()
            sim.steps(2)
            s = sim.stats()
            stepped = (int(s.steps), int(s.interactions), int(s.node_visits), int(s.tree_nodes))
            out[tb] = (first, stepped, acc0, sim.get_points()["acceleration"], len(sim))
    d, h = out[nb.TREE_DEVICE], out[nb.TREE_HOST]
    assert d[0] == h[0], (d[0], h[0])
    print(f"massless clump, stepped stats (steps, accepted, visited, nodes): device tree {d[1]}, host tree {h[1]}")
    assert d[1] == h[1] and d[1][0] == 2 and d[4] == h[4] == len(ics), (d[1], h[1])
    assert np.isfinite(d[2]).all() and np.isfinite(d[3]).all() and np.isfinite(h[2]).all() and np.isfinite(h[3]).all()


@KINDS
def test_light_bodies_below_level_21(gpu, orc, f64):
    """Cells below level 21: the emit finds their bodies by walking the group of equal first keys (d > kLevels) and reads the
    same prefix sums.  tree_moments.deep_world: clumps a few 1.2e-7 apart, eight of their bodies at mass 1e-12."""
    nb = gpu
    t, _, _ = build(nb, orc, tm.deep_world(nb, f64), tm.BOX, "deep clumps")
    depth = np.log2(tm.BOX[1] / np.float64(t["width"].min()))
    assert depth > 21, depth
    cells = np.flatnonzero(t["skip"] != np.arange(len(t["skip"])) + 1)
    below = cells[np.log2(tm.BOX[1] / t["width"][cells].astype(np.float64)) > 21]
    assert len(below) >= 4 and (t["com_mass"][below, 3] < 1e-11).any()   # internal cells below level 21, a light one among them


@KINDS
@pytest.mark.parametrize("which", ["close", "lattice"])
def test_light_pairs_in_long_chains(gpu, orc, which, f64):
    """close_pairs / lattice_pairs with every other pair at mass 1e-12: chains of ~17 one-child cells above every pair, down
    to level 19 or 20 (not below 21: that is test_light_bodies_below_level_21), ~10 nodes per body.  Two force passes:
    "lattice" has more nodes than the first node array of an f32 handle holds, and the pass that finds that out may leave
    the host build's tree behind; the second one builds into the grown array."""
    nb = gpu
    make = close_pairs if which == "close" else lattice_pairs
    ics = tm.light_pairs(make(nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE))
    with nb.Simulation(ics, *tm.BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
        sim.settings = nb.Settings(**SD)
        sim.update_forces()
        sim.update_forces()
        t, _, _ = check_tree(nb, orc, sim, tm.BOX, f"{which} pairs")
    assert len(t["skip"]) > 4 * len(ics) + 64


@KINDS
def test_suns_first_in_record_order(gpu, orc, f64):
    """The 1e-9 dust with the suns as the first records, where the reference's own fold leaves (n_c + 2) u (tree_moments
    dust_world): the device build sorts by position, so the order of the records means nothing to it."""
    build(gpu, orc, tm.dust_world(gpu, 1025, 1e-9, True, f64, suns_lead=True), tm.BOX, "dust 1e-9, suns lead")


@KINDS
def test_after_unsynchronised_steps_with_escapes(gpu, orc, f64):
    """The 1e-12 dust in a box of width 8: 5 steps in one call (bodies leave, the records are compacted and the live count stays
    on the device), one more force pass, and that tree."""
    nb = gpu
    box = ((0.0, 0.0, 0.0), 8.0)
    ics = tm.dust_world(nb, 5000, 1e-12, True, f64)
    with nb.Simulation(ics, *box, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
        sim.init()
        sim.steps(5)
        sim.update_forces()
        assert 2 < len(sim) < len(ics)
        _, _, pts = check_tree(nb, orc, sim, box, "dust 1e-12 after 5 steps")
    assert np.count_nonzero(pts["mass"] == 1.0) == 2


def test_dust_accelerations_device_tree_against_host_tree(gpu, orc):
    """End to end on the 1e-12 dust, f32 fast walk, theta2 = 0.25: per body, the device-tree handle's acceleration against the
    host-tree handle's.  Each lies within LIST_RTOL_F32 T_i of the f64 sum S_i of its own tree's accepted nodes (bh_list); both
    walks accept the same nodes (asserted: with these seeds no opening test sits within the moments' rounding of its
    threshold), so S_i differs between the trees by the moments alone.  Of an internal cell j of n_j bodies the two stored
    masses differ by at most b_j u M_j and the centres by at most b_j u |A_j|, b_j = SCHEME_R + n_j + 2 (the checker's two
    bounds, u = 2^-24); a term t = g m d / s^3, s^2 = |d|^2 + eps^2, moves by at most |t| dm / m + 2 g m |dc| / s^3 (the
    Jacobian of d / s^3 has norm <= 2 / s^3; s is taken |dc| short).  Summed over the body's accepted cells that is D_i, and

        |a_dev - a_host| <= LIST_RTOL_F32 (T_dev + T_host) + D_i."""
    nb = gpu
    n = 1025
    ics = tm.dust_world(nb, n, 1e-12)
    res = {}
    for tb in (nb.TREE_DEVICE, nb.TREE_HOST):
        with nb.Simulation(ics, *tm.BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=tb) as sim:
            sim.settings = nb.Settings(**SD)
            sim.update_forces()
            if tb == nb.TREE_DEVICE:
                check_tree(nb, orc, sim, tm.BOX, "dust 1e-12 end to end")
            t, acc = sim.tree(), sim.get_points()["acceleration"].astype(np.float64)
        ref = orc.bh_walk_list(t, ics["position"], SD["theta2"], SD["g"], SD["g_soft"])
        bh_list.check_walk(acc, ref, bh_list.LIST_RTOL_F32, what=f"tree build {tb}")
        res[tb] = (t, acc, ref)
    (td, ad, rd), (th, ah, rh) = res[nb.TREE_DEVICE], res[nb.TREE_HOST]
    assert np.array_equal(rd["accepted"], rh["accepted"]) and np.array_equal(rd["visited"], rh["visited"])
    ex = tm.exact_moments(td)
    u = tm.U[np.dtype(np.float32)]
    b = np.zeros(len(td["skip"]))
    absA = np.zeros(len(td["skip"]))
    b[ex["cell"]] = tm.SCHEME_R[np.dtype(np.float32)] + ex["n_c"] + 2.0
    absA[ex["cell"]] = np.sqrt((np.asarray(ex["A"], np.float64) ** 2).sum(axis=1))
    eps2 = float(np.float32(SD["g_soft"]) * np.float32(SD["g_soft"]))
    worst = 0.0
    for i in range(n):
        p = ics["position"][i:i + 1]
        lst = orc.bh_walk_list(td, p, SD["theta2"], SD["g"], SD["g_soft"], list_body=0)["list"]
        assert np.array_equal(lst, orc.bh_walk_list(th, p, SD["theta2"], SD["g"], SD["g_soft"], list_body=0)["list"])
        cm = td["com_mass"][lst].astype(np.float64)
        d = cm[:, :3] - p.astype(np.float64)
        dc = b[lst] * u * absA[lst]
        s = np.sqrt((d * d).sum(axis=1) + eps2)
        tmag = SD["g"] * cm[:, 3] * np.sqrt((d * d).sum(axis=1)) / s ** 3
        s_short = np.maximum(s - dc, 0.0)
        with np.errstate(divide="ignore"):
            D = float((tmag * b[lst] * u + 2.0 * SD["g"] * cm[:, 3] * (1.0 + b[lst] * u) * dc / s_short ** 3)[b[lst] > 0].sum())
        bound = bh_list.LIST_RTOL_F32 * (rd["T"][i] + rh["T"][i]) + D
        diff = float(np.linalg.norm(ad[i] - ah[i]))
        assert diff <= bound, f"body {i}: |a_dev - a_host| = {diff:.3e} beyond {bound:.3e} (moment term {D:.3e})"
        worst = max(worst, diff / bound if bound > 0 else 0.0)
    print(f"dust 1e-12 end to end: worst |a_dev - a_host| / bound = {worst:.3g}")
