"""The spatial ranks' node-list checker (tests/let_list.py), on the CPU.  Held arrays are cut from the oracle's tree of a
3 000-body Plummer sphere: three key ranges (thirds of the leaves in pre-order), a cell owned by the rank of its first body,
cells that span ranks sent to everybody, private nodes exported to a partner when every ancestor could be opened from the
partner's bounding box (the walk's own opening rule at the box's nearest point), each rank's nodes laid out in global-index
order with links turned into positions.  The honest world passes all five checks with both leaf rules, pruned and
unpruned; each planted fault is rejected by the check named for it.  The share of (body, node) terms individually
detectable at the chosen R is printed (pytest -s)."""
import copy

import numpy as np
import pytest

import let_list
import tree_moments
from bh_list import terms
from let_list import LET_LIST_RTOL_F32, check_world, rank_input, replay, world_failures

BOX = ((0.0, 0.0, 0.0), 64.0)
G, EPS, THETA2 = 1.0, 0.01, 0.25
N, RANKS = 3000, 3
_cache = {}


def rounded_tree(nb, orc):
    """The oracle's tree of the sphere with every internal cell's moments replaced by the exact ones, rounded once to f32
    (the oracle folds a cell's bodies in f32, (n_c + 2) u: a tree that is held to 1.5 u needs better)."""
    rec = nb.plummer(N, seed=20250611).astype(orc.P32)
    tree = orc.bh_build_tree(rec, *BOX)
    ex = tree_moments.exact_moments(tree)
    tree["com_mass"][ex["cell"], :3] = ex["X"].astype(np.float32)
    tree["com_mass"][ex["cell"], 3] = ex["M"].astype(np.float32)
    return rec, tree


def cut_world(orc, rec, tree, leaf_mode, prune, n_ranks=RANKS):
    """The rank_input records of n_ranks ranks cut from `tree`, with the replay's own sums as accelerations and counts."""
    skip = tree["skip"].astype(np.int64)
    m = len(skip)
    idx = np.arange(m)
    leaves = np.flatnonzero(skip == idx + 1)
    n = len(leaves)
    first, last = np.searchsorted(leaves, idx, side="left"), np.searchsorted(leaves, skip, side="left")
    cuts = tree_moments.rank_cuts(n, n_ranks)
    rank_of_leaf = np.searchsorted(cuts[1:], np.arange(n), side="right")
    owner = rank_of_leaf[first]
    spanning = rank_of_leaf[last - 1] != owner
    parent = let_list.tree_shape(skip)["parent"]
    cm = tree["com_mass"].astype(np.float64)
    w2 = tree["width"].astype(np.float64) ** 2
    ranks = []
    for r in range(n_ranks):
        mine = leaves[cuts[r]:cuts[r + 1]]
        pos = tree["com_mass"][mine, :3]
        lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
        d = cm[:, :3] - np.clip(cm[:, :3], lo, hi)
        could_open = ~(w2 < THETA2 * (d * d).sum(1) * (1.0 - 1e-4)) if prune else np.ones(m, bool)
        reach = np.ones(m, bool)
        for i in range(1, m):
            reach[i] = reach[parent[i]] and could_open[parent[i]]
        keep = (owner == r) | spanning | reach
        gi = np.flatnonzero(keep)
        origin = np.where(owner[gi] == r, 0, 1) + 2 * spanning[gi]
        held = dict(com_mass=tree["com_mass"][gi].copy(), width=tree["width"][gi].copy(), global_index=gi.astype(np.int32),
                    leaf=(skip[gi] == gi + 1), origin=origin.astype(np.int32))
        relink(held, skip)
        ref = replay(orc, held, pos, THETA2, G, EPS, leaf_mode)
        ranks.append(rank_input(held, pos, ref["S"].astype(np.float32), ref["accepted"].sum(), ref["visited"].sum(),
                                np.count_nonzero(owner[gi] == r), np.count_nonzero(owner[gi] != r)))
    return ranks


def relink(held, one_skip):
    """links = positions, as the receiver lays a list out: the number of held nodes before the node the tree links to"""
    gi = held["global_index"].astype(np.int64)
    held["skip"] = np.where(held["leaf"], np.arange(len(gi)) + 1, np.searchsorted(gi, np.asarray(one_skip, np.int64)[gi], side="left")).astype(np.int32)


def without(held, p, one_skip):
    """the held array with position p left out (the receiver never saw the record)"""
    out = {k: np.delete(v, p, axis=0) for k, v in held.items()}
    relink(out, one_skip)
    return out


def world(nb, orc, leaf_mode, prune=True):
    key = (leaf_mode, prune)
    if key not in _cache:
        if "tree" not in _cache:
            rec, tree = rounded_tree(nb, orc)
            _cache["tree"] = (rec, tree, let_list.one_tree_facts(tree))
        rec, tree, facts = _cache["tree"]
        _cache[key] = (cut_world(orc, rec, tree, leaf_mode, prune), tree, facts)
    ranks, tree, facts = _cache[key]
    return copy.deepcopy(ranks), tree, facts


def tripped(orc, ranks, tree, facts, leaf_mode):
    fails, _ = world_failures(orc, ranks, tree, THETA2, G, EPS, leaf_mode, facts, what="planted")
    return {c for c, msgs in fails.items() if msgs}, fails


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("leaf_mode", [0, 1])
def test_honest_world_passes(nb, orc, leaf_mode, prune):
    ranks, tree, facts = world(nb, orc, leaf_mode, prune)
    info = check_world(orc, ranks, tree, THETA2, G, EPS, leaf_mode, facts, what=f"leaf={leaf_mode} prune={prune}")
    sizes = [len(rk["held"]["width"]) for rk in ranks]
    print(f"\n[let list] leaf={leaf_mode} prune={prune}: held {sizes} of {len(tree['width'])} nodes, worst |a - S| / T {info['worst']:.2e}, "
          f"moments {info['moments'][0]:.2f} u / {info['moments'][1]:.2f} u")
    assert info["worst"] < LET_LIST_RTOL_F32 / 3 and max(info["moments"]) <= 1.0
    if prune:
        assert min(sizes) < 0.9 * len(tree["width"])   # the pruning leaves nodes out (the middle range's box spans the sphere)
    else:
        assert sizes == [len(tree["width"])] * RANKS


def visited_import(orc, rk, tree, leaf_mode, want_leaf):
    """(position, body) of the imported private node with the largest accepted term of any own body"""
    held = rk["held"]
    best = (0.0, -1, -1)
    for b in range(0, len(rk["pos"]), 37):
        lst = orc.bh_walk_list(dict(com_mass=held["com_mass"], width=held["width"], skip=held["skip"]), rk["pos"][b:b + 1], THETA2, G, EPS,
                               leaf_mode, 1, list_body=0)["list"]
        lst = lst[(held["origin"][lst] == 1) & (held["leaf"][lst] == want_leaf)]
        if len(lst):
            mag = np.linalg.norm(terms(held, rk["pos"][b], lst, G, EPS), axis=1)
            if mag.max() > best[0]:
                best = (float(mag.max()), int(lst[np.argmax(mag)]), b)
    assert best[1] >= 0
    return best[1], best[2]


@pytest.mark.parametrize("leaf_mode", [0, 1])
def test_an_import_node_removed_fails(nb, orc, leaf_mode):
    ranks, tree, facts = world(nb, orc, leaf_mode)
    p, b = visited_import(orc, ranks[1], tree, leaf_mode, want_leaf=True)
    ranks[1]["held"] = without(ranks[1]["held"], p, tree["skip"])
    hit, fails = tripped(orc, ranks, tree, facts, leaf_mode)
    print(f"\n[let list] leaf={leaf_mode}: import at position {p} removed -> {sorted(hit)}")
    assert {"walk", "closure", "partition"} <= hit and "structure" not in hit, fails
    assert any(f"body {b}" in line or "bodies" in line for line in fails["closure"])


@pytest.mark.parametrize("leaf_mode", [0, 1])
def test_a_node_duplicated_fails(nb, orc, leaf_mode):
    ranks, tree, facts = world(nb, orc, leaf_mode)
    p, _ = visited_import(orc, ranks[0], tree, leaf_mode, want_leaf=True)
    held = ranks[0]["held"]
    held = {k: np.insert(v, p, v[p], axis=0) for k, v in held.items()}
    relink(held, tree["skip"])
    held["skip"][p] = p + 1        # (the copy is walked too: its term counts twice)
    ranks[0]["held"] = held
    hit, fails = tripped(orc, ranks, tree, facts, leaf_mode)
    print(f"\n[let list] leaf={leaf_mode}: node at position {p} duplicated -> {sorted(hit)}")
    assert {"structure", "walk", "counts"} <= hit, fails
    assert any("not strictly ascending" in line for line in fails["structure"])


@pytest.mark.parametrize("leaf_mode", [0, 1])
def test_a_spanning_cell_with_a_neighbours_mass_fails(nb, orc, leaf_mode):
    ranks, tree, facts = world(nb, orc, leaf_mode)
    held = ranks[2]["held"]
    tops = np.flatnonzero(held["origin"] >= 2)
    assert len(tops) >= 2
    p = int(tops[-1])              # the deepest spanning cell this rank holds, given the mass of the one before it
    held["com_mass"][p, 3] = held["com_mass"][int(tops[-2]), 3]
    hit, fails = tripped(orc, ranks, tree, facts, leaf_mode)
    print(f"\n[let list] leaf={leaf_mode}: spanning cell {int(held['global_index'][p])} with a neighbour's mass -> {sorted(hit)}")
    assert "structure" in hit and "exact moments" in fails["structure"][0], fails
    assert not hit & {"counts", "closure", "partition"}


@pytest.mark.parametrize("leaf_mode", [0, 1])
@pytest.mark.parametrize("origin", [0, 1, 2])
def test_a_centre_moved_by_two_ulp_trips_the_structure_check_alone(nb, orc, leaf_mode, origin):
    ranks, tree, facts = world(nb, orc, leaf_mode)
    held = ranks[1]["held"]
    cells = np.flatnonzero((held["origin"] == origin) & ~held["leaf"])
    p = int(cells[len(cells) // 2])
    x = held["com_mass"][p, 0]
    held["com_mass"][p, 0] = np.nextafter(np.nextafter(x, np.float32(np.inf)), np.float32(np.inf))
    hit, fails = tripped(orc, ranks, tree, facts, leaf_mode)
    print(f"\n[let list] leaf={leaf_mode}: centre of node {int(held['global_index'][p])} (origin {origin}) moved by 2 ulp -> {sorted(hit)}")
    assert hit == {"structure"}, fails
    assert len(fails["structure"]) == 1 and "1 cells beyond" in fails["structure"][0]


@pytest.mark.parametrize("leaf_mode", [0, 1])
def test_an_opened_nodes_child_removed_trips_the_closure(nb, orc, leaf_mode):
    ranks, tree, facts = world(nb, orc, leaf_mode)
    rk = ranks[0]
    held = rk["held"]
    # an imported internal cell that some own body accepts: its parent was opened, so the cell is a child the walk needs
    p, b = visited_import(orc, rk, tree, leaf_mode, want_leaf=False)
    below = np.flatnonzero((held["global_index"] > held["global_index"][p]) & (held["global_index"] < tree["skip"][held["global_index"][p]]))
    rk["held"] = without(held, np.concatenate([[p], below]), tree["skip"])   # the cell and what hangs below it
    hit, fails = tripped(orc, ranks, tree, facts, leaf_mode)
    print(f"\n[let list] leaf={leaf_mode}: opened node's child at position {p} removed -> {sorted(hit)}: {fails['closure'][0]}")
    assert "closure" in hit and "structure" not in hit, fails
    assert "rank 0" in fails["closure"][0] and "opens node" in fails["closure"][0] and "children" in fails["closure"][0]


@pytest.mark.parametrize("which", ["interactions", "node_visits"])
@pytest.mark.parametrize("delta", [-1, 1])
def test_counts_off_by_one_fail(nb, orc, which, delta):
    ranks, tree, facts = world(nb, orc, 0)
    ranks[2][which] += delta
    hit, fails = tripped(orc, ranks, tree, facts, 0)
    assert hit == {"counts"} and "rank 2" in fails["counts"][0], fails


def test_a_nodes_local_count_off_by_one_fails(nb, orc):
    ranks, tree, facts = world(nb, orc, 0)
    ranks[0]["nodes_received"] += 1
    hit, fails = tripped(orc, ranks, tree, facts, 0)
    assert hit == {"partition"}, fails


def test_one_bodys_dropped_term_fails_the_walk_alone(nb, orc):
    ranks, tree, facts = world(nb, orc, 0)
    rk = ranks[1]
    p, b = visited_import(orc, rk, tree, 0, want_leaf=False)
    t = terms(rk["held"], rk["pos"][b], [p], G, EPS)[0]
    rk["acc"][b] = (rk["acc"][b].astype(np.float64) - t).astype(np.float32)
    hit, fails = tripped(orc, ranks, tree, facts, 0)
    assert hit == {"walk"} and f"first [{b}]" in fails["walk"][0], fails


def test_detectable_share(nb, orc):
    """The share of a rank's accepted (body, node) terms above 2 R T_i, over every third body of every rank."""
    for leaf_mode in (0, 1):
        ranks, tree, facts = world(nb, orc, leaf_mode)
        tot = det = tot_in = det_in = 0
        for rk in ranks:
            held = rk["held"]
            as_tree = dict(com_mass=held["com_mass"], width=held["width"], skip=held["skip"])
            ref = replay(orc, held, rk["pos"], THETA2, G, EPS, leaf_mode)
            for b in range(0, len(rk["pos"]), 3):
                lst = orc.bh_walk_list(as_tree, rk["pos"][b:b + 1], THETA2, G, EPS, leaf_mode, 1, list_body=0)["list"]
                mag = np.linalg.norm(terms(held, rk["pos"][b], lst, G, EPS), axis=1)
                seen = mag > 2 * LET_LIST_RTOL_F32 * ref["T"][b]
                imp = held["origin"][lst] % 2 == 1
                det, tot = det + int(seen.sum()), tot + len(mag)
                det_in, tot_in = det_in + int(seen[imp].sum()), tot_in + int(imp.sum())
        print(f"\n[let list] leaf={leaf_mode}: {det / tot:.1%} of {tot} terms individually detectable at R = {LET_LIST_RTOL_F32:g} "
              f"({det_in / tot_in:.1%} of the {tot_in} imported ones)")
        assert det / tot > 0.65


# ---------------------------------------------------------------------------------------------- light and massless cells on a boundary
# The planted fault here is a whole scheme: the spanning cells' moments formed from per-rank f64 prefix sums, the owner's part a
# difference of two of them (tree_moments.rank_prefix_moments: what the spatial build did while it read the high parts of its
# double-double prefixes only).  On worlds of comparable masses that is a correctly rounded store; behind a sun it is not.
def planted_world(nb, orc, ics, n_ranks, residue_ulps=0.0):
    """(ranks, tree, facts, planted com_mass): the oracle's tree of `ics` with exact moments rounded once (rounded_tree), and
    ranks cut from it after rank_prefix_moments replaced the spanning cells' moments; `tree` and `facts` are the honest ones."""
    rec = ics.astype(orc.P32)
    tree = orc.bh_build_tree(rec, *BOX)
    ex = tree_moments.exact_moments(tree)
    tree["com_mass"][ex["cell"], :3] = ex["X"].astype(np.float32)
    tree["com_mass"][ex["cell"], 3] = ex["M"].astype(np.float32)
    row = np.full(len(tree["skip"]), -1, np.int64)
    row[ex["cell"]] = np.arange(len(ex["cell"]))
    facts = dict(shape=let_list.tree_shape(tree["skip"]), exact=ex, row=row)
    planted = tree_moments.rank_prefix_moments(tree, n_ranks, residue_ulps)
    ranks = cut_world(orc, rec, dict(tree, com_mass=planted), 0, True, n_ranks)
    return ranks, tree, facts, planted


def held_as(ranks, node):
    """origin of `node` on every rank (-1: not held)"""
    out = []
    for rk in ranks:
        at = np.flatnonzero(rk["held"]["global_index"] == node)
        out.append(int(rk["held"]["origin"][at[0]]) if len(at) else -1)
    return out


@pytest.mark.parametrize("dust", tree_moments.LET_DUST_MASSES)
@pytest.mark.parametrize("n_ranks,n", tree_moments.LET_DUST_CASES)
def test_prefix_difference_spanning_cells_fail_on_dust(nb, orc, n_ranks, n, dust):
    """Every (ranks, n, dust) of the GPU test: the structure check trips on the planted scheme, alone, names spanning cells only,
    and at least one held spanning cell lies more than 10 LET_MOMENT_R u from its exact moments (a condition on the inputs: a
    lucky rounding on the device cannot hide a fault of that size)."""
    ranks, tree, facts, _ = planted_world(nb, orc, tree_moments.dust_world(nb, n, dust), n_ranks)
    hit, fails = tripped(orc, ranks, tree, facts, 0)
    assert hit == {"structure"}, fails
    lines = [line for line in fails["structure"] if "exact moments" in line]
    assert lines and len(lines) == len(fails["structure"]), fails
    for line in lines:
        origins = [int(v) for v in line.split("origins [")[1].split("]")[0].split(",")]
        assert origins and min(origins) >= 2, line
    worst = 0.0
    for r, rk in enumerate(ranks):
        h = rk["held"]
        tops = np.flatnonzero(h["origin"] >= 2)
        only = {k: v[tops] for k, v in h.items()}
        relink(only, tree["skip"])
        _, (rm, rc) = let_list.structure_failures(only, tree, facts, f"rank {r}")
        worst = max(worst, rm, rc)
    print(f"\n[let list] dust {dust:g} on {n_ranks} ranks, n={n}: planted spanning cells up to {worst:.3g} u from their exact moments")
    assert worst > 10 * let_list.LET_MOMENT_R


@pytest.mark.parametrize("own_side_only", [False, True])
@pytest.mark.parametrize("n_ranks,n,r", tree_moments.LET_MASSLESS_CASES)
def test_massless_boundary_worlds(nb, orc, n_ranks, n, r, own_side_only):
    """control_world with a massless cell across boundary r (or one whose owner's part is massless).  A prefix sum does not move
    when a massless body is added, so the planted scheme leaves an own part of exactly 0 there -- and so does the device, whose
    high parts are the doubles nearest to two prefixes of the same exact value: mass +0 and 0 / 0, the single tree's values, and
    the planted arrays pass.  With one ulp of the owner's prefix left in that part (two prefixes that associate differently and
    are not correctly rounded) the cell gets a mass and a finite centre, and the massless check names it."""
    base = tree_moments.control_world(nb, n)
    tree0 = orc.bh_build_tree(base.astype(orc.P32), *BOX)
    ics, node = tree_moments.massless_boundary(base, tree0, n_ranks, r, own_side_only)
    ranks, tree, facts, planted = planted_world(nb, orc, ics, n_ranks)
    assert np.array_equal(tree["skip"], tree0["skip"]) and np.array_equal(tree["com_mass"][:, :3][tree["skip"] == np.arange(len(tree["skip"])) + 1],
                                                                          tree0["com_mass"][:, :3][tree0["skip"] == np.arange(len(tree0["skip"])) + 1])
    held = held_as(ranks, node)
    assert held[r - 1] == 2 and held[r] == 3 and all(o in (-1, 3) for q, o in enumerate(held) if q != r - 1), held
    M = facts["exact"]["M"][facts["row"][node]]
    assert (M != 0) == own_side_only
    hit, fails = tripped(orc, ranks, tree, facts, 0)
    assert not hit, fails
    if not own_side_only:
        assert planted[node, 3] == 0 and not np.signbit(planted[node, 3]) and np.isnan(planted[node, :3]).all()
        for sign in (1.0, -1.0):
            ranks, _, _, planted = planted_world(nb, orc, ics, n_ranks, residue_ulps=sign)
            assert planted[node, 3] != 0 and np.sign(planted[node, 3]) == sign
            hit, fails = tripped(orc, ranks, tree, facts, 0)
            assert "structure" in hit and any("massless cells differ" in line and str(node) in line for line in fails["structure"]), fails


@pytest.mark.parametrize("name,n_ranks,n", [("control", 2, 300), ("control", 3, 1025), ("control", 3, 5000), ("plummer", 2, 300), ("plummer", 3, 1001),
                                            ("plummer", 5, 64), ("plummer", 8, 300), ("plummer", 4, 4097)])
def test_prefix_difference_spanning_cells_pass_on_the_old_worlds(nb, orc, name, n_ranks, n):
    """control_world and the Plummer worlds of tests/test_let_walk_list_gpu.py: the planted scheme passes every check there, at
    the same LET_MOMENT_R.  The worlds above add a check that these never made."""
    ics = tree_moments.control_world(nb, n) if name == "control" else nb.plummer(n, seed=700 + n)
    ranks, tree, facts, _ = planted_world(nb, orc, ics, n_ranks)
    info = check_world(orc, ranks, tree, THETA2, G, EPS, 0, facts, what=f"{name} n={n} on {n_ranks} ranks, planted")
    print(f"\n[let list] {name} n={n} on {n_ranks} ranks, planted prefix differences: moments {info['moments'][0]:.3f} u / {info['moments'][1]:.3f} u")
    assert max(info["moments"]) <= let_list.LET_MOMENT_R
