"""Checking a spatial rank's Barnes-Hut walk against the f64 sum of the node list that rank held.

A NBODY_SHARD_SPATIAL rank walks "its slice and the imports in global-index order" (nbody_let.cpp, launch_assemble): an
array no single-handle walk ever sees, produced by the distributed device build, the spanning cells and the pruned export.
Simulation.let_held() (nbody_debug_let_export_held) copies that array out as the walk read it.  As tests/bh_list.py does for
one handle, oracle.bh_walk_list replays the walk's opening tests over it for the rank's own bodies -- same f32 expressions,
same theta2, g, g_soft and leaf rule, following the held links -- and sums the accepted terms in f64: S_i, T_i and per-body
accepted / visited counts.  From the exports of all G ranks and the single-handle device tree of the same bodies (`one`:
Simulation.tree()) five checks are made; none has an allowance for a flipped opening test:

  walk       |a_i - S_i| <= R T_i for every own body of every rank (bh_list.check_walk), no body exempt.
  counts     a rank's stats().interactions and node_visits equal its replay's sums exactly.
  structure  the held global indices ascend strictly; every held node is the node of `one` at that index: same width bits,
             same leaf flag, a leaf the same bits (a bit copy of a body), a link that is the number of held nodes before the
             node `one` links to; an internal cell's mass and centre lie within LET_MOMENT_R roundings of the EXACT moments of
             the cell's bodies (tests/tree_moments.py: exact_moments of `one`'s leaves) -- not of the other build's values.
  closure    the pruning contract.  A second replay, in numpy, goes down `one`'s parent structure instead of the held links:
             a body visits a held node iff it opened the node's parent.  Every node a body opens must have ALL its children
             (the nodes that have it as parent in `one`) in the held array; a missing child names the rank, the body and the
             node.  The two replays' per-body accepted and visited counts must agree, which is what makes a link that leads
             past a needed child, or a cell the DIRECT walk takes for a leaf because nothing below it was sent, a failure
             and not a silent accept.
  partition  the private slice nodes of all ranks plus the spanning cells (each in its owner's slice) cover every global
             index exactly once; imported spanning cells are spanning cells of other ranks; a rank's slice and import sizes
             equal NbodyLetStats.nodes_local and nodes_received of that pass.

What the walk check can see is bh_list's: a term dropped, doubled or mis-weighted moves a_i by |t_ij|, detectable above
2 R T_i (tests/test_let_list_checker.py prints the share); what is below it is left to the exact counts and the closure.

This module is plain test infrastructure (numpy, the CPU oracle; no GPU): tests/test_let_list_checker.py runs it on held
arrays cut from the oracle's tree and on planted faults, tests/test_let_walk_list_gpu.py on the ranks themselves.
"""
from __future__ import annotations

import numpy as np

import tree_moments
from bh_list import LIST_RTOL_F32, walk_errors

#: |a_i - S_i| <= R T_i.  Worst measured on an MI355X over every case of tests/test_let_walk_list_gpu.py: 4.44e-7 (the 1e-12
#: dust of 5 000 bodies on 3 ranks, the reference's leaf rule; the dust worlds lie between 2.7e-7 and 4.4e-7, the world with
#: 1 500 bodies inside one level-16 cell at 2.5e-7, the Plummer worlds of 64 to 20 000 bodies on 2 to 8 ranks between 1.0e-7
#: and 2.3e-7, pruned and unpruned alike).  That is below a third of bh_list.LIST_RTOL_F32 (1.5e-6), so the spatial walk is
#: held to the same constant as the single-handle walks; the margin over the measured worst is 10x.
LET_LIST_RTOL_F32 = LIST_RTOL_F32
#: worst measured, same run: |a - S| / T, and the internal held cells' (mass, centre) against their exact moments in units of u
LET_WORST_MEASURED = dict(walk=4.44e-7, moments=(0.992, 0.999))

#: an internal held cell against the exact moments of its bodies, in units of u = 2^-24 of the scale (|M| for the mass, A_a =
#: sum m |x_a| / M for a centre).  The count, as in tree_moments: sums and the quotient are formed in f64 (2^-53 each: 2^-27 u
#: together) and stored once in f32: at most 1 u (half an ulp).  A rank's own part of a spanning cell is a difference of two of
#: its prefix sums and carries the rounding of everything the rank holds before the cell: r = c P_a / (A_a M) u with P_a the
#: sum over the rank's bodies sorted before the cell's end.  Taken in double-double (k_let_contrib: dd4_diff, as the single
#: build's cells) c = 2^-75 and r is below 1e-7 u even for 1e-15 dust behind a sun; the later ranks' parts are prefixes from
#: their first body, all inside the cell, nothing subtracted.  (With the high parts alone c was 2^-29: below 0.01 u on worlds
#: of comparable masses, but 1e3 u for 1e-12 dust behind a mass of 1 and 1e6 u for 1e-15 dust; measured on the dust worlds of
#: tests/test_let_walk_list_gpu.py before the change: up to 1.1e3 / 1.5e3 u and 9.3e5 / 1.4e6 u)  The bound is
#: 1 + 2^-27 + r with half a unit of room, so a centre moved by 2 ulp (off by at least 1.5 ulp > 1.5 u |x|) is caught in every
#: cell that does not straddle a coordinate plane.  Worst measured over all cases, the dust and massless worlds included:
#: 0.999 u (LET_WORST_MEASURED): a correctly rounded store and nothing else.
LET_MOMENT_R = 1.5

CHECKS = ("walk", "counts", "structure", "closure", "partition")
U32 = 2.0 ** -24


def tree_shape(skip) -> dict:
    """`parent` (-1 for the root), `depth` and `nchild` of every node of a pre-order skip list."""
    sk = np.asarray(skip, np.int64).tolist()
    m = len(sk)
    parent, depth, stack = [-1] * m, [0] * m, []
    for i in range(m):
        while stack and sk[stack[-1]] <= i:
            stack.pop()
        if stack:
            parent[i], depth[i] = stack[-1], len(stack)
        if sk[i] != i + 1:
            stack.append(i)
    parent = np.asarray(parent, np.int64)
    nchild = np.bincount(parent[parent >= 0], minlength=m) if m else np.zeros(0, np.int64)
    return dict(parent=parent, depth=np.asarray(depth, np.int64), nchild=nchild)


def rank_input(held, pos, acc, interactions, node_visits, nodes_local, nodes_received) -> dict:
    """What the checks need of one rank: let_held(), the own bodies' walk positions and accelerations (same order), the
    pass's stats() totals and its NbodyLetStats node counts."""
    return dict(held=held, pos=np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 3)),
                acc=np.asarray(acc, np.float32).reshape(-1, 3), interactions=int(interactions), node_visits=int(node_visits),
                nodes_local=int(nodes_local), nodes_received=int(nodes_received))


def links_walkable(held) -> bool:
    """Every link leads forward and not beyond the array's end (what makes the replay end)."""
    sk = np.asarray(held["skip"], np.int64)
    return bool(np.all(sk > np.arange(len(sk))) and np.all(sk <= len(sk)))


def replay(orc, held, pos, theta2, g, g_soft, leaf_mode, threads=16) -> dict:
    """oracle.bh_walk_list over the held array, following its links: S, T, accepted, visited per body."""
    tree = dict(com_mass=np.ascontiguousarray(held["com_mass"], np.float32), width=held["width"], skip=held["skip"])
    return orc.bh_walk_list(tree, pos, theta2, g, g_soft, leaf_mode, threads)


def one_tree_facts(one) -> dict:
    """Of the single-handle tree: its shape, its exact moments and, per node, the row of its cell in them (-1: a leaf)."""
    shape = tree_shape(one["skip"])
    exact = tree_moments.exact_moments(one)
    row = np.full(len(one["skip"]), -1, np.int64)
    row[exact["cell"]] = np.arange(len(exact["cell"]))
    return dict(shape=shape, exact=exact, row=row)


def indices_valid(held, one) -> bool:
    gi = np.asarray(held["global_index"], np.int64)
    return bool(len(gi) == 0 or (gi[0] >= 0 and gi[-1] < len(one["skip"]) and np.all(np.diff(gi) > 0)))


def structure_failures(held, one, facts, what) -> tuple:
    """(messages, (worst mass ratio, worst centre ratio) of the internal cells in units of u)."""
    out = []
    gi = np.asarray(held["global_index"], np.int64)
    m = len(gi)
    if not set(np.unique(held["origin"]).tolist()) <= {0, 1, 2, 3}:
        out.append(f"{what}: origins {np.unique(held['origin']).tolist()}")
    if not links_walkable(held):
        bad = np.flatnonzero(~((held["skip"] > np.arange(m)) & (held["skip"] <= m)))
        out.append(f"{what}: links that do not lead forward inside the array at positions {bad[:6].tolist()}")
    if not indices_valid(held, one):
        asc = np.flatnonzero(np.diff(gi) <= 0)
        out.append(f"{what}: global indices not strictly ascending inside [0, {len(one['skip'])}): after positions {asc[:6].tolist()}, "
                   f"first {gi[:1].tolist()}, last {gi[-1:].tolist()}")
        return out, (0.0, 0.0)
    if m == 0:
        return out, (0.0, 0.0)
    one_skip = np.asarray(one["skip"], np.int64)
    one_leaf = one_skip[gi] == gi + 1
    cm = np.asarray(held["com_mass"], np.float32)
    ocm = np.asarray(one["com_mass"], np.float32)
    bad = np.flatnonzero(np.asarray(held["width"], np.float32).view(np.uint32) != np.asarray(one["width"], np.float32)[gi].view(np.uint32))
    if len(bad):
        out.append(f"{what}: width bits differ from the single-handle tree's at global indices {gi[bad[:6]].tolist()}")
    bad = np.flatnonzero(np.asarray(held["leaf"], bool) != one_leaf)
    if len(bad):
        out.append(f"{what}: leaf flags differ from the single-handle tree's at global indices {gi[bad[:6]].tolist()}")
    want_link = np.where(one_leaf, np.arange(m) + 1, np.searchsorted(gi, one_skip[gi], side="left"))
    bad = np.flatnonzero(np.asarray(held["skip"], np.int64) != want_link)
    if len(bad):
        out.append(f"{what}: links differ from the single-handle tree's skip structure at global indices {gi[bad[:6]].tolist()}: "
                   f"{np.asarray(held['skip'])[bad[:6]].tolist()} for {want_link[bad[:6]].tolist()}")
    lf = np.flatnonzero(one_leaf)
    bad = lf[(cm[lf].view(np.uint32) != ocm[gi[lf]].view(np.uint32)).any(axis=1)]
    if len(bad):
        out.append(f"{what}: leaves that are not the single-handle tree's bits at global indices {gi[bad[:6]].tolist()}")
    cells = np.flatnonzero(~one_leaf)
    ex = facts["exact"]
    rows = facts["row"][gi[cells]]
    assert (rows >= 0).all()
    M, X, A = ex["M"][rows], ex["X"][rows], ex["A"][rows]
    live = M != 0
    dead = cells[~live]   # massless cells: the single-handle tree's bits
    bad = dead[(cm[dead].view(np.uint32) != ocm[gi[dead]].view(np.uint32)).any(axis=1)]
    if len(bad):
        out.append(f"{what}: massless cells differ from the single-handle tree's at global indices {gi[bad[:6]].tolist()}")
    got = cm[cells][live].astype(np.longdouble)
    u = np.longdouble(U32)

    def ratio(err, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(scale > 0, err / np.where(scale > 0, u * scale, 1), np.where(err == 0, 0.0, np.inf))
        return np.where(np.isfinite(err), r, np.inf).astype(np.float64)

    rm = ratio(np.abs(got[:, 3] - M[live]), np.abs(M[live]))
    rc = ratio(np.abs(got[:, :3] - X[live]), A[live]).reshape(-1, 3).max(axis=1, initial=0.0)
    bad = np.flatnonzero(~((rm <= LET_MOMENT_R) & (rc <= LET_MOMENT_R)))
    if len(bad):
        at = gi[cells[live][bad]]
        out.append(f"{what}: {len(bad)} cells beyond {LET_MOMENT_R} u of their exact moments: global indices {at[:6].tolist()}, origins "
                   f"{np.asarray(held['origin'])[cells[live][bad[:6]]].tolist()}, mass ratios {rm[bad[:6]].tolist()}, centre ratios {rc[bad[:6]].tolist()}")
    return out, (float(rm.max(initial=0.0)), float(rc.max(initial=0.0)))


def structural_replay(held, one, facts, pos, theta2, leaf_mode, what, budget=1 << 24) -> dict:
    """The walk's decisions made down the single-handle tree's PARENT structure over the held nodes (f32, the oracle's
    expressions): per-body `accepted` and `visited`, and `missing`: messages for opened nodes that lack a child."""
    gi = np.asarray(held["global_index"], np.int64)
    m, n = len(gi), len(pos)
    acc_n, vis_n = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    missing = []
    if m == 0 or n == 0:
        return dict(accepted=acc_n, visited=vis_n, missing=missing)
    shape = facts["shape"]
    par = shape["parent"][gi]
    at = np.searchsorted(gi, np.maximum(par, 0))
    hp = np.where((par >= 0) & (gi[np.minimum(at, m - 1)] == par), at, -1)   # the parent's position, -1: not held (or the root)
    leaf = np.asarray(held["leaf"], bool)
    held_children = np.bincount(hp[hp >= 0], minlength=m)
    incomplete = ~leaf & (held_children != shape["nchild"][gi])
    depth = shape["depth"][gi]
    levels = [np.flatnonzero(depth == d) for d in np.unique(depth)]
    cm = np.asarray(held["com_mass"], np.float32)
    w = np.asarray(held["width"], np.float32)
    w2 = w * w
    th = np.float32(theta2)
    chunk = max(1, budget // m)
    for b0 in range(0, n, chunk):
        p = pos[b0:b0 + chunk]
        nb = len(p)
        opened = np.zeros((m, nb), bool)
        for J in levels:
            rx, ry, rz = (cm[J, a][:, None] - p[None, :, a] for a in range(3))
            r2 = (rx * rx + ry * ry) + rz * rz
            accept = w2[J][:, None] < th * r2
            visit = np.where((hp[J] >= 0)[:, None], opened[np.maximum(hp[J], 0)], False)
            visit[J == 0] = True   # the walk starts at position 0
            if leaf_mode == 1:
                near = r2 < np.float32(1e-10)
                take = (accept | leaf[J][:, None]) & ~near
                op = visit & ~take & ~near
            else:
                take = accept
                op = visit & ~take
            opened[J] = op
            vis_n[b0:b0 + nb] += visit.sum(axis=0).astype(np.uint64)
            acc_n[b0:b0 + nb] += (visit & take).sum(axis=0).astype(np.uint64)
            if incomplete[J].any() and len(missing) < 4:
                jj, bb = np.nonzero(op & incomplete[J][:, None])
                for j, b in list(zip(jj.tolist(), bb.tolist()))[:4 - len(missing)]:
                    k = J[j]
                    missing.append(f"{what}: body {b0 + b} opens node {int(gi[k])} (position {int(k)}), which has {int(shape['nchild'][gi[k]])} "
                                   f"children in the single-handle tree and {int(held_children[k])} in the held array")
    return dict(accepted=acc_n, visited=vis_n, missing=missing)


def partition_failures(ranks, one, what) -> list:
    out = []
    m1 = len(one["skip"])
    own, tops = [], []
    for r, rk in enumerate(ranks):
        h = rk["held"]
        o = np.asarray(h["origin"])
        gi = np.asarray(h["global_index"], np.int64)
        own.append(gi[(o == 0) | (o == 2)])
        tops.append(gi[o == 2])
        n_slice, n_in = int(np.count_nonzero((o == 0) | (o == 2))), int(np.count_nonzero((o == 1) | (o == 3)))
        if (n_slice, n_in) != (rk["nodes_local"], rk["nodes_received"]):
            out.append(f"{what} rank {r}: holds {n_slice} slice nodes and {n_in} imports, NbodyLetStats says {rk['nodes_local']} and {rk['nodes_received']}")
    cover = np.sort(np.concatenate(own)) if own else np.zeros(0, np.int64)
    if not np.array_equal(cover, np.arange(m1)):
        cnt = np.bincount(cover[(cover >= 0) & (cover < m1)], minlength=m1)
        out.append(f"{what}: the ranks' slices cover {len(cover)} indices for {m1} nodes; uncovered {np.flatnonzero(cnt == 0)[:6].tolist()}, "
                   f"more than once {np.flatnonzero(cnt > 1)[:6].tolist()}")
    all_tops = np.concatenate(tops) if tops else np.zeros(0, np.int64)
    for r, rk in enumerate(ranks):
        h = rk["held"]
        o = np.asarray(h["origin"])
        gi = np.asarray(h["global_index"], np.int64)
        stray = np.setdiff1d(gi[o == 3], np.setdiff1d(all_tops, tops[r]))
        if len(stray):
            out.append(f"{what} rank {r}: imported spanning cells {stray[:6].tolist()} are no other rank's spanning cells")
        stray = np.intersect1d(gi[o == 1], all_tops)
        if len(stray):
            out.append(f"{what} rank {r}: imports {stray[:6].tolist()} marked private are spanning cells")
    return out


def world_failures(orc, ranks, one, theta2, g, g_soft, leaf_mode, facts=None, rtol=LET_LIST_RTOL_F32, what="", threads=16) -> tuple:
    """Run the five checks on a world of ranks (rank_input records).  Returns ({check: [messages]}, info) with info =
    dict(worst=worst |a - S| / T over all bodies, moments=(worst mass, worst centre ratio), refs=[per-rank replay])."""
    facts = facts if facts is not None else one_tree_facts(one)
    fails = {c: [] for c in CHECKS}
    worst, worst_m, worst_c, refs = 0.0, 0.0, 0.0, []
    for r, rk in enumerate(ranks):
        tag = f"{what} rank {r}"
        held = rk["held"]
        msgs, (rm, rc) = structure_failures(held, one, facts, tag)
        fails["structure"] += msgs
        worst_m, worst_c = max(worst_m, rm), max(worst_c, rc)
        if not links_walkable(held):
            refs.append(None)
            continue
        if len(held["width"]) == 0 and len(rk["pos"]):
            fails["structure"].append(f"{tag}: {len(rk['pos'])} bodies and no node")
            refs.append(None)
            continue
        ref = replay(orc, held, rk["pos"], theta2, g, g_soft, leaf_mode, threads)
        refs.append(ref)
        if len(rk["acc"]) != len(rk["pos"]):
            fails["walk"].append(f"{tag}: {len(rk['acc'])} accelerations for {len(rk['pos'])} bodies")
        else:
            err = walk_errors(rk["acc"], ref)
            worst = max(worst, float(err.max(initial=0.0)))
            bad = np.flatnonzero(~(err <= rtol))
            if len(bad):
                fails["walk"].append(f"{tag}: {len(bad)} of {len(err)} bodies beyond {rtol:g} T_i, first {bad[:8].tolist()} at {err[bad[:8]].tolist()}")
        a, v = int(ref["accepted"].sum()), int(ref["visited"].sum())
        if (rk["interactions"], rk["node_visits"]) != (a, v):
            fails["counts"].append(f"{tag}: accepted {rk['interactions']} visited {rk['node_visits']}, the node list gives {a} and {v}")
        if indices_valid(held, one):
            sr = structural_replay(held, one, facts, rk["pos"], theta2, leaf_mode, tag)
            fails["closure"] += sr["missing"]
            bad = np.flatnonzero((sr["accepted"] != ref["accepted"]) | (sr["visited"] != ref["visited"]))
            if len(bad):
                b = int(bad[0])
                fails["closure"].append(f"{tag}: {len(bad)} bodies walk the held links otherwise than the tree's structure, first body {b}: accepted "
                                        f"{int(ref['accepted'][b])} visited {int(ref['visited'][b])} by the links, {int(sr['accepted'][b])} and {int(sr['visited'][b])} by the structure")
    if all(indices_valid(rk["held"], one) for rk in ranks):
        fails["partition"] += partition_failures(ranks, one, what)
    else:
        fails["partition"].append(f"{what}: not checked, a rank's global indices are invalid")
    return fails, dict(worst=worst, moments=(worst_m, worst_c), refs=refs)


def check_world(orc, ranks, one, theta2, g, g_soft, leaf_mode, facts=None, rtol=LET_LIST_RTOL_F32, what="") -> dict:
    """Assert all five checks; returns world_failures' info."""
    fails, info = world_failures(orc, ranks, one, theta2, g, g_soft, leaf_mode, facts, rtol, what)
    bad = {c: m for c, m in fails.items() if m}
    if bad:
        raise AssertionError("\n".join(f"[{c}] {line}" for c, m in bad.items() for line in m[:6]))
    return info


def check_counts(ranks_stats, refs, what=""):
    """Per rank: stats() totals equal the replay's sums exactly (for tests that have the replays already)."""
    for r, (s, ref) in enumerate(zip(ranks_stats, refs)):
        a, v = int(ref["accepted"].sum()), int(ref["visited"].sum())
        assert (s.interactions, s.node_visits) == (a, v), \
            f"{what} rank {r}: accepted {s.interactions} visited {s.node_visits}, the node list gives {a} and {v}"
