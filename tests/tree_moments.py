"""Checking an exported tree's masses and centres of mass, cell by cell, against exact sums.

The other checkers (bh_list, pot_list, field_list, tidal_list, quad_list) replay a handle's OWN exported tree, so they take
its moments as given.  This one checks the moments themselves.  Input is Simulation.tree() (or a host / oracle build of the
same shape): `com_mass` [nodes, 4], `width`, `skip`, pre-order.  A node with skip[i] == i + 1 is a leaf and a bit copy of a
body (the build tests assert that); the bodies of cell i are therefore the leaves in (i, skip[i]).  For every internal cell

    M = sum m,    X_a = sum m x_a / M,    A_a = sum m |x_a| / M        (a = x, y, z; over the cell's own leaves only)

with every sum exact: each product m x is split into the double nearest to it and its error (Dekker; for f32-representable
m and x the error is 0), `math.fsum` returns the double nearest to the exact sum of those terms and, run once more with that
double negated among the terms, the remainder; the two go into one np.longdouble and the one division is made there.  No
difference of prefix sums is taken anywhere: that is the scheme under test.  What is left of reference error is 2^-63.

Asserted for every internal cell with M != 0, with u = 2^-24 for f32 trees and 2^-53 for f64 trees and n_c the cell's bodies:

  the reference's own accuracy   |mass - M| <= (n_c + 2) u |M|,   |com_a - X_a| <= (n_c + 2) u A_a
      -- a sequential fold of n_c terms in the tree's precision (n_c products, n_c - 1 additions), the division and the
      store.  Every build is held to it.  It is NOT a theorem about the fold: the quotient carries the mass's n_c - 1
      additions as well as the sum's, so the worst case is about 2 n_c u, and a fold that adds light bodies to a heavy one
      comes close to it (the host build reached 1.013 (n_c + 2) u on 7 cells of dust_world with the suns as the FIRST
      records; its worlds therefore keep them last, see there).  Do not read it as guaranteed of every build on every world.
  the device build's scheme      the same with R u for (n_c + 2) u, R = SCHEME_R[dtype], whatever n_c.

The count behind R (kernels_tree.hip: k_tree_delta_totals, k_tree_scan, k_tree_emit).  The terms m, m x_a are exact
double-doubles (the product's error comes from an FMA).  The inclusive prefix sums are double-double; a cell's sum is the
double-double difference of two prefixes, rounded to one double: 1 rounding of 2^-53 for M, 1 for each S_a = sum m x_a.  Then
S_a / M in f64: 1 rounding.  Then the store: none on f64 trees, 1 of 2^-24 on f32 trees.  So

    f64 trees   |com_a - X_a| <= (3 + r) 2^-53 A_a,        |mass - M| <= (1 + r) 2^-53 M
    f32 trees   |com_a - X_a| <= (1 + 2^-27 + r) 2^-24 A_a, |mass - M| <= (1 + 2^-29 + r) 2^-24 M

(|X_a| <= A_a; second-order terms are below 2^-50 of these).  r is what the prefixes leave behind: every double-double
addition errs by at most 3 * 2^-106 of the sum of its operands' sizes, a prefix is combined in at most 40 of them (4 in the
thread, 6 + 3 in each of the two block scans -- shuffles in the wave, the waves before it -- the carry, the tiles' totals
before that), so a difference of two prefixes is
off by at most 2^-99 P_a, P_a = sum m |x_a| over ALL bodies sorted up to the cell's last (P = sum m for the mass) -- not
of the cell.  In units of u that is r = 2^-99 P_a / (u A_a M).  For the worlds of tests/test_tree_moments_gpu.py: suns of
mass 1 with 1e-15 dust on an f32 tree, P / M ~ 1e15, r ~ 3e-8; the 1e-12 dust on an f64 tree, r ~ 0.01 for the mass and for
a cell whose bodies sit at |x_a| ~ 1, and it reaches 1 only for a two-body dust cell within 0.01 of a coordinate plane if
every one of the 40 additions errs fully and alike; the far box (P_a / (A_a M) ~ n / 2 = 2 500), r ~ 4e-11.  (The plain f64
prefix sums this replaces had 2^-53 where the 2^-99 stands: r ~ P_a / (A_a M), thousands of units on f64 trees, and on f32
trees 2^-29 P / M: 2e3 units on the 1e-12 dust, 2e6 on the 1e-15 dust.)  R rounds 3 + r and 1 + r up by one unit:

    SCHEME_R = {f32: 2, f64: 4}

and is not fitted to a run: WORST_OBSERVED records what the MI355X gave, for information.

Cells with M == 0 (all bodies massless) are set aside: their stored mass must be exactly 0, and their centre must be what
the host build -- the reference's fold -- stores for the same cell (`host_tree`), NaN for NaN.  check_moments returns how
many there were, and the caller asserts that number.

This module is plain test infrastructure (numpy and math.fsum, no GPU): tests/test_tree_moments_checker.py runs it on host
builds and on planted faults.
"""
from __future__ import annotations

import math

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
SCHEME_R = {np.dtype(np.float32): 2.0, np.dtype(np.float64): 4.0}

#: worst |error| / bound over every case of tests/test_tree_moments_gpu.py on an MI355X (device build): `reference` against
#: (n_c + 2) u, `scheme` against SCHEME_R u; (mass, centre).  The parent commit's plain f64 prefix sums, same file: see DESIGN 3.4.
WORST_OBSERVED = {
    "f32": dict(reference=(0.249, 0.25), scheme=(0.50, 0.50)),
    "f64": dict(reference=(0.25, 0.439), scheme=(0.25, 0.518)),
}

_SPLIT = 134217729.0   # 2^27 + 1 (Veltkamp)


def _two_prod(a: np.ndarray, b: np.ndarray):
    """p, e with p = fl(a b) and p + e = a b exactly (f64 arrays; no FMA in numpy: Dekker's product)."""
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _exact(terms) -> np.longdouble:
    """The exact sum of the f64 terms, to the precision of np.longdouble."""
    hi = math.fsum(terms)
    lo = math.fsum(list(terms) + [-hi])
    return np.longdouble(hi) + np.longdouble(lo)


def leaves_of(tree):
    """(indices of the leaves, in pre-order; per node the half-open range of its leaves in that list)."""
    skip = np.asarray(tree["skip"], np.int64)
    idx = np.arange(len(skip))
    leaf = np.flatnonzero(skip == idx + 1)
    first = np.searchsorted(leaf, idx, side="left")
    last = np.searchsorted(leaf, skip, side="left")
    return leaf, first, last


def exact_moments(tree) -> dict:
    """For every internal cell: `cell` (node index), `n_c`, `M`, `X` [cells, 3], `A` [cells, 3] (np.longdouble)."""
    cm = np.asarray(tree["com_mass"]).astype(np.float64)
    leaf, first, last = leaves_of(tree)
    skip = np.asarray(tree["skip"], np.int64)
    cells = np.flatnonzero(skip != np.arange(len(skip)) + 1)
    m = cm[leaf, 3]
    prod = [_two_prod(m, cm[leaf, a]) for a in range(3)]
    aprod = [_two_prod(m, np.abs(cm[leaf, a])) for a in range(3)]
    M = np.zeros(len(cells), np.longdouble)
    X = np.zeros((len(cells), 3), np.longdouble)
    A = np.zeros((len(cells), 3), np.longdouble)
    ml = m.tolist()
    pl = [(p.tolist(), e.tolist()) for p, e in prod]
    al = [(p.tolist(), e.tolist()) for p, e in aprod]
    for q, i in enumerate(cells):
        a, b = int(first[i]), int(last[i])
        M[q] = _exact(ml[a:b])
        if M[q] == 0:
            X[q] = A[q] = np.nan
            continue
        for ax in range(3):
            X[q, ax] = _exact(pl[ax][0][a:b] + pl[ax][1][a:b]) / M[q]
            A[q, ax] = _exact(al[ax][0][a:b] + al[ax][1][a:b]) / abs(M[q])
    return dict(cell=cells, n_c=(last - first)[cells], M=M, X=X, A=A)


def moment_ratios(tree, exact=None) -> dict:
    """Per internal cell with M != 0: `mass` = |mass - M| / (u |M|) and `com` [cells, 3] = |com_a - X_a| / (u A_a), in units of
    the tree's own rounding (0 where error and scale are both 0, inf where only the scale is, inf for a non-finite stored
    value); `live` marks those cells, `exact` is exact_moments(tree)."""
    ex = exact if exact is not None else exact_moments(tree)
    cm = np.asarray(tree["com_mass"])
    u = np.longdouble(U[cm.dtype])
    got = cm[ex["cell"]].astype(np.longdouble)
    live = ex["M"] != 0

    def ratio(err, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(scale > 0, err / np.where(scale > 0, u * scale, 1), np.where(err == 0, 0.0, np.inf))
        return np.where(np.isfinite(err), r, np.inf).astype(np.float64)

    mass = ratio(np.abs(got[:, 3] - ex["M"]), np.abs(ex["M"]))
    com = ratio(np.abs(got[:, :3] - ex["X"]), ex["A"])
    return dict(mass=mass, com=com, live=live, exact=ex)


def check_moments(tree, scheme: bool, host_tree=None, what="", exact=None) -> dict:
    """Assert the bounds of the module docstring on every internal cell of `tree`: the reference's (n_c + 2) u always, the
    device scheme's SCHEME_R u as well if `scheme`.  Returns dict(cells, massless, reference=(worst mass ratio, worst centre
    ratio) against (n_c + 2) u, scheme=(the same against SCHEME_R u)); `massless` counts the cells with M == 0, which are
    compared with `host_tree` (required if there are any)."""
    cm = np.asarray(tree["com_mass"])
    r = moment_ratios(tree, exact)
    ex, live = r["exact"], r["live"]
    n_c = ex["n_c"].astype(np.float64)
    out = dict(cells=int(len(n_c)), massless=int(np.count_nonzero(~live)))
    for name, per in (("reference", n_c + 2.0), ("scheme", np.full(len(n_c), SCHEME_R[cm.dtype]))):
        rm = r["mass"][live] / per[live]
        rc = (r["com"][live] / per[live][:, None])
        out[name] = (float(rm.max(initial=0.0)), float(rc.max(initial=0.0)))
        if name == "scheme" and not scheme:
            continue
        bad = np.flatnonzero(~((rm <= 1.0) & (rc <= 1.0).all(axis=1)))
        if len(bad):
            cells = ex["cell"][live][bad]
            bound = "(n_c + 2) u" if name == "reference" else f"{SCHEME_R[cm.dtype]:g} u"
            raise AssertionError(
                f"{what}: {len(bad)} of {int(live.sum())} cells beyond {bound}: worst mass {out[name][0]:.3g}, worst centre {out[name][1]:.3g} "
                f"of the bound; first cells {cells[:6].tolist()} with n_c {ex['n_c'][live][bad][:6].tolist()}, mass ratios {rm[bad][:6].tolist()}, "
                f"centre ratios {rc[bad][:6].max(axis=1).tolist()}")
    if out["massless"]:
        dead = ex["cell"][~live]
        stored = cm[dead]
        assert np.all(stored[:, 3] == 0), f"{what}: massless cells {dead[stored[:, 3] != 0][:6].tolist()} store a mass"
        assert host_tree is not None, f"{what}: {len(dead)} massless cells and no host tree to compare their centres with"
        want = np.asarray(host_tree["com_mass"])[dead]
        assert np.array_equal(stored[:, :3], want[:, :3].astype(cm.dtype), equal_nan=True), \
            f"{what}: massless cells' centres differ from the host build's: {stored[:3, :3].tolist()} against {want[:3, :3].tolist()}"
    return out


def prefix_difference_moments(tree) -> np.ndarray:
    """com_mass of `tree` with every internal cell's moments rebuilt the way the device build formed them before it carried
    double-doubles: an inclusive f64 cumulative sum of {m, m x, m y, m z} over the leaves in pre-order, a cell's sums the
    difference of two of its entries, S_a / M in f64, stored in the tree's precision.  (The planted fault of the checker's
    own tests.)"""
    cm = np.asarray(tree["com_mass"])
    leaf, first, last = leaves_of(tree)
    b = cm[leaf].astype(np.float64)
    terms = np.concatenate([b[:, 3:4], b[:, 3:4] * b[:, :3]], axis=1)
    incl = np.concatenate([np.zeros((1, 4)), np.cumsum(terms, axis=0)])
    out = cm.copy()
    skip = np.asarray(tree["skip"], np.int64)
    cells = np.flatnonzero(skip != np.arange(len(skip)) + 1)
    s = incl[last[cells]] - incl[first[cells]]
    with np.errstate(divide="ignore", invalid="ignore"):
        out[cells, :3] = (s[:, 1:] / s[:, :1]).astype(cm.dtype)
    out[cells, 3] = s[:, 0].astype(cm.dtype)
    return out


def rank_cuts(n: int, ranks: int) -> np.ndarray:
    """First sorted position of every spatial rank, and n: the first ownership bounds are the keys at the sorted positions
    r n / G (nbody_let.cpp: h_bounds), and the leaves of a tree in pre-order are the bodies in that sorted order."""
    return np.array([min(n, r * n // ranks) for r in range(ranks + 1)], np.int64)


def spanning_cells(tree, ranks: int):
    """(nodes, owner) of the internal cells of `tree` whose leaves lie on more than one of `ranks` spatial ranks; a cell belongs
    to the rank of its first leaf."""
    leaf, first, last = leaves_of(tree)
    cuts = rank_cuts(len(leaf), ranks)
    skip = np.asarray(tree["skip"], np.int64)
    cells = np.flatnonzero(skip != np.arange(len(skip)) + 1)
    owner = np.searchsorted(cuts[1:], first[cells], side="right")
    ends = np.searchsorted(cuts[1:], last[cells] - 1, side="right")
    span = ends != owner
    return cells[span], owner[span]


def rank_prefix_moments(tree, ranks: int, residue_ulps: float = 0.0) -> np.ndarray:
    """com_mass of `tree` with the moments of every cell that spans spatial ranks rebuilt the way the spatial-shard build formed
    them while it read the HIGH parts of the prefix sums only (kernels_let.hip: k_let_contrib, k_let_finalize), in its order:
    per rank an inclusive f64 cumulative sum of {m, m x, m y, m z} over that rank's own bodies; the owner's part the difference
    of two of its entries (last body, body before the cell's first); every later rank's part a plain prefix of its sums; the
    parts added up in f64 in rank order; S_a / M in f64; one store to f32.  prefix_difference_moments per rank, in short.
    (The planted fault of tests/test_let_list_checker.py.  np.cumsum is a sequential fold: it drifts by up to one rounding of
    the prefix per body, where the high part of a double-double prefix is the double nearest to the prefix, half an ulp off;
    either way a difference of two entries is off by roundings of the PREFIX, 2^-53 P, whatever is left of the cell.)

    Adding a massless body changes neither kind of prefix, so an own part of massless bodies comes out as exactly 0 here as on
    the device.  `residue_ulps` leaves that many ulps of the owner's prefix in such a part instead, in all four sums: what two
    prefixes that associate differently leave behind when neither is the correctly rounded sum (plain f64 block scans)."""
    cm = np.asarray(tree["com_mass"])
    assert cm.dtype == np.float32
    leaf, first, last = leaves_of(tree)
    cuts = rank_cuts(len(leaf), ranks)
    b = cm[leaf].astype(np.float64)
    terms = np.concatenate([b[:, 3:4], b[:, 3:4] * b[:, :3]], axis=1)
    incl = [np.cumsum(terms[cuts[r]:cuts[r + 1]], axis=0) for r in range(ranks)]
    out = cm.copy()
    cells, owners = spanning_cells(tree, ranks)
    for i, o in zip(cells.tolist(), owners.tolist()):
        a, e = int(first[i]), int(last[i])
        up = incl[o][-1]
        before = incl[o][a - cuts[o] - 1] if a > cuts[o] else np.zeros(4)
        s = up - before
        if residue_ulps and not b[a:cuts[o + 1], 3].any():
            s = s + residue_ulps * np.spacing(np.abs(up))
        for q in range(o + 1, ranks):
            t = min(e, int(cuts[q + 1])) - int(cuts[q])
            if t <= 0:
                break
            s = s + incl[q][t - 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = s[1:] / s[0]
        out[i, :3] = np.where(np.isnan(c), np.float32(np.nan), c.astype(np.float32))   # (one NaN, whatever sign the host's 0 / 0 has)
        out[i, 3] = np.float32(s[0])
    return out


# ---------------------------------------------------------------------------------------------- the test worlds
# Every coordinate and mass is an f32-representable value, also in the f64 records (generated in f32, then widened), so the
# products m x are exact in f64.  `nb` is the package (its Plummer generator and record types); seeds are fixed.
BOX = ((0.0, 0.0, 0.0), 64.0)
FAR_BOX = ((1000.0, -2000.0, 500.0), 64.0)
SIZES = (2, 3, 9, 300, 1025, 5000)
DUST_SIZES = (9, 1025, 5000)          # (one scan tile of the device build holds 1 024 bodies)
DUST_MASSES = {"f32": (1e-9, 1e-12, 1e-15), "f64": (1e-9, 1e-12)}
SUN_B = (3.3, 1.7, -2.1)
SUN_A = (-2.9, -0.4, -1.3)            # the (-,-,-) octant: sorts before almost everything; first=False mirrors it to (+,+,+)


def _records(nb, pos, mass, f64, vel=None):
    out = np.zeros(len(pos), nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    out["position"] = np.asarray(pos, np.float32)
    out["mass"] = np.asarray(mass, np.float32)
    if vel is not None:
        out["velocity"] = np.asarray(vel, np.float32)
    return out


def control_world(nb, n, f64=False):
    """A Plummer sphere with masses x U(0.5, 1.5) (test_device_tree_structure_and_forces' bodies)."""
    ics = nb.plummer(n, seed=40 + n)
    mass = ics["mass"] * np.random.default_rng(n).uniform(0.5, 1.5, n).astype(np.float32)
    return _records(nb, ics["position"], mass, f64, ics["velocity"])


def dust_world(nb, n, dust_mass, first=True, f64=False, suns_lead=False):
    """Two suns of mass 1 and n - 2 bodies of `dust_mass` in a Plummer sphere; `first`: sun A sorts before the dust.  The suns
    are the LAST two records.  The device build sorts by position, so the order of the records means nothing to it; the
    reference folds a cell in record order, and with a sun in front every later addition rounds at the sun's scale, alike
    each time (1 + k 1e-9): its mass and its sum each drift by almost n_c u and the quotient by their sum, past the
    (n_c + 2) u this file holds every build to (seen: 1.013 of it on 7 cells of the f64 host build at n = 1 025).  With
    the suns last the fold adds dust to dust and meets the bound with room, so the bound can be asserted of both builds.
    `suns_lead` makes them the first two records instead: a world for the device build alone."""
    ics = nb.plummer(n, seed=400 + n)
    pos, mass = ics["position"].copy(), np.full(n, np.float32(dust_mass))
    pos[n - 1] = np.asarray(SUN_A, np.float32) * np.float32(1.0 if first else -1.0)
    pos[n - 2] = SUN_B
    mass[n - 2:] = 1.0
    vel = ics["velocity"].copy()
    vel[n - 2:] = 0.0
    if suns_lead:
        pos, mass, vel = pos[::-1], mass[::-1], vel[::-1]
    return _records(nb, pos, mass, f64, vel)


def far_world(nb, n, f64=False):
    """n equal masses in FAR_BOX: a Plummer sphere about its centre, the coordinates rounded to f32 there."""
    ics = nb.plummer(n, seed=4000 + n)
    pos = (ics["position"].astype(np.float64) + np.asarray(FAR_BOX[0])).astype(np.float32)
    assert len(np.unique(pos, axis=0)) == n
    return _records(nb, pos, np.full(n, np.float32(1.0 / n)), f64, ics["velocity"])


MASSLESS_CELLS = 1


def massless_world(nb, n=300, f64=False):
    """A Plummer sphere of n bodies of mass 2^-9 on a grid of pitch 2^-10 (every cell's sums are exact in f32, so the host
    and the device build store the same moments to the bit and their walks decide alike), a guard body at (5.375, 5.125,
    5.125) and eight massless bodies at 5.125 +- 0.0625 along every axis: alone in the level-8 cell (5, 5.25]^3 of BOX, one in
    each of its children, the guard in the cell beside it under the same parent.  MASSLESS_CELLS = 1 cell has M == 0."""
    ics = nb.plummer(n, seed=77)
    pos = np.round(ics["position"].astype(np.float64) * 1024.0) / 1024.0
    assert len(np.unique(pos, axis=0)) == n and not np.any(np.all((pos > 4.5) & (pos <= 5.5), axis=1))
    corners = 5.125 + 0.0625 * (np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)]) * 2 - 1)
    pos = np.concatenate([pos, [[5.375, 5.125, 5.125]], corners])
    mass = np.concatenate([np.full(n + 1, 2.0 ** -9), np.zeros(8)])
    vel = np.concatenate([ics["velocity"], np.zeros((9, 3), np.float32)])
    return _records(nb, pos, mass, f64, vel)


# The worlds that put light and massless cells on a spatial rank's boundary (tests/test_let_list_checker.py on the CPU,
# tests/test_let_walk_list_gpu.py on the ranks): dust_world(nb, n, dust, first=True) on `ranks` ranks -- sun A sorts before
# almost everything, so rank 0 holds a sun and then dust up to its bound, and the spanning cells below the first level or two
# on its last body's path are dust only -- and control_world with massless_boundary applied at boundary r.
LET_DUST_CASES = ((2, 1025), (3, 5000), (8, 1025))          # (ranks, n)
LET_DUST_MASSES = (1e-12, 1e-15)
LET_MASSLESS_CASES = ((2, 300, 1), (3, 300, 2), (2, 1025, 1), (3, 1025, 1))   # (ranks, n, boundary r)


def massless_boundary(ics, tree, ranks, r, own_side_only=False):
    """(bodies, node): `ics` with a massless cell across the boundary between spatial ranks r - 1 and r of a world of `ranks`.
    `tree` is a tree of `ics` (Simulation.tree() or the oracle's: its leaves in pre-order are the bodies in sorted order, bit
    copies of the records).  `node` is the deepest internal node that holds both the leaf before and the leaf at sorted
    position r n / ranks, where the first ownership bound is drawn; every body under it gets mass 0 -- with `own_side_only`
    only those before the boundary, the part of the rank that owns the cell.  Masses move no key, so neither the order nor the
    bound changes: `node` is a cell with a part on each side whose exact M is 0 (or whose owner's part is exactly massless)."""
    leaf, first, last = leaves_of(tree)
    n = len(leaf)
    assert n == len(ics) and 0 < r < ranks
    p = int(rank_cuts(n, ranks)[r])
    assert 0 < p < n
    skip = np.asarray(tree["skip"], np.int64)
    holds = np.flatnonzero((skip != np.arange(len(skip)) + 1) & (first <= p - 1) & (last > p))
    node = int(holds.max())      # the cells that hold both are a chain of ancestors: the deepest comes last in pre-order
    where = {row.tobytes(): k for k, row in enumerate(np.ascontiguousarray(ics["position"], np.float32))}
    assert len(where) == n
    under = np.asarray(tree["com_mass"], np.float32)[leaf[first[node]:(p if own_side_only else last[node])], :3]
    out = ics.copy()
    out["mass"][[where[np.ascontiguousarray(row).tobytes()] for row in under]] = 0
    return out, node


def light_pairs(ics):
    """close_pairs / lattice_pairs of test_bh_device_tree_gpu.py with every other pair at mass 1e-12."""
    ics = ics.copy()
    light = (np.arange(len(ics)) // 2) % 2 == 1
    ics["mass"][light] = np.float32(1e-12)
    return ics


DEEP_N = 500
DEEP_CLUMP = (0, 1, 3, 7, 11, DEEP_N - 1, DEEP_N // 2) + tuple(range(99, 108))
DEEP_LIGHT = (0, 1, 7, DEEP_N - 1, 100, 102, 104, 106)


def deep_world(nb, f64=False):
    """The bodies of test_bodies_that_share_all_21_levels_get_second_keys_on_the_device at n = 500: a Plummer sphere with two
    pairs, a triple and a clump of nine a few 1.2e-7 apart, so their cells lie below level 21 of BOX (3e-5 wide), where the
    device build finds a cell's bodies by walking the group of equal first keys.  DEEP_LIGHT of them have mass 1e-12: one
    pair entirely (a cell of 2e-12 behind everything sorted before it), the others beside bodies of ordinary mass."""
    n = DEEP_N
    ics = nb.plummer(n, seed=3)
    pos = ics["position"].copy()
    rng = np.random.default_rng(n)

    def near(dst, src, k=1):
        pos[dst] = pos[src] + (rng.integers(1, 12, 3) * k).astype(np.float32) * np.float32(1.2e-7)
    near(1, 0)
    near(7, 3); near(11, 3, 2); near(n - 1, n // 2)
    for q in range(8):
        near(100 + q, 99, q + 1)
    mass = ics["mass"].copy()
    mass[list(DEEP_LIGHT)] = np.float32(1e-12)
    assert len(np.unique(pos[list(DEEP_CLUMP)], axis=0)) == len(DEEP_CLUMP)
    return _records(nb, pos, mass, f64, ics["velocity"])
