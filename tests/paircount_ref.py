"""numpy restatement of nbody_pair_counts and nbody_pair_counts_at (include/nbody_hip.h, "pair-separation counts"), integer
for integer: the squared edges E2[b] = edges[b] * edges[b] rounded once; for the auto counts the upper triangle i < j of
merge_ref.dist2_matrix (d = x_j - x_i, every product, sum and difference a numpy operation of its own), as
within_ref.triangle_r2 takes it; for the cross form d = point - body written out operation by operation; the bins by the two
comparisons (E2[b] <= r2) & (r2 < E2[b + 1]) on the squares -- never a histogram of unsquared values --, outside[0] the pairs
with r2 < E2[0] and outside[1] everything else, !(r2 < E2[n_bins]): a NaN or +inf separation lands there and in no bin."""
import numpy as np

import cells_ref  # noqa: F401  (the statistics and the adversarial worlds, re-exported for the tests)
import fof_ref
import within_ref
from merge_ref import Mismatch, dist2_matrix

MAX_BINS = 1024


# ------------------------------------------------------------------------------------------------ the edges
def squared_edges(edges):
    edges = np.asarray(edges, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return edges * edges   # each rounded once


def valid_edges(edges):
    """the arguments nbody_pair_counts accepts: 1 <= n_bins <= 1024, every edge finite, edges[0] >= 0, the squares finite and
    strictly ascending"""
    edges = np.asarray(edges, np.float64).reshape(-1)
    n_bins = len(edges) - 1
    if n_bins < 1 or n_bins > MAX_BINS:
        return False
    if not np.isfinite(edges).all() or not edges[0] >= 0.0:
        return False
    e2 = squared_edges(edges)
    return bool(np.isfinite(e2).all() and (e2[:-1] < e2[1:]).all())


def log_edges(lo, hi, n_bins):
    """n_bins + 1 edges from lo to hi in equal steps of the logarithm (any strictly ascending set would do: the calls take the
    doubles as they are)"""
    e = np.float64(lo) * (np.float64(hi) / np.float64(lo)) ** (np.arange(n_bins + 1, dtype=np.float64) / np.float64(n_bins))
    e[0], e[-1] = lo, hi
    return e


# ------------------------------------------------------------------------------------------------ the counts
def bin_r2(r2, edges):
    """(counts [n_bins] uint64, outside [2] uint64) of the separations r2 (any shape)"""
    e2 = squared_edges(edges)
    r2 = np.asarray(r2, np.float64).reshape(-1)
    n_bins = len(e2) - 1
    counts = np.zeros(n_bins, np.uint64)
    with np.errstate(all="ignore"):
        for b in range(n_bins):
            counts[b] = np.count_nonzero((e2[b] <= r2) & (r2 < e2[b + 1]))   # closed below, open above; a NaN matches nothing
        below = np.count_nonzero(r2 < e2[0])
        beyond = np.count_nonzero(~(r2 < e2[n_bins]))
    return counts, np.array([below, beyond], np.uint64)


def auto_r2(rec):
    """[n (n - 1) / 2] f64: r2 of every pair i < j"""
    n = len(rec)
    return dist2_matrix(rec)[np.triu(np.ones((n, n), bool), 1)]


def pair_counts(rec, edges, r2=None):
    assert valid_edges(edges)
    return bin_r2(auto_r2(rec) if r2 is None else r2, edges)


def cross_r2(rec, points):
    """[n, m] f64: r2 of every (body, point) pair, d = point - body"""
    x = np.ascontiguousarray(rec["position"], np.float64)   # exact for f32 records
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dx = np.subtract(p[None, :, 0], x[:, None, 0])
        dy = np.subtract(p[None, :, 1], x[:, None, 1])
        dz = np.subtract(p[None, :, 2], x[:, None, 2])
        xx = np.multiply(dx, dx)
        yy = np.multiply(dy, dy)
        zz = np.multiply(dz, dz)
        return np.add(np.add(xx, yy), zz)


def pair_counts_at(rec, points, edges):
    assert valid_edges(edges)
    return bin_r2(cross_r2(rec, points), edges)


def check(got, want, what=""):
    """the device's (counts, outside) against the restatement's, integer for integer"""
    for name, g, w in (("counts", got[0], want[0]), ("outside", got[1], want[1])):
        g = np.asarray(g)
        if g.dtype != np.uint64 or g.shape != w.shape or not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0] if g.shape == w.shape else []
            raise Mismatch(f"{what}: {name} differ at {list(bad[:8])} ({len(bad)} in all): got {list(g[bad[:4]])}, want {list(w[bad[:4]])}")


# ------------------------------------------------------------------------------------------------ worlds
LATTICE_EDGES = (0.0, 1.0, 2.0, 3.0)


def lattice_edges(nb, f64, side=5):
    """the integer lattice of fof_ref: with the edges 0, 1, 2, 3 many pairs have r2 exactly 1, 4 and 9 -- on a closed lower
    edge (counted in the bin that begins there) and on the open upper one (not counted in the bin that ends there)"""
    return fof_ref.lattice(nb, side, f64)


#: the worlds of the GPU tests: those of tests/test_within_gpu.py, and the lattice above
WORLDS = within_ref.WORLDS + ["lattice_edges"]


def world(nb, name, f64):
    """(records, lengths): the lengths are the world's own (its linking lengths or radii elsewhere)"""
    if name == "lattice_edges":
        return lattice_edges(nb, f64), (1.0, 3.0)
    return within_ref.world(nb, name, f64)


def bin_sets(lengths, diameter):
    """{name: edges} for a world looked at with `lengths`: one bin, 33 and 1 024 log bins about its largest length, a set that
    begins above zero, and one whose last edge exceeds the world's diameter (the grid degenerates to one cell)"""
    top = float(max(lengths))
    sets = {"one": np.array([0.0, top]),
            "log33": log_edges(top * 1e-3, top, 33),
            "log1024": log_edges(top * 1e-4, 2.0 * top, 1024),
            "from_above_zero": np.array([0.5 * top, 0.75 * top, top, 1.5 * top])}
    if np.isfinite(diameter) and diameter > 0.0:
        sets["beyond_the_world"] = np.array([0.0, 0.25 * diameter, 0.5 * diameter, 2.0 * diameter + 1.0])
    return sets


def diameter(rec):
    """an upper bound of the largest finite separation: the diagonal of the bounding box of the bodies with finite coordinates"""
    x = np.ascontiguousarray(rec["position"], np.float64)
    x = x[np.isfinite(x).all(axis=1)]
    if len(x) == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.sqrt(((x.max(axis=0) - x.min(axis=0)) ** 2).sum()))
