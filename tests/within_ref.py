"""numpy restatement of nbody_neighbors_within, nbody_density and nbody_density_center (include/nbody_hip.h, "neighbours within
a radius"), integer for integer and bit for bit: the upper triangle of the unsoftened squared distances in f64, r2_ij for
i < j computed as merge_ref.dist2_matrix computes it (every product, sum and difference a numpy operation of its own) and
mirrored -- r2_ji == r2_ij bit for bit --, the relation j != i and r2 < radius * radius (strict, a NaN or +inf never
qualifies), the CSR list in ascending index, the densities as one sequential sum per body over its neighbours and itself in
ascending index, and the centre's four sums in diag_ref.tree_sum's order (blocks of 256, the pairwise tree, the blocks added
in ascending order)."""
import numpy as np

import cells_ref  # noqa: F401  (the statistics and the adversarial worlds, re-exported for the tests)
import diag_ref
import fof_ref  # noqa: F401  (the worlds, re-exported for the tests)
from merge_ref import Mismatch, dist2_matrix

TOP_HAT, CUBIC_SPLINE = 0, 1
KERNELS = (TOP_HAT, CUBIC_SPLINE)


def same_bits(a, b):
    """equal bit for bit; a NaN equals any NaN (IEEE 754 leaves the sign and payload of a NaN that an operation produces to the
    implementation: x86 makes inf - inf a negative quiet NaN, the device a positive one)"""
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    b = np.ascontiguousarray(np.asarray(b, np.float64))
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def triangle_r2(rec):
    """[n, n] f64: r2[i, j] for i < j as computed from d = x_j - x_i, r2[j, i] the same bits, the diagonal +inf (j != i)"""
    n = len(rec)
    full = dist2_matrix(rec)
    upper = np.triu(np.ones((n, n), bool), 1)
    r2 = np.where(upper, full, full.T)   # the triangle i < j, mirrored
    r2[np.arange(n), np.arange(n)] = np.inf
    return r2


def relation(rec, radius, r2=None):
    """[n, n] bool: j is a neighbour of i"""
    r2 = triangle_r2(rec) if r2 is None else r2
    R2 = np.float64(radius) * np.float64(radius)   # rounded once
    with np.errstate(all="ignore"):
        return r2 < R2   # (strict; NaN and +inf compare false, the diagonal with them)


def neighbors(rec, radius, adj=None):
    """(offset [n + 1] uint64, neighbor [offset[n]] int32)"""
    adj = relation(rec, radius) if adj is None else adj
    n = len(rec)
    offset = np.zeros(n + 1, np.uint64)
    offset[1:] = np.cumsum(adj.sum(axis=1, dtype=np.uint64))
    i, j = np.nonzero(adj)   # row-major: ascending i, ascending j within it
    return offset, j.astype(np.int32)


def spline_w(u):
    """the M4 spline at u in [0, 2] without its normalisation, every operation rounded on its own"""
    u = np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        inner = (1.0 - 1.5 * (u * u)) + 0.75 * ((u * u) * u)
        t = 2.0 - u
        outer = 0.25 * ((t * t) * t)
        return np.where(u < 1.0, inner, outer)


def norm_of(radius, kernel):
    radius = np.float64(radius)
    if kernel == TOP_HAT:
        return np.float64(4.1887902047863905) * ((radius * radius) * radius)
    hs = radius * np.float64(0.5)
    return np.float64(3.141592653589793) * ((hs * hs) * hs)


def density(rec, radius, kernel, r2=None):
    """(rho [n] f64, count [n] int32)"""
    n = len(rec)
    r2 = triangle_r2(rec) if r2 is None else r2
    adj = relation(rec, radius, r2)
    m = np.ascontiguousarray(rec["mass"], np.float64)   # exact for f32 records
    with np.errstate(all="ignore"):
        if kernel == TOP_HAT:
            term = np.broadcast_to(m[None, :], (n, n)).copy()
        else:
            hs = np.float64(radius) * np.float64(0.5)
            u = np.sqrt(np.where(adj, r2, 0.0)) / hs
            u[np.arange(n), np.arange(n)] = 0.0   # the body's own term: u = 0, no r2
            term = m[None, :] * spline_w(u)
        took = adj.copy()
        took[np.arange(n), np.arange(n)] = True
        s = np.zeros(n, np.float64)
        for j in range(n):   # one sequential sum per body, ascending j, from +0.0
            s = np.where(took[:, j], s + term[:, j], s)
        rho = s / norm_of(radius, kernel)
    return rho, took.sum(axis=1).astype(np.int32)


def center_terms(rec, rho):
    x = np.ascontiguousarray(rec["position"], np.float64)
    t = np.zeros((len(rec), 4))
    with np.errstate(all="ignore"):
        t[:, 0] = rho
        for c in range(3):
            t[:, 1 + c] = rho * x[:, c]   # rounded once
    return t


def density_center(rec, radius, kernel, rho=None):
    """(center [3] f64, rho_sum)"""
    rho = density(rec, radius, kernel)[0] if rho is None else rho
    with np.errstate(all="ignore"):
        sums = diag_ref.tree_sum(center_terms(rec, rho))
        return sums[1:4] / sums[0], float(sums[0])


def rows(rec, who, radius):
    """the lists of the bodies `who` alone, for worlds too large for the matrix: [(neighbours int32 ascending)]"""
    x = np.ascontiguousarray(rec["position"], np.float64)
    R2 = np.float64(radius) * np.float64(radius)
    out = []
    for i in who:
        with np.errstate(all="ignore"):
            # (r2_ij from either side is the same bits: negation is exact)
            d = [x[:, c] - x[i, c] for c in range(3)]
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            near = r2 < R2
        near[i] = False
        out.append(np.nonzero(near)[0].astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ checks
def check_lists(got_offset, got_neighbor, want_offset, want_neighbor):
    got_offset, got_neighbor = np.asarray(got_offset), np.asarray(got_neighbor)
    if got_offset.dtype != np.uint64 or got_offset.shape != want_offset.shape or not np.array_equal(got_offset, want_offset):
        raise Mismatch(f"offsets differ: got {list(got_offset[:8])} ..., want {list(want_offset[:8])} ...")
    if got_neighbor.dtype != np.int32 or got_neighbor.shape != want_neighbor.shape or not np.array_equal(got_neighbor, want_neighbor):
        bad = np.nonzero(got_neighbor != want_neighbor)[0] if got_neighbor.shape == want_neighbor.shape else []
        raise Mismatch(f"neighbours differ at {list(bad[:8])} ({len(bad)} in all)")


def check_density(got_rho, got_count, want_rho, want_count):
    if np.asarray(got_count).dtype != np.int32 or not np.array_equal(got_count, want_count):
        raise Mismatch("the term counts differ")
    if not same_bits(got_rho, want_rho):
        bad = np.nonzero(np.asarray(got_rho) != np.asarray(want_rho))[0]
        raise Mismatch(f"densities differ in bits at {list(bad[:8])}: {np.asarray(got_rho)[bad[:4]]} against {np.asarray(want_rho)[bad[:4]]}")


def check_center(got_center, got_sum, want_center, want_sum):
    if not same_bits(got_center, want_center) or not same_bits(got_sum, want_sum):
        raise Mismatch(f"centre {got_center!r} sum {got_sum!r} against {want_center!r} {want_sum!r}")


# ------------------------------------------------------------------------------------------------ worlds
#: the worlds of tests/test_cells_gpu.py, each with the radii it is looked at with (its linking lengths there)
WORLDS = ["clumpy0", "clumpy1", "clumpy2", "clumpy255", "clumpy256", "clumpy257", "clumpy1000", "chain", "cut_chain", "star", "two_lattices",
          "lattice", "wall_pairs", "side_lattice", "coincident", "clump_and_outliers", "huge", "holed_lattice"]


def world(nb, name, f64):
    """(records, radii)"""
    if name.startswith("clumpy"):
        n = int(name[6:])
        return fof_ref.clumpy(nb, n, seed=n, f64=f64), (fof_ref.CLUMPY_B,)
    if name == "chain":
        return fof_ref.chain(nb, 1025, 0.25, f64)[0], (0.25,)
    if name == "cut_chain":
        return fof_ref.chain(nb, 1025, 0.25, f64, cut=500)[0], (0.25,)
    if name == "star":
        return fof_ref.star(nb, 600, 0.25, f64), (0.25,)
    if name == "two_lattices":
        return fof_ref.two_lattices(nb, 6, 0.25, f64), (0.25,)
    if name == "lattice":
        return fof_ref.lattice(nb, 5, f64), (1.0, 1.001)
    for other, rec, radii in cells_ref.adversarial(nb, f64):
        if other == name:
            return rec, radii
    raise KeyError(name)
