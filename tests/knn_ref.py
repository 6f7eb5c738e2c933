"""numpy restatement of nbody_knn, nbody_knn_density and nbody_knn_density_center (include/nbody_hip.h, "k nearest neighbours"),
integer for integer and bit for bit: within_ref.triangle_r2's matrix of unsoftened f64 squared distances (r2_ji == r2_ij bit
for bit, the diagonal +inf), every row's entries with r2 < +inf in the order (r2 ascending, then j ascending) -- a stable sort
of the row, the non-finite entries removed --, cut to k and padded with -1 and +inf; Casertano & Hut's density from the row as
the header writes it, one numpy operation per rounding; the centre's four sums through within_ref.center_terms and
diag_ref.tree_sum.  And what the call reports about itself: how many rows the cells answer for a hint, and the hints the GPU
tests use."""
import numpy as np

import cells_ref
import diag_ref
import within_ref
from merge_ref import Mismatch
from within_ref import same_bits  # noqa: F401  (re-exported for the tests)

MAX_K = 32
KS = (1, 6, 32)
VOLUME = np.float64(4.1887902047863905)   # NBODY_KERNEL_TOP_HAT's constant


def lists(rec, k, r2=None):
    """(neighbor [n, k] int32, dist2 [n, k] f64)"""
    n = len(rec)
    r2 = within_ref.triangle_r2(rec) if r2 is None else r2
    with np.errstate(all="ignore"):
        key = np.where(r2 < np.inf, r2, np.inf)   # a NaN or an infinite r2 never enters; the diagonal is +inf
    order = np.argsort(key, axis=1, kind="stable") if n else np.zeros((0, 0), np.int64)   # equal r2: ascending j
    ranked = np.take_along_axis(key, order, axis=1) if n else key
    neighbor = np.full((n, k), -1, np.int32)
    dist2 = np.full((n, k), np.inf, np.float64)
    m = min(k, n)
    if m:
        took = ranked[:, :m] < np.inf
        neighbor[:, :m] = np.where(took, order[:, :m], -1)
        dist2[:, :m] = np.where(took, ranked[:, :m], np.inf)
    return neighbor, dist2


def density(rec, k, neighbor, dist2):
    """(rho [n] f64, rk2 [n] f64) from the rows of lists(rec, k)"""
    n = len(rec)
    m = np.ascontiguousarray(rec["mass"], np.float64)   # exact for f32 records
    complete = neighbor[:, k - 1] >= 0 if n else np.zeros(0, bool)
    with np.errstate(all="ignore"):
        M = np.zeros(n, np.float64)
        for slot in range(k - 1):   # one sequential sum per body, in list order, from +0.0
            M = np.where(complete, M + m[np.where(complete, neighbor[:, slot], 0)], M)
        r2 = dist2[:, k - 1]
        r = np.sqrt(np.where(complete, r2, 1.0))
        rho = np.where(complete, M / (VOLUME * ((r * r) * r)), 0.0)
    return rho, np.where(complete, r2, np.inf)


def density_center(rec, rho):
    """(center [3] f64, rho_sum)"""
    with np.errstate(all="ignore"):
        sums = diag_ref.tree_sum(within_ref.center_terms(rec, rho))
        return sums[1:4] / sums[0], float(sums[0])


def grid_runs(rec, hint):
    """whether a call with this hint under NBODY_SEARCH_CELLS runs the cell search"""
    return bool(len(rec)) and hint > 0.0 and cells_ref.expected_stats(rec, hint)[0] == 1


def stats(rec, k, hint, dist2):
    """(rows answered from the cells, rows answered by the all-pairs pass) on a handle in NBODY_SEARCH_CELLS; dist2: lists(rec, k)'s"""
    n = len(rec)
    if not grid_runs(rec, hint):
        return (0, n)
    R2 = np.float64(hint) * np.float64(hint)   # rounded once
    finished = int((dist2[:, k - 1] < R2).sum())   # at least k bodies with r2 < R2
    return (finished, n - finished)


def split_hint(dist2, k):
    """A hint that leaves both finished and unfinished rows, or None when no hint can: the k-th r2 of the complete rows, v = the
    middle one of their distinct values (not the least), and the largest hint with fl(hint hint) <= v -- the rows at v and beyond
    stay unfinished, the rows below it finish.  None: fewer than two distinct values and no incomplete row beside a complete one."""
    kth = dist2[:, k - 1] if len(dist2) else np.zeros(0)
    values = np.unique(kth[kth < np.inf])
    if len(values) == 0:
        return None   # no complete row: nothing can finish
    if len(values) == 1:
        if (kth < np.inf).all():
            return None   # every row has the same k-th distance: all finish or none does
        v = values[0] * 4.0   # every complete row finishes, the incomplete ones cannot
    else:
        v = values[len(values) // 2]
    hint = np.sqrt(v)
    while hint * hint > v:
        hint = np.nextafter(hint, 0.0)
    return float(hint) if hint > 0.0 else None


# ------------------------------------------------------------------------------------------------ checks
def check_lists(got_neighbor, got_dist2, want_neighbor, want_dist2):
    got_neighbor, got_dist2 = np.asarray(got_neighbor), np.asarray(got_dist2)
    if got_neighbor.dtype != np.int32 or got_neighbor.shape != want_neighbor.shape or not np.array_equal(got_neighbor, want_neighbor):
        bad = np.argwhere(got_neighbor != want_neighbor) if got_neighbor.shape == want_neighbor.shape else []
        raise Mismatch(f"neighbours differ at {[tuple(b) for b in bad[:6]]} ({len(bad)} in all), shapes {got_neighbor.shape} {want_neighbor.shape}")
    if got_dist2.dtype != np.float64 or got_dist2.shape != want_dist2.shape or got_dist2.tobytes() != want_dist2.tobytes():
        raise Mismatch("the squared distances differ in bits")


def check_density(got_rho, got_rk2, want_rho, want_rk2):
    if not same_bits(got_rho, want_rho):
        bad = np.nonzero(np.asarray(got_rho) != np.asarray(want_rho))[0]
        raise Mismatch(f"densities differ in bits at {list(bad[:8])}: {np.asarray(got_rho)[bad[:4]]} against {np.asarray(want_rho)[bad[:4]]}")
    if not same_bits(got_rk2, want_rk2):
        raise Mismatch("the k-th squared distances differ in bits")
