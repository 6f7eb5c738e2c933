"""numpy restatement of the uniform cell grid of NBODY_SEARCH_CELLS (include/nbody_hip.h, "pair search"; csrc/cell_grid.h), bit
for bit: which bodies are gridded, lo, side, usable, every body's key, the occupied cells and the candidate pairs -- the
unordered pairs of gridded bodies whose cell indices differ by at most 1 on every axis -- counted by grouping the keys and
summing over adjacent cells (O(27 n)), and for small n by the plain |dk| <= 1 matrix.  And the adversarial worlds that
tests/test_cells_checker.py and tests/test_cells_gpu.py share."""
import numpy as np

import fof_ref

MARGIN = 2.0 ** -20
CELL_BITS = 21
CELL_MAX = 2 ** CELL_BITS - 1
NO_KEY = np.uint64(2 ** 64 - 1)


def positions(rec):
    return np.ascontiguousarray(rec["position"], np.float64)   # exact for f32 records


def grid(x, length):
    """dict(lo [3], side, usable, keys [n] uint64, gridded [n] bool) for points x [n, 3] f64"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    length = np.float64(length)
    ok = np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        if ok.any():
            lo_raw, hi = x[ok].min(axis=0), x[ok].max(axis=0)
            lo = lo_raw + 0.0   # (a zero bound counts as +0.0)
            extent = np.float64((hi - lo_raw).max())
        else:
            lo, extent = np.zeros(3), np.float64(0.0)
        by_length, by_extent = length * np.float64(1.0 + MARGIN), extent * np.float64(MARGIN)
        side = by_length if by_length > by_extent else by_extent
        usable = bool(np.isfinite(extent) and np.isfinite(side) and np.isfinite(length * length))
        keys = np.full(len(x), NO_KEY, np.uint64)
        if usable and ok.any():
            q = np.floor((x[ok] - lo) / side)   # one subtraction, one division, each rounded once
            k = np.minimum(q, float(CELL_MAX)).astype(np.uint64)
            keys[ok] = (k[:, 0] << np.uint64(2 * CELL_BITS)) | (k[:, 1] << np.uint64(CELL_BITS)) | k[:, 2]
    return dict(lo=lo, side=float(side), usable=usable, keys=keys, gridded=ok)


def unpack(keys):
    """[m, 3] int64 cell indices of keys that are not NO_KEY"""
    k = np.asarray(keys, np.uint64)
    return np.stack([(k >> np.uint64(2 * CELL_BITS)), (k >> np.uint64(CELL_BITS)) & np.uint64(CELL_MAX), k & np.uint64(CELL_MAX)],
                    axis=1).astype(np.int64)


def occupied(keys):
    return len(np.unique(keys[keys != NO_KEY]))


def candidates(keys):
    """candidate pairs: c (c - 1) / 2 inside each occupied cell, and c * c' for each of its 13 neighbours that come later"""
    uniq, counts = np.unique(keys[keys != NO_KEY], return_counts=True)
    if not len(uniq):
        return 0
    counts = counts.astype(object)   # Python integers: no overflow
    total = int(sum(c * (c - 1) // 2 for c in counts))
    cell = unpack(uniq)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) <= (0, 0, 0):
                    continue
                nb = cell + np.array([dx, dy, dz])
                inside = ((nb >= 0) & (nb <= CELL_MAX)).all(axis=1)
                nk = (nb[:, 0].astype(np.uint64) << np.uint64(2 * CELL_BITS)) | (nb[:, 1].astype(np.uint64) << np.uint64(CELL_BITS)) | \
                    nb[:, 2].astype(np.uint64)
                at = np.searchsorted(uniq, nk)
                hit = inside & (at < len(uniq))
                hit[hit] &= uniq[at[hit]] == nk[hit]
                total += int(sum(counts[hit] * counts[at[hit]]))
    return total


def candidate_matrix(keys):
    """[n, n] bool: both gridded and |dk| <= 1 on every axis (the diagonal cleared)"""
    keys = np.asarray(keys, np.uint64)
    ok = keys != NO_KEY
    k = unpack(np.where(ok, keys, np.uint64(0)))
    near = (np.abs(k[:, None, :] - k[None, :, :]) <= 1).all(axis=2) & ok[:, None] & ok[None, :]
    near[np.arange(len(keys)), np.arange(len(keys))] = False
    return near


def expected_stats(rec_or_x, length):
    """what nbody_pair_search_stats reports after a call under NBODY_SEARCH_CELLS"""
    x = positions(rec_or_x) if getattr(rec_or_x, "dtype", None) is not None and rec_or_x.dtype.names else np.asarray(rec_or_x, np.float64)
    g = grid(x, length)
    if not g["usable"] or not g["gridded"].any():
        return (0, 0, 0, 0)   # the fallback rule
    return (1, int(g["gridded"].sum()), occupied(g["keys"]), candidates(g["keys"]))


# ------------------------------------------------------------------------------------------------ adversarial worlds
WALL_B = 0.3


def wall_pairs(nb, f64, b=WALL_B):
    """pairs at separations nextafter(b, 0) and b (1 - 2^-50) laid across cell walls on each axis: body 0 at the origin fixes
    lo = 0, so the walls stand at multiples of side = b (1 + 2^-20); each pair straddles the wall at 3 side"""
    side = np.float64(b) * np.float64(1.0 + MARGIN)
    x = [np.zeros(3)]
    for axis in range(3):
        for m, sep in enumerate((np.nextafter(np.float64(b), 0.0), np.float64(b) * (1.0 - 2.0 ** -50))):
            for frac in (0.25, 0.5, 1.0 - 2.0 ** -30):
                base = np.full(3, 7.0 * side)
                base[(axis + 1) % 3] += (8.0 * len(x)) * side   # every pair far from the others
                a = base.copy()
                a[axis] = 3.0 * side - frac * sep
                c = a.copy()
                c[axis] = a[axis] + sep
                x += [a, c]
    return fof_ref._records(nb, np.array(x), f64, 23)


def side_lattice(nb, f64, b=WALL_B, n_side=4):
    """a lattice whose spacing equals the cell side for the length b: every body on a wall"""
    side = np.float64(b) * np.float64(1.0 + MARGIN)
    g = np.arange(n_side, dtype=np.float64) * side
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return fof_ref._records(nb, x, f64, 29)


def coincident(nb, f64, n=70):
    """all bodies at one point: E = 0, one cell"""
    return fof_ref._records(nb, np.tile(np.array([[1.5, -2.25, 0.75]]), (n, 1)), f64, 31)


CLUMP_B = 1e-9


def clump_and_outliers(nb, f64, n=300):
    """a tight clump about (1, 1, 1) of width 4 b for b = 1e-9, and two outliers 1e3 apart: the side comes from E * 2^-20"""
    rng = np.random.default_rng(37)
    x = 1.0 + 4.0 * CLUMP_B * rng.uniform(0.0, 1.0, (n, 3))
    x[5] = 0.0
    x[n - 3] = 1e3
    return fof_ref._records(nb, x, f64, 41)


def huge(nb, f64):
    """coordinates of +-1e308: hi - lo overflows, usable == 0 (f32 records hold them as infinities: those bodies are not gridded)"""
    rng = np.random.default_rng(43)
    x = rng.uniform(-1.0, 1.0, (60, 3))
    x[1::2] = x[0::2] + 0.01   # close pairs
    x[7] = (1e308, 0.0, 0.0)
    x[20] = (-1e308, 1.0, 0.0)
    with np.errstate(over="ignore"):
        return fof_ref._records(nb, x, f64, 47)


def holed_lattice(nb, f64):
    """the integer lattice of the FoF tests with a NaN body and an infinite one"""
    rec = fof_ref.lattice(nb, 5, f64)
    rec["position"][7, 2] = np.nan
    rec["position"][9, 0] = np.inf
    return rec


def adversarial(nb, f64):
    """[(name, records, lengths)]"""
    return [("wall_pairs", wall_pairs(nb, f64), (WALL_B, 0.5 * WALL_B, 3.0 * WALL_B)),
            ("side_lattice", side_lattice(nb, f64), (WALL_B, WALL_B * (1.0 + 2.0 ** -19), 2.0 * WALL_B)),
            ("coincident", coincident(nb, f64), (1e-3, 1.0)),
            ("clump_and_outliers", clump_and_outliers(nb, f64), (CLUMP_B, 2.5 * CLUMP_B)),
            ("huge", huge(nb, f64), (0.05, 1.0)),
            ("holed_lattice", holed_lattice(nb, f64), (1.0, 1.001, 1.5))]
