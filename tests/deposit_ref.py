"""nbody_deposit restated in numpy (include/nbody_hip.h, "grid deposit"; csrc/deposit_grid.h): every operation is one f64 ufunc,
rounded on its own, the terms become integers with np.rint(np.ldexp(t, S)) and are added into an int64 array with np.add.at,
the grid is np.ldexp(acc as f64, -S).  Also the worlds and grids of tests/test_deposit_checker.py and test_deposit_gpu.py, and a
plain Python triple loop (math.floor, math.ldexp, round) the restatement itself is checked against."""
import math

import numpy as np

NGP, CIC, TSC = 0, 1, 2
MASS, MOMENTUM_X, MOMENTUM_Y, MOMENTUM_Z, MV2, NUMBER = 0, 1, 2, 3, 4, 5
SCHEMES = (NGP, CIC, TSC)
QUANTITIES = (MASS, MOMENTUM_X, MOMENTUM_Y, MOMENTUM_Z, MV2, NUMBER)
LIMIT = 2.0 ** 31

#: name -> (origin, spacing, dims, project_axis)
GRIDS = {
    "16^3": ((-2.0, -2.0, -2.0), 0.25, (16, 16, 16), -1),
    "5x3x2": ((-0.625, -0.375, -0.25), 0.25, (5, 3, 2), -1),
    "1x1x1": ((-2.0, -2.0, -2.0), 4.0, (1, 1, 1), -1),
    "32x32x1_z": ((-2.0, -2.0, 0.0), 0.125, (32, 32, 1), 2),
    "1x8x8_x": ((0.0, -2.0, -2.0), 0.5, (1, 8, 8), 0),
}
WORLDS = ("plummer4099", "one_cell", "lattice", "far_periodic", "holed", "n0", "n1", "n2", "n257")
PERIOD = 4.0   # of the 16^3 grid: far_periodic's bodies stand up to 3 000 periods away on either side


def world(nb, name, f64):
    """The records of a world, in the handle's dtype (an f32 world holds f32 values: the restatement widens them exactly)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "plummer4099":   # unequal masses: a sum of equal terms would not depend on its order even in plain f64
        rec = nb.plummer(4099, seed=7, f64=f64)
        rec["mass"] = rec["mass"] * rng.uniform(0.5, 1.5, len(rec))
        return rec
    if name.startswith("n"):
        return nb.plummer(int(name[1:]), seed=11, f64=f64)
    n = {"one_cell": 4099, "lattice": 600, "far_periodic": 500, "holed": 300}[name]
    rec = nb.plummer(n, seed=13, f64=f64)
    if name == "one_cell":   # cell (9, 9, 9) of the 16^3 grid: [0.25, 0.5)^3
        rec["position"] = rng.uniform(0.30, 0.45, (n, 3))
        rec["mass"] = rng.uniform(0.5, 1.5, n) / n
    elif name == "lattice":   # multiples of half a spacing of the 16^3 grid, some of them off it
        rec["position"] = rng.integers(-18, 19, (n, 3)) * 0.125
    elif name == "far_periodic":
        rec["position"] = rng.uniform(-2.0, 2.0, (n, 3)) + PERIOD * rng.integers(-3000, 3001, (n, 3))
    elif name == "holed":
        rec["position"][3, 0] = np.nan
        rec["position"][50, 1] = np.inf
        rec["position"][51, 2] = -np.inf
        rec["position"][299] = np.nan
        rec["velocity"][7, 1] = np.nan   # skipped under MOMENTUM_Y and MV2 only
        rec["velocity"][8, 0] = np.inf   # skipped under MOMENTUM_X and MV2 only
    return rec


def bodies(rec):
    """(xyz [n][3], vel [n][3], mass [n]) as f64"""
    return (np.ascontiguousarray(rec["position"], np.float64).reshape(-1, 3), np.ascontiguousarray(rec["velocity"], np.float64).reshape(-1, 3),
            np.ascontiguousarray(rec["mass"], np.float64).reshape(-1))


def quantity(rec, which):
    xyz, v, m = bodies(rec)
    with np.errstate(all="ignore"):
        if which == MASS:
            return m.copy()
        if which in (MOMENTUM_X, MOMENTUM_Y, MOMENTUM_Z):
            return m * v[:, which - 1]
        if which == MV2:
            return m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return np.ones(len(m))


def _axis(u, scheme):
    """(first [n] int64, weights [n][cnt]) of one axis"""
    if scheme == NGP:
        return np.floor(u).astype(np.int64), np.ones((len(u), 1))
    if scheme == CIC:
        s = u - 0.5
        i0 = np.floor(s)
        f = s - i0
        return i0.astype(np.int64), np.stack([1.0 - f, f], 1)
    i = np.floor(u)
    d = (u - i) - 0.5
    a, b = 0.5 - d, 0.5 + d
    return i.astype(np.int64) - 1, np.stack([0.5 * (a * a), 0.75 - d * d, 0.5 * (b * b)], 1)


def scale(n, qmax):
    return 61 - int(np.frexp(float(qmax))[1]) - (0 if n <= 1 else (n - 1).bit_length())


def deposit(xyz, q, origin, spacing, dims, scheme, periodic=False, project_axis=-1, order=None, parts=False):
    """(grid [dims] f64, counts [4] uint64); parts: (grid, counts, acc int64 [dims], S, skipped mask, per-body class).  order: a
    permutation the bodies are visited in (it cannot show)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1)
    n = len(q)
    dims = tuple(int(d) for d in dims)
    acc = np.zeros(dims, np.int64)
    skipped = ~(np.isfinite(xyz).all(1) & np.isfinite(q))
    first, weight, count_on = [], [], []
    with np.errstate(all="ignore"):
        for c in range(3):
            if c == project_axis:
                first.append(np.zeros(n, np.int64))
                weight.append(np.ones((n, 1)))
                continue
            u = (xyz[:, c] - origin[c]) / spacing
            skipped |= ~(np.abs(u) < LIMIT)
            f, w = _axis(np.where(np.abs(u) < LIMIT, u, 0.0), scheme)
            first.append(f)
            weight.append(w)
    ok = ~skipped
    for c in range(3):
        idx = first[c][:, None] + np.arange(weight[c].shape[1])[None, :]
        on = np.ones(idx.shape, bool) if (periodic or c == project_axis) else (idx >= 0) & (idx < dims[c])
        count_on.append(on.sum(1))
    full = np.all([count_on[c] == weight[c].shape[1] for c in range(3)], 0)
    none = np.any([count_on[c] == 0 for c in range(3)], 0)
    cls = np.where(skipped, 3, np.where(none, 2, np.where(full, 0, 1)))
    counts = np.array([(cls == k).sum() for k in range(4)], np.uint64)
    qmax = float(np.abs(q[ok]).max()) if ok.any() else 0.0
    S = scale(n, qmax)
    visit = np.arange(n) if order is None else np.asarray(order)
    visit = visit[ok[visit]]
    for a in range(weight[0].shape[1]):
        for b in range(weight[1].shape[1]):
            for c in range(weight[2].shape[1]):
                cell, good = [], np.ones(len(visit), bool)
                for axis, k in ((0, a), (1, b), (2, c)):
                    i = first[axis][visit] + k
                    if periodic or axis == project_axis:
                        i = np.mod(i, dims[axis])
                    else:
                        good &= (i >= 0) & (i < dims[axis])
                    cell.append(i)
                t = q[visit] * ((weight[0][visit, a] * weight[1][visit, b]) * weight[2][visit, c])
                k64 = np.rint(np.ldexp(t, S)).astype(np.int64)
                np.add.at(acc, (cell[0][good], cell[1][good], cell[2][good]), k64[good])
    grid = np.ldexp(acc.astype(np.float64), -S) if n else np.zeros(dims)
    return (grid, counts, acc, S, skipped, cls) if parts else (grid, counts)


def deposit_loops(xyz, q, origin, spacing, dims, scheme, periodic=False, project_axis=-1):
    """The same with plain Python floats and ints, one body and one term at a time: (grid, counts)."""
    n = len(q)
    acc = np.zeros(dims, object)
    acc[...] = 0
    stencils, counts, qmax = [], [0, 0, 0, 0], 0.0
    for i in range(n):
        st, skip = [], not (all(math.isfinite(float(v)) for v in xyz[i]) and math.isfinite(float(q[i])))
        for c in range(3):
            if skip:
                break
            if c == project_axis:
                st.append([(0, 1.0)])
                continue
            u = (float(xyz[i][c]) - origin[c]) / spacing
            if not abs(u) < LIMIT:
                skip = True
            elif scheme == NGP:
                st.append([(math.floor(u), 1.0)])
            elif scheme == CIC:
                s = u - 0.5
                i0 = math.floor(s)
                f = s - i0
                st.append([(i0, 1.0 - f), (i0 + 1, f)])
            else:
                j = math.floor(u)
                d = (u - j) - 0.5
                a, b = 0.5 - d, 0.5 + d
                st.append([(j - 1, 0.5 * (a * a)), (j, 0.75 - d * d), (j + 1, 0.5 * (b * b))])
        if skip:
            counts[3] += 1
            stencils.append(None)
            continue
        on = [sum(1 for j, _ in st[c] if periodic or c == project_axis or 0 <= j < dims[c]) for c in range(3)]
        counts[2 if 0 in on else 0 if all(on[c] == len(st[c]) for c in range(3)) else 1] += 1
        qmax = max(qmax, abs(float(q[i])))
        stencils.append(st)
    S = 61 - math.frexp(qmax)[1] - (0 if n <= 1 else (n - 1).bit_length())
    for i, st in enumerate(stencils):
        if st is None:
            continue
        for ix, wx in st[0]:
            for iy, wy in st[1]:
                for iz, wz in st[2]:
                    cell = [ix, iy, iz]
                    if periodic:
                        cell = [cell[c] % dims[c] for c in range(3)]
                    if all(0 <= cell[c] < dims[c] for c in range(3)):
                        acc[tuple(cell)] += round(math.ldexp(float(q[i]) * ((wx * wy) * wz), S))   # (round: ties to even)
    grid = np.zeros(dims)
    for cell in np.ndindex(*dims):
        grid[cell] = math.ldexp(float(acc[cell]), -S) if n else 0.0
    return grid, np.array(counts, np.uint64)


def same_bits(got, want, what):
    """grid and counts equal byte for byte (+0.0 and -0.0 differ; NaN never arises)"""
    assert got[0].shape == want[0].shape, f"{what}: shape {got[0].shape} vs {want[0].shape}"
    if got[0].tobytes() != want[0].tobytes():
        bad = np.argwhere(got[0].view(np.uint64) != want[0].view(np.uint64))
        c = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} cells differ, first {c}: {got[0][c]!r} vs {want[0][c]!r}")
    assert [int(v) for v in got[1]] == [int(v) for v in want[1]], f"{what}: counts {got[1]} vs {want[1]}"
