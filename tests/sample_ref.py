"""nbody_grid_sample restated in numpy (include/nbody_hip.h, "grid sample"; csrc/sample_grid.h): every operation is one f64 ufunc,
rounded on its own, the terms are added point by point in the order a, b, c.  It reuses nothing of the library.  Also the worlds
and grids of tests/test_sample_checker.py and test_sample_gpu.py, and a plain Python triple loop (math.floor, floats) the
restatement itself is checked against."""
import math

import numpy as np

NGP, CIC, TSC = 0, 1, 2
VALUE, GRADIENT2, GRADIENT4 = 0, 1, 2
SCHEMES = (NGP, CIC, TSC)
OPS = (VALUE, GRADIENT2, GRADIENT4)
INSIDE, PARTIAL, OUTSIDE, SKIPPED = 0, 1, 2, 3
LIMIT = 2.0 ** 31
REACH = {VALUE: 0, GRADIENT2: 1, GRADIENT4: 2}

#: name -> (origin, spacing, dims, project_axis)
GRIDS = {
    "1x1x1": ((-2.0, -2.0, -2.0), 4.0, (1, 1, 1), -1),
    "2x2x2": ((-2.0, -2.0, -2.0), 2.0, (2, 2, 2), -1),
    "5x7x3": ((-0.625, -0.875, -0.375), 0.25, (5, 7, 3), -1),
    "16^3": ((-2.0, -2.0, -2.0), 0.25, (16, 16, 16), -1),
    "64x64x1_z": ((-2.0, -2.0, 0.0), 0.0625, (64, 64, 1), 2),
    "1x2x3": ((-0.5, -1.0, -1.5), 1.0, (1, 2, 3), -1),    # periodic axes of 1, 2 and 3 cells
    "4x3x4": ((-1.0, -0.75, -1.0), 0.5, (4, 3, 4), -1),   # not periodic: every term of GRADIENT4 is dropped
}
WORLDS = ("n1", "n63", "n64", "n65", "n257", "plummer4099", "one_cell", "holed")


def world(nb, name, f64):
    """The records of a world, in the handle's dtype (an f32 world holds f32 values: the restatement widens them exactly)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "plummer4099":
        return nb.plummer(4099, seed=7, f64=f64)
    if name.startswith("n"):
        return nb.plummer(int(name[1:]), seed=11, f64=f64)
    n = {"one_cell": 4099, "holed": 300}[name]
    rec = nb.plummer(n, seed=13, f64=f64)
    if name == "one_cell":   # cell (9, 9, 9) of the 16^3 grid: [0.25, 0.5)^3
        rec["position"] = rng.uniform(0.30, 0.45, (n, 3))
    elif name == "holed":
        rec["position"][3, 0] = np.nan
        rec["position"][50, 1] = np.inf
        rec["position"][51, 2] = -np.inf
        rec["position"][299] = np.nan
        rec["position"][60] = (1.0e6, -3.0e5, 2.0e4)       # far outside every grid
        rec["position"][61] = (-7.5e8, 0.25, 0.25)
        rec["position"][62] = (2.0 ** 31 * 0.25 - 2.0, 0.1, 0.1)   # 16^3: u = 2^31 exactly on x (skipped there)
        rec["position"][63] = (-(2.0 ** 31) * 0.0625 - 2.0, 0.1, 0.1)   # 64x64x1: u = -2^31 exactly on x
        rec["position"][64] = (2.0 ** 29 - 2.0 - 0.25, 0.1, 0.1)   # 16^3: the last u below 2^31 but one cell
    return rec


def points(rec):
    """xyz [n][3] as f64"""
    return np.ascontiguousarray(rec["position"], np.float64).reshape(-1, 3)


def make_grid(name, fields, seed=0):
    """[fields][nx][ny][nz] f64: the same cells for the same name, fields and seed"""
    dims = GRIDS[name][2]
    rng = np.random.default_rng(1000 * seed + 10 * sum(map(ord, name)) + fields)
    return rng.standard_normal((fields,) + tuple(dims))


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


def sample(xyz, grid, origin, spacing, scheme, op, periodic=False, project_axis=-1):
    """(out [n][fields or 3] f64, cls [n] uint8, counts [4] uint64)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    grid = np.asarray(grid, np.float64)
    if grid.ndim == 3:
        grid = grid[None]
    fields, dims = grid.shape[0], grid.shape[1:]
    n, reach = len(xyz), REACH[op]
    out = np.zeros((n, fields if op == VALUE else 3))
    skipped = ~np.isfinite(xyz).all(1)
    first, weight = [], []
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
    cnt = [weight[c].shape[1] for c in range(3)]
    wrap = [periodic or c == project_axis for c in range(3)]
    on, wide = [], np.ones(n, bool)
    for c in range(3):
        idx = first[c][:, None] + np.arange(cnt[c])[None, :]
        on.append(np.full(n, cnt[c]) if wrap[c] else ((idx >= 0) & (idx < dims[c])).sum(1))
        if not periodic and c != project_axis:   # every read of a gradient: the stencil widened by its reach
            wide &= (first[c] - reach >= 0) & (first[c] + (cnt[c] - 1) + reach < dims[c])
    full = np.all([on[c] == cnt[c] for c in range(3)], 0)
    none = np.any([on[c] == 0 for c in range(3)], 0)
    cls = np.where(skipped, SKIPPED, np.where(none, OUTSIDE, np.where(full & wide, INSIDE, PARTIAL))).astype(np.uint8)
    counts = np.array([(cls == k).sum() for k in range(4)], np.uint64)
    den = (12.0 if op == GRADIENT4 else 2.0) * spacing

    def on_axis(i, c):
        """(indices brought onto axis c, which of them land)"""
        if wrap[c]:
            return np.mod(i, dims[c]), np.ones(n, bool)
        return np.clip(i, 0, dims[c] - 1), (i >= 0) & (i < dims[c])

    with np.errstate(all="ignore"):
        for a in range(cnt[0]):
            for b in range(cnt[1]):
                for c in range(cnt[2]):
                    cell, good = [], ~skipped
                    for axis, k in ((0, a), (1, b), (2, c)):
                        i, ok = on_axis(first[axis] + k, axis)
                        cell.append(i)
                        good = good & ok
                    w = (weight[0][:, a] * weight[1][:, b]) * weight[2][:, c]
                    if op == VALUE:
                        for f in range(fields):
                            t = w * grid[f][cell[0], cell[1], cell[2]]
                            out[good, f] = out[good, f] + t[good]
                        continue
                    for k in range(3):
                        if k == project_axis:
                            continue
                        raw = first[k] + (a, b, c)[k]
                        at, landed = {}, good
                        for off in ((-1, 1) if reach == 1 else (-2, -1, 1, 2)):
                            i, ok = on_axis(raw + off, k)
                            nb = list(cell)
                            nb[k] = i
                            at[off] = grid[0][nb[0], nb[1], nb[2]]
                            landed = landed & ok
                        if reach == 1:
                            d = (at[1] - at[-1]) / den
                        else:
                            d = (8.0 * (at[1] - at[-1]) - (at[2] - at[-2])) / den
                        t = w * d
                        out[landed, k] = out[landed, k] + t[landed]
    return out, cls, counts


def sample_loops(xyz, grid, origin, spacing, scheme, op, periodic=False, project_axis=-1):
    """The same with plain Python floats and ints, one point and one term at a time."""
    grid = np.asarray(grid, np.float64)
    if grid.ndim == 3:
        grid = grid[None]
    fields, dims = grid.shape[0], grid.shape[1:]
    n, reach = len(xyz), REACH[op]
    width = fields if op == VALUE else 3
    out, cls, counts = np.zeros((n, width)), np.zeros(n, np.uint8), [0, 0, 0, 0]
    den = (12.0 if op == GRADIENT4 else 2.0) * spacing

    def land(i, c):
        if periodic or c == project_axis:
            return i % dims[c]
        return i if 0 <= i < dims[c] else None

    def mul(w, v):   # IEEE: 0 * inf is NaN (Python floats do that too)
        return w * v

    for p in range(n):
        st, skip = [], not all(math.isfinite(float(v)) for v in xyz[p])
        for c in range(3):
            if skip:
                break
            if c == project_axis:
                st.append([(0, 1.0)])
                continue
            u = (float(xyz[p][c]) - origin[c]) / spacing
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
            cls[p] = SKIPPED
            counts[SKIPPED] += 1
            continue
        on = [sum(1 for j, _ in st[c] if land(j, c) is not None) for c in range(3)]
        every = all(land(j + o, c) is not None for c in range(3) if c != project_axis for j, _ in st[c] for o in range(-reach, reach + 1))
        kind = OUTSIDE if 0 in on else INSIDE if all(on[c] == len(st[c]) for c in range(3)) and every else PARTIAL
        cls[p] = kind
        counts[kind] += 1
        acc = [0.0] * width
        for ix, wx in st[0]:
            for iy, wy in st[1]:
                for iz, wz in st[2]:
                    cell = [land(ix, 0), land(iy, 1), land(iz, 2)]
                    if None in cell:
                        continue
                    w = (wx * wy) * wz
                    if op == VALUE:
                        for f in range(fields):
                            acc[f] = acc[f] + mul(w, float(grid[f][tuple(cell)]))
                        continue
                    raw = (ix, iy, iz)
                    for k in range(3):
                        if k == project_axis:
                            continue
                        at = {}
                        for off in ((-1, 1) if reach == 1 else (-2, -1, 1, 2)):
                            i = land(raw[k] + off, k)
                            if i is None:
                                at = None
                                break
                            nb = list(cell)
                            nb[k] = i
                            at[off] = float(grid[0][tuple(nb)])
                        if at is None:
                            continue
                        d = (at[1] - at[-1]) / den if reach == 1 else (8.0 * (at[1] - at[-1]) - (at[2] - at[-2])) / den
                        acc[k] = acc[k] + mul(w, d)
        out[p] = acc
    return out, cls, np.array(counts, np.uint64)


def same_bits(got, want, what):
    """out, cls and counts equal byte for byte (+0.0 and -0.0 differ, a NaN equals the same NaN)"""
    assert got[0].shape == want[0].shape, f"{what}: shape {got[0].shape} vs {want[0].shape}"
    if got[0].tobytes() != want[0].tobytes():
        bad = np.argwhere(np.ascontiguousarray(got[0]).view(np.uint64) != np.ascontiguousarray(want[0]).view(np.uint64))
        r = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} outputs differ, first {r}: {got[0][r]!r} vs {want[0][r]!r}")
    assert np.array_equal(np.asarray(got[1], np.uint8), np.asarray(want[1], np.uint8)), f"{what}: classes differ at {np.flatnonzero(np.asarray(got[1]) != np.asarray(want[1]))[:8]}"
    assert [int(v) for v in got[2]] == [int(v) for v in want[2]], f"{what}: counts {got[2]} vs {want[2]}"
