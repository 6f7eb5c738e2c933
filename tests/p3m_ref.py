"""nbody_p3m_field restated in numpy (include/nbody_hip.h, "P3M field"; csrc/p3m_pairs.h is the statement).  The mesh part is the
composition of deposit_ref.deposit, the periodic solve of poisson_ref with the split table product D'[i] = D[i] S[i] restated here,
and sample_ref.sample; the short-range part -- chain cells, the walk's order, the minimum-image term and the sequential sums -- is
restated here, every numpy operation rounded on its own.  Also the all-pairs sum, the Ewald sum and the worlds the tests share."""
import math

import numpy as np

import deposit_ref
import poisson_ref
import sample_ref

NGP, CIC, TSC = 0, 1, 2
GRADIENT2, GRADIENT4 = sample_ref.GRADIENT2, sample_ref.GRADIENT4
SPECTRAL, DIFF2 = poisson_ref.SPECTRAL, poisson_ref.DIFF2
BOTH, MESH_ONLY, SHORT_ONLY = 0, 1, 2
INTERVALS = 4096
SQRT_PI = 1.7724538509055159
INDEX_LIMIT = 2147483648.0


# ---- the split factors
def table(r_split, r_cut):
    """[4097][2] = {F, P} at x_k = k h from math.erfc and math.exp, in the header's expression tree"""
    h = (float(r_cut) / float(r_split)) / float(INTERVALS)
    out = np.zeros((INTERVALS + 1, 2))
    for k in range(INTERVALS + 1):
        x = float(k) * h
        e = math.erfc(x / 2.0)
        out[k] = (e + (x / SQRT_PI) * math.exp(-((x * x) / 4.0)), e)
    return out


def exact_F(x):
    return math.erfc(x / 2.0) + (x / math.sqrt(math.pi)) * math.exp(-x * x / 4.0)


def exact_P(x):
    return math.erfc(x / 2.0)


# ---- the mesh part
def split_solve(mass, spacing, g, green, deconvolve, scheme, r_split):
    """poisson_ref.solve's periodic branch with D'[i] = D[i] S[i], S[i] = exp(-(K[i] (r_split r_split))): always multiplied"""
    mass = np.ascontiguousarray(mass, np.float64)
    shape = mass.shape
    spacing, g, r_split = float(spacing), float(g), float(r_split)
    re, im = poisson_ref.transform(mass.copy(), np.zeros(shape))
    c = -((poisson_ref.FOUR_PI * g) / ((spacing * spacing) * spacing))
    K = [poisson_ref.k_table(green, n, spacing) for n in shape]
    den = (K[0][:, None, None] + K[1][None, :, None]) + K[2][None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(den == 0.0, 0.0, c / den)
    rr = r_split * r_split
    D = []
    for a, n in enumerate(shape):
        d = poisson_ref.d_table(deconvolve, scheme, n) if deconvolve else np.ones(n)
        s = np.array([math.exp(-(float(k) * rr)) for k in K[a]], np.float64)
        D.append(d * s)
    f = f * ((D[0][:, None, None] * D[1][None, :, None]) * D[2][None, None, :])
    re, im = poisson_ref.transform(f * re, f * im, inverse=True)
    return re * (1.0 / float(mass.size)) + 0.0


# ---- the short-range part
def chain_shift(spacing, r_cut):
    shift = 0
    while float(1 << shift) * float(spacing) < float(r_cut):
        shift += 1
    return shift


def chain_cells(xyz, m, origin, spacing, dims, shift):
    """(cell [n] int64, -1 where there is none; chain dims)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (xyz - np.asarray(origin, np.float64)) / float(spacing)
        ok = np.isfinite(xyz).all(1) & np.isfinite(m) & (np.abs(u) < INDEX_LIMIT).all(1)
    cd = [int(d) >> shift for d in dims]
    cell = np.full(len(xyz), -1, np.int64)
    i = np.floor(u[ok]).astype(np.int64) % np.asarray(dims, np.int64)
    cc = i >> shift
    cell[ok] = (cc[:, 0] * cd[1] + cc[:, 1]) * cd[2] + cc[:, 2]
    return cell, cd


def neighbours(cell, cd):
    """the 27 chain cells around `cell` in the walk's order"""
    cz, cy, cx = cell % cd[2], (cell // cd[2]) % cd[1], cell // (cd[2] * cd[1])
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                out.append((((cx + dx) % cd[0]) * cd[1] + (cy + dy) % cd[1]) * cd[2] + (cz + dz) % cd[2])
    return out


def _terms(T, L, R2, scale, soften, xt, trow, xp, mp, prow):
    """targets [t] against partners [p] in the partners' order: (w d [t][p][3], the potential's term [t][p], counted [t][p] bool,
    looked [t][p] bool); a term that is not added is +0.0"""
    d = xp[None, :, :] - xt[:, None, :]
    d = d - np.rint(d / L) * L
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    looked = np.ones(r2.shape, bool) if trow is None else (trow[:, None] != prow[None, :])
    counted = looked & (r2 < R2)
    added = counted & ~((r2 == 0.0) & (soften == 0.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.sqrt(r2) * scale
        k = np.minimum(np.where(added, t, 0.0).astype(np.int64), INTERVALS - 1)
        fr = t - k.astype(np.float64)
        Fv = T[k, 0] + fr * (T[k + 1, 0] - T[k, 0])
        Pv = T[k, 1] + fr * (T[k + 1, 1] - T[k, 1])
        inv = 1.0 / np.sqrt(r2 + soften * soften)
        w = (mp[None, :] * ((inv * inv) * inv)) * Fv
        wd = np.where(added[..., None], w[..., None] * d, 0.0)
        ph = np.where(added, (mp[None, :] * inv) * Pv, 0.0)
    return wd, ph, counted, looked


def _sequential(wd, ph):
    """the sums from +0.0 over the partners in their order (an unadded term is a zero, which changes no bit of a sum that began at +0.0)"""
    a = np.zeros((wd.shape[0], 3))
    p = np.zeros(wd.shape[0])
    for j in range(wd.shape[1]):
        a = a + wd[:, j, :]
        p = p + ph[:, j]
    return a, p


def short_range(body_xyz, body_m, origin, spacing, dims, g, r_cut, soften, T, points=None, all_pairs=False):
    """(out [n][4] = {acc_short, phi_short}, partners looked at, terms with r2 < R2[, sum |term| [n][4], terms of each target
    [n]]): the walk over chain cells, or (all_pairs) every body with a chain cell in ascending row -- the same terms, another order"""
    body_xyz = np.asarray(body_xyz, np.float64).reshape(-1, 3)
    body_m = np.asarray(body_m, np.float64).reshape(-1)
    spacing, g, r_cut, soften = float(spacing), float(g), float(r_cut), float(soften)
    shift = chain_shift(spacing, r_cut)
    bcell, cd = chain_cells(body_xyz, body_m, origin, spacing, dims, shift)
    at_bodies = points is None
    P = body_xyz if at_bodies else np.asarray(points, np.float64).reshape(-1, 3)
    tcell = bcell if at_bodies else chain_cells(P, np.zeros(len(P)), origin, spacing, dims, shift)[0]
    L = np.asarray(dims, np.float64) * spacing
    R2, scale = r_cut * r_cut, float(INTERVALS) / r_cut
    out = np.zeros((len(P), 4))
    mag = np.zeros((len(P), 4))
    each = np.zeros(len(P), np.int64)
    looked = counted = 0
    members = {int(c): np.flatnonzero(bcell == c) for c in np.unique(bcell) if c >= 0}   # (ascending row)
    everybody = np.flatnonzero(bcell >= 0)
    for c in np.unique(tcell):
        if c < 0:
            continue
        t = np.flatnonzero(tcell == c)
        if all_pairs:
            p = everybody
        else:
            lists = [members[n] for n in neighbours(int(c), cd) if n in members]
            p = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        wd, ph, cnt, lk = _terms(T, L, R2, scale, soften, P[t], t if at_bodies else None, body_xyz[p], body_m[p], p)
        a, s = _sequential(wd, ph)
        out[t, :3] = g * a
        out[t, 3] = 0.0 - g * s
        mag[t, :3] = abs(g) * np.abs(wd).sum(1)
        mag[t, 3] = abs(g) * np.abs(ph).sum(1)
        each[t] = cnt.sum(1)
        looked += int(lk.sum())
        counted += int(cnt.sum())
    return (out, looked, counted, mag, each) if all_pairs else (out, looked, counted)


def p3m_field(body_xyz, body_m, origin, spacing, dims, g, r_split, r_cut, T, scheme=CIC, gradient=GRADIENT2, green=SPECTRAL, deconvolve=0,
              soften=0.0, terms=BOTH, points=None):
    """(acc [n][3], phi [n], cls [n] uint8, counts [8] uint64, partners looked at, terms with r2 < R2)"""
    body_xyz = np.asarray(body_xyz, np.float64).reshape(-1, 3)
    mass, c_dep = deposit_ref.deposit(body_xyz, body_m, origin, spacing, dims, scheme, True, -1)
    pot = split_solve(mass, spacing, g, green, deconvolve, scheme, r_split)
    p = body_xyz if points is None else np.asarray(points, np.float64).reshape(-1, 3)
    grad, cls, c_smp = sample_ref.sample(p, pot, origin, spacing, scheme, gradient, True, -1)
    acc = 0.0 - grad
    phi = sample_ref.sample(p, pot, origin, spacing, scheme, sample_ref.VALUE, True, -1)[0][:, 0]
    counts = np.concatenate([c_dep, c_smp]).astype(np.uint64)
    looked = counted = 0
    if terms != MESH_ONLY:
        s, looked, counted = short_range(body_xyz, body_m, origin, spacing, dims, g, r_cut, soften, T, points)
        if terms == SHORT_ONLY:
            acc, phi = s[:, :3].copy(), s[:, 3].copy()
        else:
            acc, phi = acc + s[:, :3], phi + s[:, 3]
    return acc, phi, cls, counts, looked, counted


# ---- the Ewald sum of a periodic cube of side `box` (the physics anchor): acc [n][3] with g = 1
def ewald_acc(xyz, m, box, alpha, n_max, k_max):
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    acc = np.zeros((n, 3))
    d0 = xyz[None, :, :] - xyz[:, None, :]   # r_j - r_i
    d0 = d0 - np.rint(d0 / box) * box
    rng = range(-n_max, n_max + 1)
    for ix in rng:
        for iy in rng:
            for iz in rng:
                d = d0 + np.array([ix, iy, iz], np.float64) * box
                r2 = (d * d).sum(-1)
                if ix == 0 and iy == 0 and iz == 0:
                    r2[np.arange(n), np.arange(n)] = np.inf
                r = np.sqrt(r2)
                erfc = np.vectorize(math.erfc)(alpha * r)
                w = erfc / (r2 * r) + (2.0 * alpha / math.sqrt(math.pi)) * np.exp(-alpha * alpha * r2) / r2
                acc += ((m[None, :] * w)[..., None] * d).sum(1)
    ks = np.arange(-k_max, k_max + 1)
    kv = np.stack(np.meshgrid(ks, ks, ks, indexing="ij"), -1).reshape(-1, 3)
    kv = kv[(kv != 0).any(1)].astype(np.float64) * (2.0 * math.pi / box)
    k2 = (kv * kv).sum(1)
    phase = xyz @ kv.T                                    # [n][k]
    sr, si = m @ np.cos(phase), m @ np.sin(phase)         # sum_j m_j cos, sin (k . r_j)
    # sum_j m_j sin(k . (r_i - r_j)) = sin(k r_i) sr - cos(k r_i) si
    s = np.sin(phase) * sr[None, :] - np.cos(phase) * si[None, :]
    coef = (4.0 * math.pi / box ** 3) * np.exp(-k2 / (4.0 * alpha * alpha)) / k2
    acc -= (s * coef[None, :]) @ kv
    return acc


def ewald_world(seed=11):
    """64 bodies in the unit box: 32 uniform, 32 in a clump of a quarter of a cell of the 32^3 grid; unequal masses"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(0.0, 1.0, (32, 3)), np.array([0.37, 0.52, 0.61]) + rng.uniform(-0.5, 0.5, (32, 3)) * (0.25 / 32.0)])
    return xyz, rng.uniform(0.5, 1.5, 64) / 64.0


def rms_relative(acc, want):
    """sqrt(mean_i |acc_i - want_i|^2 / |want_i|^2)"""
    return float(np.sqrt(np.mean(((acc - want) ** 2).sum(1) / (want ** 2).sum(1))))


# ---- the worlds of tests/test_p3m_checker.py and test_p3m_gpu.py
#: name -> (origin, spacing, dims)
GRIDS = {
    "p16": ((-2.0, -2.0, -2.0), 0.25, (16, 16, 16)),
    "p16x32x64": ((-2.0, -4.0, -8.0), 0.25, (16, 32, 64)),
    "p32x16x16": ((-4.0, -2.0, -2.0), 0.25, (32, 16, 16)),
}


def box_of(grid_name):
    origin, spacing, dims = GRIDS[grid_name]
    lo = np.asarray(origin, np.float64)
    return lo, lo + spacing * np.asarray(dims, np.float64)


def uniform_world(grid_name, n, seed=3, outside=False):
    """n bodies uniform in the box with unequal masses; outside: some of them moved whole periods out of it"""
    lo, hi = box_of(grid_name)
    rng = np.random.default_rng(seed + n)
    xyz = rng.uniform(lo, hi, (n, 3))
    if outside:
        xyz[::7] += (hi - lo) * rng.integers(-3, 4, (len(xyz[::7]), 3))
    return xyz, rng.uniform(0.5, 1.5, n) / n


def face_world(grid_name, r_cut, per_face=3, seed=5):
    """bodies inside the box within 1e-3 r_cut of either side of EVERY chain face, plus a sprinkling elsewhere"""
    origin, spacing, dims = GRIDS[grid_name]
    lo, hi = box_of(grid_name)
    rng = np.random.default_rng(seed)
    c = (1 << chain_shift(spacing, r_cut)) * spacing
    rows = []
    for axis in range(3):
        for f in range(int(round((hi[axis] - lo[axis]) / c)) + 1):
            for side in (-1.0, 1.0):
                p = rng.uniform(lo, hi, (per_face, 3))
                p[:, axis] = lo[axis] + f * c + side * rng.uniform(1e-9, 1e-3, per_face) * r_cut
                rows.append(p)
    xyz = np.concatenate(rows + [rng.uniform(lo, hi, (64, 3))])
    xyz = xyz[((xyz >= lo) & (xyz < hi)).all(1)]
    return xyz, rng.uniform(0.5, 1.5, len(xyz)) / len(xyz)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        r = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first {r}: {got[r]!r} vs {want[r]!r}")
