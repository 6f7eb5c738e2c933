"""nbody_grid_poisson restated in numpy (csrc/poisson_grid.h is the statement): the radix-2 stages vectorised over the lines,
every numpy operation rounded on its own, real and imaginary parts in arrays of their own (no complex arithmetic of numpy's),
the twiddles and the per-axis tables from math.cos and math.sin.  Also the test inputs and the exact oracles the tests share."""
import math

import numpy as np

SPECTRAL, DIFF2 = 0, 1
NGP, CIC, TSC = 0, 1, 2
PI = math.pi
TWO_PI = 2.0 * math.pi
FOUR_PI = 4.0 * math.pi

PERIODIC_SHAPES = ((1, 1, 64), (64, 1, 1), (16, 8, 4), (2, 2, 2))
ISOLATED_SHAPES = ((8, 4, 2), (16, 16, 1), (1, 1, 32))
SOFTENS = (0.0, 0.05)


def twiddles(L):
    """[L / 2][2]: (cos(a), -sin(a)), a = (2 pi k) / L, with the entries at k = 0 and k = L / 4 written as constants"""
    t = np.array([[math.cos((TWO_PI * float(k)) / float(L)), -math.sin((TWO_PI * float(k)) / float(L))] for k in range(L // 2)], np.float64)
    t[0] = (1.0, 0.0)
    if L >= 4:
        t[L // 4] = (0.0, -1.0)
    return t


def _reverse(L):
    p = L.bit_length() - 1
    return np.array([int(format(i, f"0{p}b")[::-1], 2) if p else 0 for i in range(L)], np.int64)


def _axis(re, im, axis, inverse):
    """the lines along `axis` of the arrays (re, im), transformed; new arrays"""
    L = re.shape[axis]
    if L == 1:
        return re, im
    T = twiddles(L)
    wre, wim = T[:, 0], (-T[:, 1] if inverse else T[:, 1])
    re, im = np.moveaxis(re, axis, -1), np.moveaxis(im, axis, -1)
    shape = re.shape
    rev = _reverse(L)
    xr, xi = np.empty(shape), np.empty(shape)
    xr[..., rev], xi[..., rev] = re, im           # x[rev(i)] <- x[i]
    xr, xi = xr.reshape(-1, L), xi.reshape(-1, L)
    h = 1
    while h < L:
        step = L // (2 * h)
        cr, ci = wre[::step][:h], wim[::step][:h]     # w = T[j (L / (2 h))], j < h
        vr, vi = xr.reshape(-1, L // (2 * h), 2, h), xi.reshape(-1, L // (2 * h), 2, h)
        ar, ai, br, bi = vr[:, :, 0, :], vi[:, :, 0, :], vr[:, :, 1, :], vi[:, :, 1, :]
        tr = cr * br - ci * bi
        ti = cr * bi + ci * br
        nr, ni = np.empty_like(vr), np.empty_like(vi)
        nr[:, :, 0, :], ni[:, :, 0, :] = ar + tr, ai + ti
        nr[:, :, 1, :], ni[:, :, 1, :] = ar - tr, ai - ti
        xr, xi = nr.reshape(-1, L), ni.reshape(-1, L)
        h *= 2
    return np.moveaxis(xr.reshape(shape), -1, axis), np.moveaxis(xi.reshape(shape), -1, axis)


def transform(re, im, inverse=False):
    """z, then y, then x; not scaled"""
    for axis in (2, 1, 0):
        re, im = _axis(re, im, axis, inverse)
    return np.ascontiguousarray(re), np.ascontiguousarray(im)


def _mode(i, n):
    return i if i <= n // 2 else i - n


def k_table(green, n, spacing):
    if n == 1:
        return np.zeros(1)
    if green == SPECTRAL:
        k = [(TWO_PI * float(_mode(i, n))) / (float(n) * spacing) for i in range(n)]
        return np.array([v * v for v in k], np.float64)
    v = [(2.0 * math.sin((PI * float(i)) / float(n))) / spacing for i in range(n)]
    return np.array([x * x for x in v], np.float64)


def d_table(deconvolve, scheme, n):
    out = np.ones(n)
    for i in range(1, n):
        a = (PI * float(_mode(i, n))) / float(n)
        s = math.sin(a) / a
        w = s
        for _ in range(deconvolve * (scheme + 1) - 1):
            w = w * s
        out[i] = 1.0 / w
    return out


def green_factor(shape, spacing, g, green, deconvolve, scheme):
    """f [nx][ny][nz] of the periodic multiply"""
    spacing, g = float(spacing), float(g)
    c = -((FOUR_PI * g) / ((spacing * spacing) * spacing))
    K = [k_table(green, n, spacing) for n in shape]
    den = (K[0][:, None, None] + K[1][None, :, None]) + K[2][None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(den == 0.0, 0.0, c / den)
    if deconvolve:
        D = [d_table(deconvolve, scheme, n) for n in shape]
        f = f * ((D[0][:, None, None] * D[1][None, :, None]) * D[2][None, None, :])
    return f


def kernel_grid(shape, spacing, soften):
    """Kr on the padded grid"""
    spacing, soften = float(spacing), float(soften)
    d = []
    for n in shape:
        P = 1 if n == 1 else 2 * n
        m = np.array([0 if n == 1 else (i if i <= n else 2 * n - i) for i in range(P)], np.float64)
        d.append(spacing * m)
    dx, dy, dz = d[0][:, None, None], d[1][None, :, None], d[2][None, None, :]
    r2 = ((dx * dx + dy * dy) + dz * dz) + soften * soften
    with np.errstate(divide="ignore"):
        kr = 1.0 / np.sqrt(r2)
    kr[0, 0, 0] = 1.0 / soften if soften > 0.0 else 0.0
    return kr


def solve(mass, spacing, g, periodic=False, green=SPECTRAL, soften=0.0, deconvolve=0, scheme=CIC):
    """phi [nx][ny][nz]: the restatement of nbody_host_grid_poisson"""
    mass = np.ascontiguousarray(mass, np.float64)
    shape = mass.shape
    g = float(g)
    if periodic:
        re, im = transform(mass.copy(), np.zeros(shape))
        f = green_factor(shape, spacing, g, green, deconvolve, scheme)
        re, im = transform(f * re, f * im, inverse=True)
        return re * (1.0 / float(mass.size)) + 0.0
    padded = tuple(1 if n == 1 else 2 * n for n in shape)
    big = np.zeros(padded)
    big[: shape[0], : shape[1], : shape[2]] = mass
    mr, mi = transform(big, np.zeros(padded))
    kr, ki = transform(kernel_grid(shape, spacing, soften), np.zeros(padded))
    pr = kr * mr - ki * mi
    pi = kr * mi + ki * mr
    re, im = transform(pr, pi, inverse=True)
    points = float(np.prod(padded))
    return np.ascontiguousarray(((-g) * (re * (1.0 / points)) + 0.0)[: shape[0], : shape[1], : shape[2]])


# ---- inputs
def masses(shape, kind, seed=0):
    """random masses with a spread of 2^20 | a single non-zero cell | all zero"""
    rng = np.random.default_rng(1000 * seed + sum(shape) + 7 * shape[0])
    if kind == "zero":
        return np.zeros(shape)
    if kind == "single":
        m = np.zeros(shape)
        m.reshape(-1)[int(rng.integers(0, m.size))] = 1.375
        return m
    return rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-10, 11, shape)


KINDS = ("random", "single", "zero")


# ---- exact oracles
def direct_sum(mass, spacing, g, soften):
    """-g sum_c' M[c'] Kr(c - c') in np.longdouble"""
    mass = np.asarray(mass, np.float64)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in mass.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.longdouble)
    m = mass.reshape(-1).astype(np.longdouble)
    h, eps = np.longdouble(spacing), np.longdouble(soften)
    d = (idx[:, None, :] - idx[None, :, :]) * h
    r2 = (d * d).sum(-1) + eps * eps
    with np.errstate(divide="ignore"):
        kr = 1.0 / np.sqrt(r2)
    if soften == 0.0:
        kr[np.arange(len(m)), np.arange(len(m))] = 0.0
    return (-np.longdouble(g) * (kr @ m)).reshape(mass.shape)


def numpy_periodic(mass, spacing, g, green, deconvolve=0, scheme=CIC):
    """the periodic solve by numpy.fft with the same per-axis tables"""
    f = green_factor(mass.shape, spacing, g, green, deconvolve, scheme)
    return np.fft.ifftn(f * np.fft.fftn(mass)).real


def laplacian7(phi, spacing):
    """the 7-point Laplacian with wrapped indices"""
    out = -6.0 * phi
    for axis in range(3):
        out = out + np.roll(phi, 1, axis) + np.roll(phi, -1, axis)
    return out / (spacing * spacing)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        r = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} cells differ, first {r}: {got[r]!r} vs {want[r]!r}")
