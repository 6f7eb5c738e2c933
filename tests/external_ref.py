"""The static external field restated in numpy (include/nbody_hip.h, "external field").

Accelerations: operation by operation in the precision asked for (np.float32 or np.float64), in the order the header fixes.
numpy rounds every array operation on its own and its sqrt and divide are IEEE, so these are the library's bits in both math
modes.  Potentials: the header's expressions in plain f64.

A component here is (kind, p, center): kind one of PLUMMER, HERNQUIST, MIYAMOTO_NAGAI, LOGARITHMIC, p the kind's parameters
(padded to four with zeros), center three coordinates."""
import numpy as np

PLUMMER, HERNQUIST, MIYAMOTO_NAGAI, LOGARITHMIC = 0, 1, 2, 3

#: one field per kind and one mix of eight components, off-centre so that no coordinate is special
FIELDS = {
    "plummer": [(PLUMMER, (3.0, 0.25), (0.125, -0.25, 0.0625))],
    "point": [(PLUMMER, (2.5, 0.0), (-0.3, 0.1, 0.2))],
    "hernquist": [(HERNQUIST, (10.0, 1.5), (0.0, 0.2, -0.1))],
    "mn": [(MIYAMOTO_NAGAI, (5.0, 3.0, 0.3), (0.1, 0.0, 0.05))],
    "mn_a0": [(MIYAMOTO_NAGAI, (5.0, 0.0, 0.3), (0.0, 0.0, 0.0))],
    "log": [(LOGARITHMIC, (1.2, 0.5, 0.9, 0.7), (0.05, -0.05, 0.0))],
    "mix8": [(PLUMMER, (3.0, 0.25), (0.125, -0.25, 0.0625)), (HERNQUIST, (10.0, 1.5), (0.0, 0.2, -0.1)),
             (MIYAMOTO_NAGAI, (5.0, 3.0, 0.3), (0.1, 0.0, 0.05)), (LOGARITHMIC, (1.2, 0.5, 0.9, 0.7), (0.05, -0.05, 0.0)),
             (PLUMMER, (0.5, 0.0), (1.0, 1.0, 1.0)), (HERNQUIST, (-2.0, 0.7), (-1.0, 0.5, 0.25)),
             (MIYAMOTO_NAGAI, (1.0, 0.0, 1.0), (0.0, -1.0, 0.0)), (LOGARITHMIC, (0.3, 2.0, 1.0, 1.0), (0.0, 0.0, 0.0))],
}


def padded(p):
    return tuple(float(v) for v in p) + (0.0,) * (4 - len(p))


def to_abi(nb, comps):
    """the components as the mirror's NbodyExternalComponent records"""
    return [nb.external_component(kind, padded(p), center) for kind, p, center in comps]


def acc_terms(comp, g, pos, dtype):
    """[n, 3] of dtype: one component's term, every operation rounded to dtype on its own"""
    F = np.dtype(dtype).type
    kind, p, center = comp
    p = [F(v) for v in padded(p)]
    c = [F(v) for v in center]
    g = F(g)
    pos = np.asarray(pos, dtype)
    dx, dy, dz = pos[:, 0] - c[0], pos[:, 1] - c[1], pos[:, 2] - c[2]
    zero = np.zeros_like(dx)
    with np.errstate(all="ignore"):
        if kind == PLUMMER:
            r2 = ((dx * dx + dy * dy) + dz * dz) + p[1] * p[1]
            r = np.sqrt(r2)
            f = (g * p[0]) / (r2 * r)
            t = [-(dx * f), -(dy * f), -(dz * f)]
            skip = r2 == 0
        elif kind == HERNQUIST:
            r = np.sqrt((dx * dx + dy * dy) + dz * dz)
            ra = r + p[1]
            f = (g * p[0]) / (r * (ra * ra))
            t = [-(dx * f), -(dy * f), -(dz * f)]
            skip = r == 0
        elif kind == MIYAMOTO_NAGAI:
            B = np.sqrt(dz * dz + p[2] * p[2])
            aB = p[1] + B
            D = (dx * dx + dy * dy) + aB * aB
            f = (g * p[0]) / (D * np.sqrt(D))
            fz = (f * aB) / B
            t = [-(dx * f), -(dy * f), -(dz * fz)]
            skip = np.zeros(len(dx), bool)
        elif kind == LOGARITHMIC:
            yq, zq = dy / p[2], dz / p[3]
            S = ((p[1] * p[1] + dx * dx) + yq * yq) + zq * zq
            f = (p[0] * p[0]) / S
            t = [-(dx * f), -((dy / (p[2] * p[2])) * f), -((dz / (p[3] * p[3])) * f)]
            skip = np.zeros(len(dx), bool)
        else:
            raise ValueError(kind)
    out = np.stack([np.where(skip, zero, v) for v in t], axis=1)
    assert out.dtype == np.dtype(dtype)
    return out


def acc(comps, g, pos, dtype):
    """s [n, 3] of dtype: s = 0, then s += term for the components in ascending order"""
    s = np.zeros((len(pos), 3), dtype)
    for comp in comps:
        s = s + acc_terms(comp, g, pos, dtype)
    return s


def phi_terms(comp, g, pos):
    """[n] f64: one component's potential (Plummer: 0 where the term is skipped)"""
    kind, p, center = comp
    p = padded(p)
    pos = np.asarray(pos, np.float64)
    dx, dy, dz = pos[:, 0] - center[0], pos[:, 1] - center[1], pos[:, 2] - center[2]
    g = float(g)
    with np.errstate(all="ignore"):
        if kind == PLUMMER:
            r2 = ((dx * dx + dy * dy) + dz * dz) + p[1] * p[1]
            return np.where(r2 == 0, 0.0, -((g * p[0]) / np.sqrt(r2)))
        if kind == HERNQUIST:
            return -((g * p[0]) / (np.sqrt((dx * dx + dy * dy) + dz * dz) + p[1]))
        if kind == MIYAMOTO_NAGAI:
            aB = p[1] + np.sqrt(dz * dz + p[2] * p[2])
            return -((g * p[0]) / np.sqrt((dx * dx + dy * dy) + aB * aB))
        if kind == LOGARITHMIC:
            yq, zq = dy / p[2], dz / p[3]
            S = ((p[1] * p[1] + dx * dx) + yq * yq) + zq * zq
            return (0.5 * (p[0] * p[0])) * np.log(S)
    raise ValueError(kind)


def phi(comps, g, pos):
    """(phi [n] f64 summed over the components in ascending order, T [n] = the sum of the terms' magnitudes)"""
    total = np.zeros(len(pos), np.float64)
    mags = np.zeros(len(pos), np.float64)
    for comp in comps:
        t = phi_terms(comp, g, pos)
        total = total + t
        mags = mags + np.abs(t)
    return total, mags


# The bound of a potential against this restatement: (PHI_K + C) 2^-53 T_i, C = components, T_i = sum of |term|.
# PHI_K = the roundings of the longest potential expression as restated, the logarithmic one, along its deepest chain:
#   d = x - c (1), d / q (1), its square (1), the three additions into S (3), log (2: a library logarithm is within 1 ulp,
#   counted twice because the library's and numpy's may differ by two), v0 v0 (1), its half (exact, 0), the product (1)
# = 11.  The other kinds are shorter (Miyamoto-Nagai: 10).  Every term is a product / quotient of positive sums, so each
# rounding moves it by at most 2^-53 of its magnitude -- except the logarithm's argument near S = 1, where ln S loses relative
# accuracy; the test fields keep rc^2 + |d|^2 away from 1 by construction or the term is dominated by the others in T_i.
# The C summations of terms add at most C 2^-53 T_i.
PHI_K = 11


def phi_bound(comps, mags):
    return (PHI_K + len(comps)) * 2.0 ** -53 * mags


def leapfrog_orbits(comps, g, rec, dts, lo, hi):
    """The leapfrog of include/nbody_hip.h on massless particles in the external field alone, f32, bit for bit: half drift,
    retain by the inclusive walls [lo, hi] (order kept), acc = 0 + s(x), kick, half drift.  rec: PointParticle<f32> records."""
    rec = rec.copy()
    half = np.float32(0.5)
    for dt in dts:
        dt = np.float32(dt)
        x, v = rec["position"], rec["velocity"]
        x = x + (v * half) * dt
        keep = ((x >= np.float32(lo)) & (x <= np.float32(hi))).all(axis=1)
        rec = rec[keep]
        x, v = x[keep], v[keep]
        a = np.zeros_like(x) + acc(comps, g, x, np.float32)
        v = v + a * dt
        x = x + (v * half) * dt
        rec["position"], rec["velocity"], rec["acceleration"] = x, v, a
    return rec
