"""numpy restatement of nbody_partners and nbody_bound_pairs (include/nbody_hip.h, "binary census"), bit for bit: the full n x n
matrix of two-body energies in f64, every product, sum and difference a numpy operation of its own (nothing contracted, IEEE
sqrt and divide), a diagonal of +inf, NaN mapped to +inf, argmin with the lowest index on ties; the mutual pairs of negative
energy and their orbital elements in the arithmetic the header writes beside the fields of NbodyBoundPair."""
import numpy as np

BOUND_PAIR_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("energy", "<f8"), ("binding", "<f8"), ("semi_major", "<f8"),
                             ("eccentricity", "<f8"), ("period", "<f8"), ("separation", "<f8")])
FIELDS = BOUND_PAIR_DTYPE.names
TWO_PI = 6.283185307179586


class Mismatch(AssertionError):
    pass


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    b = np.ascontiguousarray(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def widened(rec):
    """(x [n, 3], v [n, 3], m [n]) in f64: exact for f32 records"""
    return (np.ascontiguousarray(rec["position"], np.float64), np.ascontiguousarray(rec["velocity"], np.float64),
            np.ascontiguousarray(rec["mass"], np.float64))


def settings_of(sim):
    """(g, g_soft) as the handle holds them, widened (an f32 handle has rounded them to f32)"""
    s = sim.settings
    return float(s.g), float(s.g_soft)


def energy_matrix(rec, g, g_soft):
    """e[i, j] = 0.5 w2 - (g (m_i + m_j)) / sqrt(r2), the diagonal included as computed"""
    x, v, m = widened(rec)
    g, g_soft = np.float64(g), np.float64(g_soft)
    with np.errstate(all="ignore"):
        soft2 = g_soft * g_soft
        d = [x[None, :, c] - x[:, None, c] for c in range(3)]   # d[i, j] = x_j - x_i
        r2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + soft2
        del d
        w = [v[None, :, c] - v[:, None, c] for c in range(3)]
        w2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        del w
        return 0.5 * w2 - (g * (m[:, None] + m[None, :])) / np.sqrt(r2)


def partners(rec, g, g_soft):
    """(partner [n] int32, energy [n] f64)"""
    n = len(rec)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float64)
    e = energy_matrix(rec, g, g_soft)
    e[np.arange(n), np.arange(n)] = np.inf
    e[np.isnan(e)] = np.inf
    j = np.argmin(e, axis=1)   # the first of equal minima
    best = e[np.arange(n), j]
    partner = np.where(best < np.inf, j, -1).astype(np.int32)
    return partner, best


def bound_pairs(rec, g, g_soft):
    """(pairs [BOUND_PAIR_DTYPE] in ascending i, binding_sum)"""
    partner, energy = partners(rec, g, g_soft)
    n = len(rec)
    idx = np.arange(n)
    safe = np.where(partner >= 0, partner, 0)
    first = (partner > idx) & (partner[safe] == idx) & (energy < 0.0) if n else np.zeros(0, bool)
    i = idx[first]
    j = partner[first].astype(np.int64)
    x, v, m = widened(rec)
    g = np.float64(g)
    out = np.zeros(len(i), BOUND_PAIR_DTYPE)
    with np.errstate(all="ignore"):
        dx, dy, dz = (x[j, c] - x[i, c] for c in range(3))
        wx, wy, wz = (v[j, c] - v[i, c] for c in range(3))
        e = energy[i]
        M = m[i] + m[j]
        gm = g * M
        hx, hy, hz = dy * wz - dz * wy, dz * wx - dx * wz, dx * wy - dy * wx
        h2 = (hx * hx + hy * hy) + hz * hz
        a = gm / (-2.0 * e)
        q = 1.0 + ((2.0 * e) * h2) / (gm * gm)
        out["i"], out["j"] = i, j
        out["energy"] = e
        out["binding"] = ((m[i] * m[j]) / M) * e
        out["semi_major"] = a
        out["eccentricity"] = np.sqrt(np.where(q > 0.0, q, 0.0))
        out["period"] = TWO_PI * (a * np.sqrt(a / gm))
        out["separation"] = np.sqrt((dx * dx + dy * dy) + dz * dz)
        total = 0.0
        for b in out["binding"]:
            total = total + float(b)
    return out, total


def check_partners(partner, energy, rec, g, g_soft):
    want_p, want_e = partners(rec, g, g_soft)
    partner = np.asarray(partner)
    if partner.dtype != np.int32 or partner.shape != want_p.shape or not np.array_equal(partner, want_p):
        bad = np.nonzero(partner != want_p)[0] if partner.shape == want_p.shape else []
        raise Mismatch(f"partner differs at {list(bad[:8])}: got {list(partner[bad[:8]])}, want {list(want_p[bad[:8]])}")
    if not same_bits(energy, want_e):
        raise Mismatch("energy differs in bits")


def check_bound_pairs(pairs, binding_sum, rec, g, g_soft):
    want, want_sum = bound_pairs(rec, g, g_soft)
    if len(pairs) != len(want):
        raise Mismatch(f"{len(pairs)} pairs, want {len(want)}")
    for f in ("i", "j"):
        if not np.array_equal(pairs[f], want[f]):
            raise Mismatch(f"{f} differs")
    for f in FIELDS[2:]:
        if not same_bits(pairs[f], want[f]):
            bad = np.nonzero(np.ascontiguousarray(pairs[f]).view(np.uint64) != np.ascontiguousarray(want[f]).view(np.uint64))[0]
            raise Mismatch(f"{f} differs in bits at {list(bad[:8])}: got {list(pairs[f][bad[:8]])}, want {list(want[f][bad[:8]])}")
    if not same_bits(binding_sum, want_sum):
        raise Mismatch(f"binding sum {binding_sum!r}, want {want_sum!r}")
    return len(want)


# ------------------------------------------------------------------------------------------------ bodies with planted binaries
def planted_bodies(nb, n, planted, seed, f64=True):
    """n normal-random bodies (velocities scaled by 0.5, masses uniform in [0.5, 1.5] / n); for k < planted, body 2k + 1 is
    placed at separation 1e-3 (k + 1) from body 2k along a random direction and moves, relative to it, at 0.8 of the circular
    speed sqrt(g M / r) (g = 1) perpendicular to the separation.  Returns the records."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 3))
    v = 0.5 * rng.standard_normal((n, 3))
    m = rng.uniform(0.5, 1.5, n) / n
    for k in range(planted):
        a, b = 2 * k, 2 * k + 1
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        t = np.cross(u, rng.standard_normal(3))
        t /= np.linalg.norm(t)
        r = 1e-3 * (k + 1)
        x[b] = x[a] + r * u
        v[b] = v[a] + 0.8 * np.sqrt((m[a] + m[b]) / r) * t
    rec = np.zeros(n, nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    rec["position"], rec["velocity"], rec["mass"] = x, v, m
    return rec


def lattice_bodies(nb, side, f64):
    """side^3 equal masses at rest on an exact integer lattice: every energy is -g 2m / sqrt(integer), ties everywhere"""
    g = np.arange(side, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rec = np.zeros(len(x), nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    rec["position"] = x
    rec["mass"] = 0.25
    return rec
