"""numpy restatement of nbody_nearest, nbody_contacts and nbody_merge_contacts (include/nbody_hip.h, "sticky mergers"), bit for
bit: the full n x n matrix of unsoftened squared distances in f64, every product, sum and difference a numpy operation of its
own (nothing contracted), a diagonal of +inf, NaN mapped to +inf, argmin with the lowest index on ties; the mutual pairs with
r2 < radius * radius (strict), every field of NbodyContact, and the merged records -- f64 arithmetic, then one rounding to the
records' own type."""
import numpy as np

CONTACT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("into", "<i4"), ("reserved", "<i4"), ("separation", "<f8"), ("mass", "<f8"),
                          ("dkinetic", "<f8")])
FLOAT_FIELDS = ("separation", "mass", "dkinetic")
VECTORS = ("position", "velocity", "acceleration")


class Mismatch(AssertionError):
    pass


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    b = np.ascontiguousarray(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dist2_matrix(rec):
    """r2[i, j] = (dx dx + dy dy) + dz dz with d = x_j - x_i, the diagonal included as computed"""
    x = np.ascontiguousarray(rec["position"], np.float64)   # exact for f32 records
    with np.errstate(all="ignore"):
        d = [x[None, :, c] - x[:, None, c] for c in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def nearest(rec):
    """(nearest [n] int32, dist2 [n] f64)"""
    n = len(rec)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float64)
    r2 = dist2_matrix(rec)
    r2[np.arange(n), np.arange(n)] = np.inf
    r2[np.isnan(r2)] = np.inf
    j = np.argmin(r2, axis=1)   # the first of equal minima
    best = r2[np.arange(n), j]
    return np.where(best < np.inf, j, -1).astype(np.int32), best


def contacts(rec, radius):
    """the list [CONTACT_DTYPE] in ascending i"""
    near, d2 = nearest(rec)
    n = len(rec)
    idx = np.arange(n)
    R2 = np.float64(radius) * np.float64(radius)
    safe = np.where(near >= 0, near, 0)
    first = (near > idx) & (near[safe] == idx) & (d2 < R2) if n else np.zeros(0, bool)
    i = idx[first]
    j = near[first].astype(np.int64)
    v = np.ascontiguousarray(rec["velocity"], np.float64)
    m = np.ascontiguousarray(rec["mass"], np.float64)
    out = np.zeros(len(i), CONTACT_DTYPE)
    with np.errstate(all="ignore"):
        wx, wy, wz = (v[j, c] - v[i, c] for c in range(3))
        w2 = (wx * wx + wy * wy) + wz * wz
        M = m[i] + m[j]
        out["i"], out["j"] = i, j
        out["into"] = i - np.searchsorted(np.sort(j), i, side="left")   # i minus the absorbed bodies below i
        out["separation"] = np.sqrt(d2[i])
        out["mass"] = M
        out["dkinetic"] = np.where(M == 0.0, 0.0, -0.5 * (((m[i] * m[j]) / M) * w2))
    return out


def merged1(mi, qi, mj, qj, M):
    """((m_i q_i) + (m_j q_j)) / M per element, every operation rounded on its own; M == 0: (q_i + q_j) 0.5"""
    with np.errstate(all="ignore"):
        return np.where(M == 0.0, (qi + qj) * 0.5, ((mi * qi) + (mj * qj)) / M)


def merge(rec, radius, extra=None):
    """(the records after nbody_merge_contacts, the list).  extra: an [n, 3] f64 array carried like the acceleration (a Hermite
    handle's jerk); then the merged extra comes third."""
    lst = contacts(rec, radius)
    i, j = lst["i"].astype(np.int64), lst["j"].astype(np.int64)
    out = rec.copy()
    m = np.ascontiguousarray(rec["mass"], np.float64)
    mi, mj = m[i], m[j]
    M = mi + mj
    for f in VECTORS:
        q = np.ascontiguousarray(rec[f], np.float64)
        out[f][i] = merged1(mi[:, None], q[i], mj[:, None], q[j], M[:, None])   # (the assignment rounds to the records' type once)
    out["mass"][i] = M
    keep = np.ones(len(rec), bool)
    keep[j] = False
    if extra is None:
        return out[keep], lst
    e = np.array(extra, np.float64)
    e[i] = merged1(mi[:, None], e[i], mj[:, None], e[j], M[:, None])
    return out[keep], lst, e[keep]


# ------------------------------------------------------------------------------------------------ checks
def check_nearest(got_nearest, got_dist2, rec):
    want_n, want_d = nearest(rec)
    got_nearest = np.asarray(got_nearest)
    if got_nearest.dtype != np.int32 or got_nearest.shape != want_n.shape or not np.array_equal(got_nearest, want_n):
        bad = np.nonzero(got_nearest != want_n)[0] if got_nearest.shape == want_n.shape else []
        raise Mismatch(f"nearest differs at {list(bad[:8])}: got {list(got_nearest[bad[:8]])}, want {list(want_n[bad[:8]])}")
    if not same_bits(got_dist2, want_d):
        raise Mismatch("dist2 differs in bits")


def check_contacts(got, rec, radius):
    want = contacts(rec, radius)
    if len(got) != len(want):
        raise Mismatch(f"{len(got)} contacts, want {len(want)}")
    for f in ("i", "j", "into", "reserved"):
        if not np.array_equal(got[f], want[f]):
            raise Mismatch(f"{f} differs: got {list(got[f][:8])}, want {list(want[f][:8])}")
    for f in FLOAT_FIELDS:
        if not same_bits(got[f], want[f]):
            raise Mismatch(f"{f} differs in bits: got {list(got[f][:8])}, want {list(want[f][:8])}")
    return len(want)


def check_records(got, want, what="records"):
    if len(got) != len(want):
        raise Mismatch(f"{what}: {len(got)} against {len(want)} records")
    for f in VECTORS + ("mass",):
        if got[f].tobytes() != want[f].tobytes():
            bad = np.nonzero((np.asarray(got[f]) != np.asarray(want[f])).reshape(len(got), -1).any(axis=1))[0]
            raise Mismatch(f"{what}: {f} differs at rows {list(bad[:8])}")


# ------------------------------------------------------------------------------------------------ bodies
def cloud(nb, n, seed, f64, close=0):
    """n bodies, normal-random positions of scale 4 rounded to the records' type, random velocities, accelerations and masses in
    [0.5, 1.5] / n; for k < close, body n - 1 - 2k is moved to within 1e-3 of body 3k (pairs far apart in index) and given its
    velocity but for 1e-2 of a normal deviate a component (the pair stays together for a few steps)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    rec["position"] = 4.0 * rng.standard_normal((n, 3))
    rec["velocity"] = 0.5 * rng.standard_normal((n, 3))
    rec["acceleration"] = rng.standard_normal((n, 3))
    rec["mass"] = rng.uniform(0.5, 1.5, n) / max(n, 1)
    for k in range(close):
        a, b = 3 * k, n - 1 - 2 * k
        if a < b:
            rec["position"][b] = rec["position"][a] + 1e-3 * rng.uniform(0.2, 0.5, 3)
            rec["velocity"][b] = rec["velocity"][a] + 1e-2 * rng.standard_normal(3)
    return rec


def lattice(nb, side, f64, seed=3):
    """side^3 bodies on an exact integer lattice, random masses and velocities: ties at every distance"""
    rng = np.random.default_rng(seed)
    g = np.arange(side, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rec = np.zeros(len(x), nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    rec["position"] = x
    rec["velocity"] = rng.standard_normal(x.shape)
    rec["mass"] = rng.uniform(0.5, 1.5, len(x))
    return rec
