"""numpy restatement of nbody_moments and nbody_lagrangian_radii (include/nbody_hip.h, "diagnostics of the state as a whole").

Moments: the ten sums in the device's association order -- per block of 256 bodies the pairwise tree sum[t] += sum[t + half],
the blocks then added in ascending order -- so the device's output is reproduced BIT FOR BIT.

Radii: the exact order of the bodies by (r2, index), np.longdouble prefix sums of the masses in that order, and for every
fraction the set of bodies ADMISSIBLE under the prefix bound the header states (every c_j within n 2^-53 sum|m| of the exact
prefix).  Where all prefixes are exact in f64 (masses that are integer multiples of 2^-20) the answer is unique and
radii_exact gives it bit for bit."""
import numpy as np

WIDTH = 256


class Mismatch(AssertionError):
    pass


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------- moments
def moment_terms(rec):
    """[n, 10] f64: per body m, m x_c, m v_c, l_c -- every product and difference rounded on its own"""
    x = rec["position"].astype(np.float64)
    v = rec["velocity"].astype(np.float64)
    m = rec["mass"].astype(np.float64)
    t = np.zeros((len(rec), 10))
    t[:, 0] = m
    for c in range(3):
        t[:, 1 + c] = m * x[:, c]
        t[:, 4 + c] = m * v[:, c]
    t[:, 7] = (x[:, 1] * v[:, 2] - x[:, 2] * v[:, 1]) * m
    t[:, 8] = (x[:, 2] * v[:, 0] - x[:, 0] * v[:, 2]) * m
    t[:, 9] = (x[:, 0] * v[:, 1] - x[:, 1] * v[:, 0]) * m
    return t


def tree_sum(terms, width=WIDTH):
    """columns of terms [n, q] summed like the device: blocks of `width` rows padded with +0.0, sum[t] += sum[t + half] for
    half = width / 2 ... 1, then the block sums added to +0.0 in ascending block order"""
    terms = np.asarray(terms, np.float64)
    n, q = terms.shape
    blocks = -(-n // width)
    a = np.zeros((blocks * width, q))
    a[:n] = terms
    a = a.reshape(blocks, width, q)
    half = width // 2
    while half:
        a = a[:, :half] + a[:, half:2 * half]
        half //= 2
    out = np.zeros(q)
    for b in range(blocks):
        out = out + a[b, 0]
    return out


def moments(rec, width=WIDTH):
    """{M, X[3], P[3], L[3]} of PointParticle records, the device's bits"""
    return tree_sum(moment_terms(rec), width)


def center_of_mass(rec):
    mom = moments(rec)
    with np.errstate(divide="ignore", invalid="ignore"):
        return mom[1:4] / mom[0]


def check_moments(got, rec):
    """got: the ten doubles of nbody_moments (or a Moments tuple's raw values) for `rec`"""
    got = np.asarray(got, np.float64)
    want = moments(rec)
    if not same_bits(got, want):
        bad = [i for i in range(10) if bits(got)[i] != bits(want)[i]]
        raise Mismatch(f"moments differ from the restatement in components {bad}: {got[bad]} against {want[bad]}")


def raw(mom):
    """Simulation.moments() -> the ten doubles"""
    return np.concatenate([[mom.mass], mom.mass_dipole, mom.momentum, mom.angular_momentum])


# --------------------------------------------------------------------------------------------------------------- radii
def r2_of(rec, center):
    c = np.asarray(center, np.float64)
    d = rec["position"].astype(np.float64) - c
    with np.errstate(invalid="ignore", over="ignore"):
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def order_of(rec, center):
    """(indices of the bodies kept, ascending by (r2, index); r2 of every body)"""
    r2 = r2_of(rec, center)
    kept = np.nonzero(~np.isnan(r2))[0]
    return kept[np.argsort(r2[kept], kind="stable")], r2


def prefixes(rec, order):
    """np.longdouble inclusive prefix sums of the masses in that order"""
    return np.cumsum(rec["mass"].astype(np.float64)[order].astype(np.longdouble))


def radii_exact(rec, center, fractions):
    """(radii, mass) where every prefix is exact in f64 (asserted): the unique answer"""
    fractions = np.asarray(fractions, np.float64)
    order, r2 = order_of(rec, center)
    if not len(order):
        return np.full(len(fractions), np.nan), 0.0
    c = np.cumsum(rec["mass"].astype(np.float64)[order])
    assert np.array_equal(c.astype(np.longdouble), prefixes(rec, order)), "the prefixes of this body set are not exact in f64"
    mass = c[-1]
    j = np.searchsorted(c, fractions * mass, side="left")   # the first c_j >= target
    return np.sqrt(r2[order[j]]), float(mass)


def check_radii_exact(got_radii, got_mass, rec, center, fractions):
    want, mass = radii_exact(rec, center, fractions)
    if not same_bits(got_mass, mass):
        raise Mismatch(f"mass {got_mass!r} against {mass!r}")
    if not same_bits(got_radii, want):
        bad = np.nonzero(bits(got_radii) != bits(want))[0]
        raise Mismatch(f"radii differ for fractions {np.asarray(fractions)[bad][:5]}: {np.asarray(got_radii)[bad][:5]} against {want[bad][:5]}")


def admissible(rec, center, fractions):
    """(first, last, order, r2, exact mass, bound): for fraction k the bodies order[first[k] .. last[k]] are the ones a scan
    within the stated bound may pick.  bound = n 2^-53 sum|m| for the device's prefixes, + n 2^-63 sum|m| for the longdouble
    prefixes they are compared with here (64-bit significand).  The device's mass lies within `bound` of the exact one, and its
    target f * mass carries one rounding, so the target lies in [f (E - bound) (1 - 2^-53), f (E + bound) (1 + 2^-53)]; body j
    can be picked iff its prefix may reach the target's low end while the one before it may stay below the high end."""
    fractions = np.asarray(fractions, np.float64).astype(np.longdouble)
    order, r2 = order_of(rec, center)
    n = len(order)
    assert n > 0 and (rec["mass"] >= 0).all()
    e = prefixes(rec, order)
    total = np.abs(rec["mass"].astype(np.float64)[order]).astype(np.longdouble).sum()
    bound = np.longdouble(n) * total * (np.longdouble(2.0) ** -53 + np.longdouble(2.0) ** -63)
    u = np.longdouble(2.0) ** -53
    t_lo = fractions * (e[-1] - bound) * (1 - u)
    t_hi = fractions * (e[-1] + bound) * (1 + u)
    first = np.searchsorted(e + bound, t_lo, side="left")
    last = np.minimum(np.searchsorted(e - bound, t_hi, side="left"), n - 1)
    assert (first <= last).all()
    return first, last, order, r2, e[-1], bound


def check_radii_admissible(got_radii, got_mass, rec, center, fractions):
    first, last, order, r2, mass, bound = admissible(rec, center, fractions)
    if not abs(np.longdouble(got_mass) - mass) <= bound:
        raise Mismatch(f"mass {got_mass!r} is further than the bound from {mass!r}")
    for k, r in enumerate(np.asarray(got_radii, np.float64)):
        ok = np.sqrt(r2[order[first[k]:last[k] + 1]])
        if not (bits(ok) == bits(r)).any():
            raise Mismatch(f"fraction {np.asarray(fractions)[k]!r}: radius {r!r} belongs to no admissible body ({ok[:4]})")
    return int((last > first).sum())


# ----------------------------------------------------------------------------------------------------------- body sets
def exact_mass_bodies(nb, n, seed, f64):
    """n Plummer bodies whose masses are integer multiples of 2^-20 and sum to a power of two: every prefix is exact in f64,
    f = c_j / M is exact and so is f * M -- the answer to every fraction is unique"""
    rec = nb.plummer(n, seed=seed, f64=f64)
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 64, n)
    total = 1 << int(np.ceil(np.log2(k.sum() + 1)))
    k[-1] += total - k.sum()
    rec["mass"] = k * 2.0 ** -20
    return rec


def exact_fractions(rec, center):
    """0, 1, 0.5, fractions landing exactly on a prefix and one ulp either side of it"""
    order, _ = order_of(rec, center)
    c = np.cumsum(rec["mass"].astype(np.float64)[order])
    on = c[np.unique(np.linspace(0, len(c) - 1, 7).astype(int))] / c[-1]
    fr = np.concatenate([[0.0, 1.0, 0.5], on, np.nextafter(on, 0.0), np.minimum(np.nextafter(on, 2.0), 1.0)])
    return fr
