"""numpy restatement of nbody_fof_labels and nbody_fof_groups (include/nbody_hip.h, "friends-of-friends groups"): the full n x n
matrix of unsoftened squared distances in f64 exactly as merge_ref.dist2_matrix computes it, the links r2 < b * b (strict, a NaN
never links), the labels by min-label propagation to a fixed point, the groups with at least min_members bodies in ascending
first index, their members in ascending index, and the seven sums of a group in the header's order -- lane t = k mod 64 adds
its terms in ascending k from +0.0, then sum[t] += sum[t + half] for half = 32 .. 1 -- bit for bit."""
import numpy as np

from merge_ref import Mismatch, dist2_matrix, same_bits  # noqa: F401  (re-exported for the tests)

GROUP_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("offset", "<i4"), ("reserved", "<i4"), ("mass", "<f8"),
                        ("mx", "<f8", (3,)), ("mv", "<f8", (3,))])


def links(rec, b):
    """[n, n] bool: r2 < B2 with B2 = b * b rounded once; the diagonal is cleared (a body is no friend of its own)"""
    n = len(rec)
    B2 = np.float64(b) * np.float64(b)
    with np.errstate(all="ignore"):
        adj = dist2_matrix(rec) < B2   # (a NaN compares false)
    adj[np.arange(n), np.arange(n)] = False
    return adj


def labels(rec, b):
    """[n] int32: the lowest index of every body's connected component.  Each round a body takes the least label among itself and
    its friends, then the label of its label (a body of its own component, so the round stays inside components); the fixed
    point is constant on components and is their minimum."""
    n = len(rec)
    lab = np.arange(n, dtype=np.int64)
    if n == 0:
        return lab.astype(np.int32)
    adj = links(rec, b)
    while True:
        new = np.minimum(lab, np.where(adj, lab[None, :], n).min(axis=1))
        new = new[new]
        if np.array_equal(new, lab):
            return lab.astype(np.int32)
        lab = new


def lane_tree_sum(terms):
    """the header's order for one group: terms [count] f64 -> one f64"""
    s = np.zeros(64, np.float64)
    for k, t in enumerate(np.asarray(terms, np.float64)):
        s[k % 64] = s[k % 64] + t   # lane k mod 64, ascending k, from +0.0
    half = 32
    while half >= 1:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0]


def groups(rec, b, min_members=2, lab=None):
    """(groups [GROUP_DTYPE] in ascending first, members [int32]): the components with count >= min_members"""
    lab = labels(rec, b) if lab is None else np.asarray(lab)
    x = np.ascontiguousarray(rec["position"], np.float64)   # exact for f32 records
    v = np.ascontiguousarray(rec["velocity"], np.float64)
    m = np.ascontiguousarray(rec["mass"], np.float64)
    roots, counts = np.unique(lab, return_counts=True)   # ascending
    out, members, offset = [], [], 0
    for root, count in zip(roots, counts):
        if count < min_members:
            continue
        who = np.nonzero(lab == root)[0]   # ascending
        g = np.zeros((), GROUP_DTYPE)
        g["first"], g["count"], g["offset"] = root, count, offset
        with np.errstate(all="ignore"):
            g["mass"] = lane_tree_sum(m[who])
            for c in range(3):
                g["mx"][c] = lane_tree_sum(m[who] * x[who, c])   # each product rounded once
                g["mv"][c] = lane_tree_sum(m[who] * v[who, c])
        out.append(g)
        members.append(who)
        offset += count
    return (np.array(out, GROUP_DTYPE) if out else np.zeros(0, GROUP_DTYPE),
            np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32))


# ------------------------------------------------------------------------------------------------ checks
def check_labels(got, n_groups, rec, b, want=None):
    want = labels(rec, b) if want is None else want
    got = np.asarray(got)
    if got.dtype != np.int32 or got.shape != want.shape or not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0] if got.shape == want.shape else []
        raise Mismatch(f"labels differ at {list(bad[:8])}: got {list(got[bad[:8]])}, want {list(want[bad[:8]])} ({len(bad)} in all)")
    if n_groups != len(np.unique(want)):
        raise Mismatch(f"{n_groups} groups, want {len(np.unique(want))}")


def check_groups(got, got_members, want, want_members):
    if len(got) != len(want):
        raise Mismatch(f"{len(got)} groups, want {len(want)}")
    for f in ("first", "count", "offset", "reserved"):
        if not np.array_equal(got[f], want[f]):
            raise Mismatch(f"{f} differs: got {list(got[f][:8])}, want {list(want[f][:8])}")
    if np.asarray(got_members).dtype != np.int32 or not np.array_equal(got_members, want_members):
        raise Mismatch("the member lists differ")
    for f in ("mass", "mx", "mv"):
        if not same_bits(got[f], want[f]):
            bad = np.nonzero((np.asarray(got[f]) != np.asarray(want[f])).reshape(len(got), -1).any(axis=1))[0]
            raise Mismatch(f"{f} differs in bits in groups {list(bad[:8])}")


# ------------------------------------------------------------------------------------------------ bodies
def _records(nb, x, f64, seed):
    rng = np.random.default_rng(seed)
    n = len(x)
    rec = np.zeros(n, nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE)
    rec["position"] = x   # (rounded to the records' type once)
    rec["velocity"] = 0.5 * rng.standard_normal((n, 3))
    rec["acceleration"] = rng.standard_normal((n, 3))
    rec["mass"] = rng.uniform(0.5, 1.5, n) / max(n, 1)
    return rec


CLUMPY_B = 0.1


def clumpy(nb, n, seed, f64):
    """n bodies for the linking length CLUMPY_B: a sparse uniform background in [-8, 8]^3 (singletons), a blob of n / 5 bodies and
    one of n / 11 (normal, sigma 0.08 and 0.06: one large group each and a few stragglers), and up to five pairs 0.05 apart --
    all at random indices, so that the blobs' members lie in every 256-body tile"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-8.0, 8.0, (n, 3))
    who = rng.permutation(n)
    a, b2, pairs = n // 5, n // 11, min(5, n // 20)
    at = 0
    x[who[at:at + a]] = np.array([3.0, 0.0, 0.0]) + 0.08 * rng.standard_normal((a, 3))
    at += a
    x[who[at:at + b2]] = np.array([-3.0, 2.0, 0.0]) + 0.06 * rng.standard_normal((b2, 3))
    at += b2
    for k in range(pairs):
        p, q = who[at + 2 * k], who[at + 2 * k + 1]
        x[p] = np.array([0.0, -5.0 + k, 6.0])
        x[q] = x[p] + np.array([0.03, 0.04, 0.0])
    if n == 2:
        x[1] = x[0] + np.array([0.03, 0.04, 0.0])
    return _records(nb, x, f64, seed + 1)


def lattice(nb, side, f64, seed=3):
    """side^3 bodies on an exact integer lattice, random masses and velocities: ties at every distance"""
    g = np.arange(side, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return _records(nb, x, f64, seed)


def chain(nb, n, b, f64, cut=None, seed=11):
    """n bodies on a line at spacing 0.9 b, their indices scrambled by a fixed permutation that keeps body 0 at the start of the
    line; cut = k: the gap between the k-th and (k + 1)-th body along the line is 1.1 b instead"""
    s = np.arange(n, dtype=np.float64) * (0.9 * b)
    if cut is not None:
        s[cut + 1:] += 0.2 * b
    perm = np.concatenate([[0], 1 + np.random.default_rng(seed).permutation(n - 1)])   # place along the line -> index
    x = np.zeros((n, 3))
    x[perm, 0] = s
    return _records(nb, x, f64, seed + 1), perm


def star(nb, n_shell, b, f64, hub=300, seed=13):
    """one hub (index `hub`) and n_shell bodies on a shell of radius 0.9 b about it"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n_shell + 1, 3))
    x = 5.0 + 0.9 * b * u / np.linalg.norm(u, axis=1)[:, None]
    x[hub] = 5.0
    return _records(nb, x, f64, seed + 1)


def two_lattices(nb, side, b, f64, seed=17):
    """two side^3 lattices of spacing 0.9 b, the second one clear of the first by a gap of 1.5 b along z; even indices are the
    first lattice's, odd ones the second's"""
    g = np.arange(side, dtype=np.float64) * (0.9 * b)
    one = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    other = one + np.array([0.0, 0.0, g[-1] + 1.5 * b])
    x = np.empty((2 * len(one), 3))
    x[0::2], x[1::2] = one, other
    return _records(nb, x, f64, seed)
