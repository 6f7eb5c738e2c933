"""numpy restatement of nbody_fof_bound_groups (include/nbody_hip.h, "self-bound subsets of friends-of-friends groups"), built
on fof_ref.labels and fof_ref.groups: per listed FoF group the alive flags, the seven sums of the alive members in the header's
lane order (k = the position in the FoF list), every alive member's energy with the partner sum cut into tiles of 256
positions -- vectorised over the members i, sequential over the partners k inside a tile, so the association order is the
header's --, the verdict !(e < 0), strip-all-at-once, and the records, members and energies of what is left, bit for bit."""
import numpy as np

import fof_ref
from fof_ref import Mismatch, same_bits  # noqa: F401  (re-exported for the tests)

BOUND_GROUP_DTYPE = np.dtype([("first", "<i4"), ("fof_count", "<i4"), ("count", "<i4"), ("offset", "<i4"), ("iterations", "<i4"),
                              ("converged", "<i4"), ("mass", "<f8"), ("mx", "<f8", (3,)), ("mv", "<f8", (3,)), ("kinetic", "<f8"),
                              ("potential", "<f8")])
TILE = 256


def lane_tree_sum_alive(terms, alive):
    """the header's order for one group with flags: lane k mod 64 adds its ALIVE terms in ascending k from +0.0 (k = the position
    in the FoF list; a dead member adds nothing), then sum[t] += sum[t + half] for half = 32 .. 1"""
    terms = np.asarray(terms, np.float64)
    rows = -(-len(terms) // 64)
    t = np.zeros(rows * 64, np.float64)
    a = np.zeros(rows * 64, bool)
    t[: len(terms)], a[: len(terms)] = terms, alive
    s = np.zeros(64, np.float64)
    for row_t, row_a in zip(t.reshape(rows, 64), a.reshape(rows, 64)):
        s = np.where(row_a, s + row_t, s)
    half = 32
    while half >= 1:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0]


def seven_sums(x, v, m, alive):
    """[7]: m, m x_c, m v_c of the alive members, each product rounded once"""
    out = [lane_tree_sum_alive(m, alive)]
    out += [lane_tree_sum_alive(m * x[:, c], alive) for c in range(3)]
    out += [lane_tree_sum_alive(m * v[:, c], alive) for c in range(3)]
    return np.array(out, np.float64)


def evaluate(x, v, m, alive, g, soft2):
    """one evaluation pass on the alive set of one group: (sums [7], e [count], u2, phi); the entries of dead members mean nothing"""
    cnt = len(m)
    sums = seven_sums(x, v, m, alive)
    V = sums[4:7] / sums[0]
    own = np.arange(cnt)
    s = np.zeros(cnt, np.float64)
    for t0 in range(0, cnt, TILE):
        p = np.zeros(cnt, np.float64)
        for k in range(t0, min(t0 + TILE, cnt)):
            if not alive[k]:
                continue
            dx, dy, dz = x[k, 0] - x[:, 0], x[k, 1] - x[:, 1], x[k, 2] - x[:, 2]
            r2 = ((dx * dx + dy * dy) + dz * dz) + soft2
            p = np.where(own != k, p + m[k] / np.sqrt(r2), p)
        s = s + p   # every tile, also one with no live partner
    phi = -(g * s)
    ux, uy, uz = v[:, 0] - V[0], v[:, 1] - V[1], v[:, 2] - V[2]
    u2 = (ux * ux + uy * uy) + uz * uz
    return sums, 0.5 * u2 + phi, u2, phi


def bound_groups(rec, b, g, g_soft, min_members=2, max_iterations=32, lab=None, fof=None, history=None):
    """(groups [BOUND_GROUP_DTYPE], members [int32], energy [f64]).  g and g_soft are the handle's settings, widened exactly (an
    f32 handle: np.float32 values).  fof = the (groups, members) of fof_ref.groups(rec, b, min_members), if already known.
    history (a dict, optional) receives per FoF group `first` the list of the positions k removed after each pass, and
    "dissolved": the firsts of the groups that are not listed."""
    assert min_members >= 2 and 1 <= max_iterations <= 1024
    g, g_soft = np.float64(g), np.float64(g_soft)
    soft2 = g_soft * g_soft
    grp, mem = fof_ref.groups(rec, b, min_members, lab=lab) if fof is None else fof
    X = np.ascontiguousarray(rec["position"], np.float64)   # exact for f32 records
    Vel = np.ascontiguousarray(rec["velocity"], np.float64)
    M = np.ascontiguousarray(rec["mass"], np.float64)
    out, members, energy, offset = [], [], [], 0
    if history is not None:
        history["dissolved"] = []
    with np.errstate(all="ignore"):
        for fg in grp:
            who = mem[fg["offset"]:fg["offset"] + fg["count"]]
            x, v, m = X[who], Vel[who], M[who]
            alive = np.ones(len(who), bool)
            removed, t, dissolved = [], 0, False
            while True:
                sums, e, u2, phi = evaluate(x, v, m, alive, g, soft2)
                unbound = alive & ~(e < 0)   # a NaN energy is unbound, -inf is bound
                if not unbound.any():
                    converged = 1
                    break
                if t + 1 == max_iterations:   # nobody is removed by the last pass
                    converged = 0
                    break
                alive &= ~unbound
                removed.append(np.nonzero(unbound)[0])
                if alive.sum() < min_members:
                    dissolved = True
                    break
                t += 1
            if history is not None:
                history[int(fg["first"])] = removed
                if dissolved:
                    history["dissolved"].append(int(fg["first"]))
            if dissolved:
                continue
            r = np.zeros((), BOUND_GROUP_DTYPE)
            r["first"], r["fof_count"], r["count"], r["offset"] = fg["first"], fg["count"], alive.sum(), offset
            r["iterations"], r["converged"] = t + 1, converged
            r["mass"], r["mx"], r["mv"] = sums[0], sums[1:4], sums[4:7]
            r["kinetic"] = lane_tree_sum_alive((0.5 * m) * u2, alive)
            r["potential"] = lane_tree_sum_alive((0.5 * m) * phi, alive)
            out.append(r)
            members.append(who[alive])
            energy.append(e[alive])
            offset += int(alive.sum())
    return (np.array(out, BOUND_GROUP_DTYPE) if out else np.zeros(0, BOUND_GROUP_DTYPE),
            np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32),
            np.concatenate(energy).astype(np.float64) if energy else np.zeros(0, np.float64))


def brute_energy(rec, who, g, g_soft):
    """an independent f64 reference for the members `who` (the alive set of one group): (e [len(who)], bound [len(who)]) with
    plain np.sum over the partners; bound_i = fof-count-free part of the tolerance: g sum_k |term_ik| + (|u_i| + sum_k |m v|_k / M)^2"""
    x = np.asarray(rec["position"], np.float64)[who]
    v = np.asarray(rec["velocity"], np.float64)[who]
    m = np.asarray(rec["mass"], np.float64)[who]
    d = x[None, :, :] - x[:, None, :]
    with np.errstate(all="ignore"):
        inv = m[None, :] / np.sqrt(np.sum(d * d, axis=2) + np.float64(g_soft) ** 2)
    inv[np.arange(len(who)), np.arange(len(who))] = 0.0
    phi = -np.float64(g) * np.sum(inv, axis=1)
    mean = np.sum(m[:, None] * v, axis=0) / np.sum(m)
    u = v - mean
    e = 0.5 * np.sum(u * u, axis=1) + phi
    bound = np.float64(g) * np.sum(np.abs(inv), axis=1) + (np.linalg.norm(u, axis=1) + np.sum(np.abs(m[:, None] * v)) / np.sum(m)) ** 2
    return e, bound


# ------------------------------------------------------------------------------------------------ checks
def check_bound_groups(got, got_members, got_energy, want, want_members, want_energy):
    """every byte of the records, the members and the energies"""
    if len(got) != len(want):
        raise Mismatch(f"{len(got)} bound groups, want {len(want)}")
    if np.asarray(got).dtype != BOUND_GROUP_DTYPE:
        raise Mismatch(f"records of dtype {np.asarray(got).dtype}")
    for f in ("first", "fof_count", "count", "offset", "iterations", "converged"):
        if not np.array_equal(got[f], want[f]):
            raise Mismatch(f"{f} differs: got {list(got[f][:8])}, want {list(want[f][:8])}")
    if np.asarray(got_members).dtype != np.int32 or not np.array_equal(got_members, want_members):
        raise Mismatch("the member lists differ")
    for f in ("mass", "mx", "mv", "kinetic", "potential"):
        if not same_bits(got[f], want[f]):
            bad = np.nonzero((np.asarray(got[f]).view(np.uint64) != np.asarray(want[f]).view(np.uint64)).reshape(len(got), -1).any(axis=1))[0]
            raise Mismatch(f"{f} differs in bits in groups {list(bad[:8])}: got {got[f][bad[:2]]}, want {want[f][bad[:2]]}")
    if np.asarray(got_energy).dtype != np.float64 or not same_bits(got_energy, want_energy):
        bad = np.nonzero(np.asarray(got_energy).view(np.uint64) != np.asarray(want_energy).view(np.uint64))[0] \
            if len(got_energy) == len(want_energy) else []
        raise Mismatch(f"the energies differ in bits at {list(bad[:8])} ({len(bad)} in all)")
    if np.asarray(got).tobytes() != np.asarray(want).tobytes():
        raise Mismatch("the records differ in bytes")


# ------------------------------------------------------------------------------------------------ bodies
WORLD_B = fof_ref.CLUMPY_B
WORLD_G, WORLD_G_SOFT = 1.0, 0.05
BIG, HOT, COLD = np.array([3.0, 0.0, 0.0]), np.array([-3.0, 2.0, 0.0]), np.array([0.0, 4.0, -4.0])


def _directions(rng, n):
    u = rng.standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def world(nb, n, f64):
    """fof_ref.clumpy(n)'s geometry for the linking length WORLD_B -- background singletons, the blob of n / 5 bodies at BIG, the
    one of n / 11 at HOT, up to five pairs -- plus a third blob of n / 16 background bodies moved to COLD, and velocities that
    decide every group's fate under g = WORLD_G, g_soft = WORLD_G_SOFT (the big blob's mass is 0.2, its central escape speed
    about 1.8):
      BIG   speeds uniform in [0, 2) in random directions: the fastest escape in the first pass, which makes the well
            shallower, so more escape in the next one -- several passes, members lost in more than one.  The lowest-index
            bodies of the blob, up to and including the first one within 0.1 of its centre (a sure member), move at 4: the
            group's `first` is itself removed
      HOT   speeds in [4, 8): well above escape (about 1.5); the group dissolves after its first pass
      COLD  a common drift plus 0.01 normal: bound, nobody removed, one pass
      the pairs (and the two bodies of n == 2) share one velocity: bound"""
    rec = fof_ref.clumpy(nb, n, seed=n, f64=f64).copy()
    if n == 0:
        return rec
    rng = np.random.default_rng(7919 + n)
    x = np.asarray(rec["position"], np.float64)
    far = lambda c, r: np.linalg.norm(x - c, axis=1) > r   # noqa: E731
    loose = np.nonzero(far(BIG, 1.0) & far(HOT, 1.0) & (np.abs(x[:, 2] - 6.0) > 0.5))[0][: n // 16]
    if n >= 255:
        rec["position"][loose] = COLD + 0.04 * rng.standard_normal((len(loose), 3))
        rec["velocity"][loose] = np.array([1.0, 0.5, -0.25]) + 0.01 * rng.standard_normal((len(loose), 3))
    x = np.asarray(rec["position"], np.float64)
    big = np.nonzero(~far(BIG, 0.6))[0]
    rec["velocity"][big] = np.array([0.3, -0.2, 0.1]) + rng.uniform(0.0, 2.0, (len(big), 1)) * _directions(rng, len(big))
    core = big[np.linalg.norm(x[big] - BIG, axis=1) < 0.1]
    if len(core):
        fast = big[big <= core[0]]
        rec["velocity"][fast] = 4.0 * _directions(rng, len(fast))
    hot = np.nonzero(~far(HOT, 0.5))[0]
    rec["velocity"][hot] = rng.uniform(4.0, 8.0, (len(hot), 1)) * _directions(rng, len(hot))
    pairs = np.nonzero((np.abs(x[:, 2] - 6.0) < 0.01) & (np.abs(x[:, 0]) < 0.05))[0]
    rec["velocity"][pairs] = np.array([0.2, 0.0, -0.1])
    if n == 2:
        rec["velocity"][1] = rec["velocity"][0]
    return rec
