"""The probe checker of tests/hermite_probe.py, on the CPU: the plain f64 numpy evaluation of F passes it with a margin, and the
errors a pair-jerk kernel can make at a set or slice boundary -- one term dropped, doubled, with w negated, built from another
body's velocity, without its -3 (d.w)/q d part, or anything at all landing on the probe body itself -- fail it."""
import numpy as np
import pytest

import hermite_ref as hr
from bf64_bound import PROBE64
from hermite_probe import (MEASURED_RJP_WORST, PROBE_G, PROBE_MASS, RJP, check_probe_aj, probe_columns, probe_records64, probe_reference_aj,
                           probe_velocities, set_probe)

EPS = 2.0 ** -7


def probe_world(nb, n):
    pos = nb.plummer(2 * n + 64, seed=n)["position"]
    pos = np.ascontiguousarray(pos[np.abs(pos).max(1) < 30.0][:n], np.float64)
    assert len(pos) == n
    return pos, probe_velocities(n)


def numpy_aj(pos, vel, k, eps, block=255):
    """hermite_ref.fast_aj of the probe world of column k.  Massless bodies act on nothing, so the world is evaluated as
    sub-worlds of body k and `block` other bodies at a time: the rows are those of the whole world's evaluation bit for bit
    (every partner but k adds an exact zero), at n * block pair terms instead of n * n."""
    n = len(pos)
    a, j = np.zeros((n, 3)), np.zeros((n, 3))
    others = np.delete(np.arange(n), k)
    m = np.zeros(block + 1)
    m[0] = PROBE_MASS
    for c0 in range(0, max(1, len(others)), block):
        idx = np.concatenate([[k], others[c0:c0 + block]])
        sa, sj = hr.fast_aj(pos[idx], vel[idx], m[:len(idx)], PROBE_G, eps)
        a[idx], j[idx] = sa, sj
    return a, j


def test_sub_worlds_give_the_whole_worlds_rows_bit_for_bit(nb):
    pos, vel = probe_world(nb, 1025)
    for k, eps in ((0, 0.0), (512, EPS), (1024, 0.0)):
        m = np.zeros(1025)
        m[k] = PROBE_MASS
        a, j = hr.fast_aj(pos, vel, m, PROBE_G, eps)
        sa, sj = numpy_aj(pos, vel, k, eps)
        assert np.array_equal(a, sa) and np.array_equal(j, sj)
        ba, bj = hr.fast_aj_blocked(pos, vel, m, PROBE_G, eps, block=200)
        assert np.array_equal(a, ba) and np.array_equal(j, bj)


def test_the_bound_is_admissible():
    assert 13 * 2.0 ** -53 <= RJP <= 1e-13
    assert 2.5 * MEASURED_RJP_WORST <= RJP <= 4 * MEASURED_RJP_WORST       # about 3x the measurement


def test_probe_records_keep_their_velocities(nb):
    pos, vel = probe_world(nb, 65)
    rec = probe_records64(nb.PARTICLE_DTYPE64, pos, vel)
    rec["acceleration"] = 1.0
    for k in (3, 64):
        set_probe(rec, k)
        assert np.array_equal(rec["velocity"], vel) and np.array_equal(rec["position"], pos) and not rec["acceleration"].any()
        assert rec["mass"][k] == PROBE_MASS and np.count_nonzero(rec["mass"]) == 1
    assert (np.abs(vel).max(1) > 0).all() and len(np.unique(vel, axis=0)) == 65


@pytest.mark.parametrize("n,cols", [(65, None), (1025, (0, 255, 256, 511, 512, 1024)), (12033, (0, 255, 256, 6016, 12032))])
def test_numpy_f64_passes_the_probe_with_a_margin(nb, n, cols):
    pos, vel = probe_world(nb, n)
    cols = probe_columns(n, every_below=70) if cols is None else cols
    worst_a = worst_j = 0.0
    for c, k in enumerate(cols):
        eps = (0.0, EPS)[c % 2]
        a, j = numpy_aj(pos, vel, k, eps)
        ea, ej = check_probe_aj(a, j, pos, vel, k, PROBE_G, eps, what="numpy f64")
        worst_a, worst_j = max(worst_a, ea), max(worst_j, ej)
    print(f"\n[hermite probe checker] numpy f64 n={n} ({len(cols)} columns): worst |a - S_a| / |S_a| {worst_a:.3e}, |j - S_j| / T_j {worst_j:.3e}")
    assert worst_a <= PROBE64 / 4 and worst_j <= RJP / 4


def test_listed_rows_are_checked_against_their_own_bodies(nb):
    pos, vel = probe_world(nb, 300)
    k = 17
    a, j = numpy_aj(pos, vel, k, 0.0)
    ref = probe_reference_aj(pos, vel, k, PROBE_G, 0.0)
    ids = np.random.default_rng(1).permutation(300)[:100]
    ids[5] = k if k not in ids else ids[5]
    check_probe_aj(a[ids], j[ids], pos, vel, k, PROBE_G, 0.0, rows=ids, ref=ref, what="listed")
    with pytest.raises(AssertionError):        # the same rows in another order belong to other bodies
        check_probe_aj(a[np.sort(ids)], j[np.sort(ids)], pos, vel, k, PROBE_G, 0.0, rows=ids, ref=ref, what="misplaced")
    bad = j[ids].copy()
    bad[ids == k] = 1e-300
    with pytest.raises(AssertionError):
        check_probe_aj(a[ids], bad, pos, vel, k, PROBE_G, 0.0, rows=ids, ref=ref, what="self, listed")


def terms(pos, vel, k, i, eps, w=None, radial=True):
    """Body k's acceleration and jerk term at body i in f64, with the velocity difference and the radial part to choose."""
    d = pos[k] - pos[i]
    w = vel[k] - vel[i] if w is None else w
    q = d @ d + eps * eps
    c = PROBE_G * PROBE_MASS / (q * np.sqrt(q))
    return d * c, (w - (3.0 * (d @ w) / q if radial else 0.0) * d) * c


@pytest.mark.parametrize("eps", [0.0, EPS])
def test_probe_rejects_single_pair_errors(nb, eps):
    n = 1025
    pos, vel = probe_world(nb, n)
    for k in (0, 511, 512, n - 1):
        a, j = numpy_aj(pos, vel, k, eps)
        ref = probe_reference_aj(pos, vel, k, PROBE_G, eps)
        check = lambda aa, jj, what: check_probe_aj(aa, jj, pos, vel, k, PROBE_G, eps, ref=ref, what=what)  # noqa: E731
        check(a, j, "numpy f64")
        for i in ((k - 1) % n, (k + 1) % n, (k + 256) % n):
            ta, tj = terms(pos, vel, k, i, eps)
            assert np.allclose(ta, a[i], rtol=1e-14, atol=0) and np.allclose(tj, j[i], rtol=1e-12, atol=1e-14 * float(ref[2][i]))
            other = (i + 1) % n if (i + 1) % n != k else (i + 2) % n
            wrong = {
                "dropped": (0.0 * ta, 0.0 * tj),
                "doubled": (2.0 * ta, 2.0 * tj),
                "w negated": terms(pos, vel, k, i, eps, w=-(vel[k] - vel[i])),
                "another body's velocity": terms(pos, vel, k, i, eps, w=vel[k] - vel[other]),
                "no -3 (d.w)/q d": terms(pos, vel, k, i, eps, radial=False),
            }
            for name, (wa, wj) in wrong.items():
                bad = j.copy()
                bad[i] = wj
                with pytest.raises(AssertionError, match="jerks"):      # the jerk alone is wrong ...
                    check(a, bad, name)
                if name in ("dropped", "doubled"):                         # ... or the acceleration alone
                    bad = a.copy()
                    bad[i] = wa
                    with pytest.raises(AssertionError, match="accelerations"):
                        check(bad, j, name)
                else:
                    assert np.array_equal(wa, ta)
        # the self pair (0 * inf at eps = 0) or any term landing on the probe body itself: in a and, separately, in j
        for value in (a[(k + 1) % n], j[(k + 1) % n], 1e-300, np.nan, np.inf):
            bad = a.copy()
            bad[k] = value
            with pytest.raises(AssertionError, match="accelerations"):
                check(bad, j, "row k of a")
            bad = j.copy()
            bad[k] = value
            with pytest.raises(AssertionError, match="jerks"):
                check(a, bad, "row k of j")
        # a jerk a few bounds off (a term rounded far more coarsely than f64)
        bad = j.copy()
        bad[(k + 7) % n] += 4 * RJP * float(ref[2][(k + 7) % n]) * np.array([1.0, 0.0, 0.0])
        with pytest.raises(AssertionError, match="jerks"):
            check(a, bad, "slightly off")
