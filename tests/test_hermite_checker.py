"""The Hermite tests' own yardsticks (tests/hermite_ref.py), checked without a GPU: the per-row bounds see a faulty pair,
hermite_step is fourth order, strict_aj agrees with the longdouble sum, and the mirror declares the new entry points."""
import numpy as np
import pytest

import hermite_ref as hr


@pytest.fixture(scope="module")
def w256():
    x, v, m = hr.world(256)
    rows = np.arange(256)
    return x, v, m, hr.direct_aj(x, v, m, hr.G, hr.EPS, rows)


def pair_terms(x, v, m, g, eps):
    """[n, n, 3] terms of a and of j (row i, partner j; zero on the diagonal), longdouble."""
    L = np.longdouble
    p, u, mm = x.astype(L), v.astype(L), m.astype(L)
    d = p[None] - p[:, None]
    w = u[None] - u[:, None]
    q = (d * d).sum(-1) + L(eps) * L(eps)
    k = L(g) * mm[None, :] / (q * np.sqrt(q))
    np.fill_diagonal(k, 0)
    dw = (d * w).sum(-1)
    return d * k[..., None], (w - (3 * dw / q)[..., None] * d) * k[..., None]


def test_committed_bounds_are_admissible():
    assert 0 < hr.RJ <= 1e-12
    assert 0 < hr.R <= 1e-12


def test_a_single_faulty_pair_is_far_above_the_bounds(w256):
    """Dropping (1 term), doubling (1 term) or sign-flipping (2 terms) any single pair moves its row by at least one whole
    term: the smallest term of world(256) is >= 1e-7 T_j for the jerk and >= 1e-5 T_a for the acceleration."""
    x, v, m, (Sa, Ta, Sj, Tj) = w256
    ta, tj = pair_terms(x, v, m, hr.G, hr.EPS)
    off = ~np.eye(256, dtype=bool)
    ra = np.sqrt((ta * ta).sum(-1)) / Ta[:, None]
    rj = np.sqrt((tj * tj).sum(-1)) / Tj[:, None]
    print(f"\n[hermite checker] smallest single term: {float(rj[off].min()):.2e} T_j, {float(ra[off].min()):.2e} T_a")
    assert rj[off].min() >= 1e-7 and ra[off].min() >= 1e-5
    assert rj[off].min() > 1e4 * hr.RJ and ra[off].min() > 1e4 * hr.R
    # ... and the bound check itself reports such a row: drop / double / flip pair (17, 200) of the true sums
    for factor in (0.0, 2.0, -1.0):
        bad_j = Sj.copy()
        bad_j[17] += (factor - 1) * tj[17, 200]
        err = np.sqrt(((bad_j - Sj) ** 2).sum(1)) / Tj
        assert err[17] > hr.RJ and (np.delete(err, 17) == 0).all()
        bad_a = Sa.copy()
        bad_a[17] += (factor - 1) * ta[17, 200]
        err = np.sqrt(((bad_a - Sa) ** 2).sum(1)) / Ta
        assert err[17] > hr.R


def test_strict_restatement_agrees_with_the_longdouble_sum(w256):
    x, v, m, (Sa, Ta, Sj, Tj) = w256
    a, j = hr.strict_aj(x, v, m, hr.G, hr.EPS)
    ea = np.sqrt(((a.astype(np.longdouble) - Sa) ** 2).sum(1)) / Ta
    ej = np.sqrt(((j.astype(np.longdouble) - Sj) ** 2).sum(1)) / Tj
    assert ea.max() < 1e-14 and ej.max() < 1e-14
    # the sums of the terms (no triangle slack possible): T bounds |S|
    assert (np.sqrt((Sa ** 2).sum(1)) <= Ta).all() and (np.sqrt((Sj ** 2).sum(1)) <= Tj).all()


def test_strict_aj_degenerate_worlds():
    for n in (0, 1):
        x, v, m = hr.world(n)
        a, j = hr.strict_aj(x, v, m, hr.G, hr.EPS)
        assert a.shape == (n, 3) and not a.any() and not j.any()
        assert hr.suggest_dt(a, j, 0.02) == float("inf")


def run(x, v, m, steps, T=0.5):
    s = hr.start(x, v, m, force=hr.fast_aj)
    for _ in range(steps):
        s = hr.hermite_step(s, T / steps, force=hr.fast_aj)
    return s


def test_hermite_step_is_fourth_order():
    """Max position error against a 1024-step run over T = 0.5 on world(64): the ratio from 64 to 128 steps is within
    [12, 24] around the 16 of a fourth-order scheme."""
    x, v, m = hr.world(64)
    ref = run(x, v, m, 1024)[0]
    e64 = np.abs(run(x, v, m, 64)[0] - ref).max()
    e128 = np.abs(run(x, v, m, 128)[0] - ref).max()
    print(f"\n[hermite checker] position error 64 steps {e64:.3e}, 128 steps {e128:.3e}, ratio {e64 / e128:.2f}")
    assert 12.0 <= e64 / e128 <= 24.0


def test_retain_drops_in_order_and_keeps_the_held_derivatives():
    x, v, m = hr.world(16)
    x[5] = (31.9, 0.0, 0.0)
    v[5] = (100.0, 0.0, 0.0)      # through the wall at +32 within one step of 1/128
    s0 = hr.start(x, v, m)
    s1 = hr.hermite_step(s0, 1.0 / 128)
    assert len(s1[0]) == 15
    full = hr.hermite_step(s0, 1.0 / 128, box=((0.0, 0.0, 0.0), 1e6))
    keep = np.delete(np.arange(16), 5)
    for got, want in zip(s1, full):
        assert np.array_equal(got, want[keep])
    # a NaN position is outside; walls are inclusive
    pts = np.array([[32.0, -32.0, 0.0], [np.nan, 0.0, 0.0], [32.0000001, 0.0, 0.0]])
    assert hr.contains(pts, *hr.BOX).tolist() == [True, False, False]


def test_mirror_declares_the_entry_points(nb):
    names = {"nbody_set_integrator", "nbody_get_integrator", "nbody_download_jerk", "nbody_suggest_dt"}
    assert names <= set(nb.DECLARED_SYMBOLS)
    assert (nb.LEAPFROG, nb.HERMITE4) == (0, 1)
    for name in names:
        assert hasattr(nb.lib, name)
    assert all(hasattr(nb.Simulation, k) for k in ("integrator", "jerk", "suggest_dt"))
