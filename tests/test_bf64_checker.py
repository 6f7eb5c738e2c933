"""The f64 bound of tests/bf64_bound.py, on the CPU: the oracle's f64 bf_update_forces (the reference's loop in double)
passes it, and each single corruption of one body a kernel could make -- a pair dropped, doubled or applied with the
wrong sign, the partner's mass taken for the body's own, two bodies' results swapped -- fails it."""
import numpy as np
import pytest

from bf64_bound import PROBE64, check_bound, direct_rows
from bf_probe import PROBE_G, check_probe, probe_columns, probe_records, set_probe

SD = dict(g=1.25, g_soft=1e-2, dt=1e-3, theta2=0.5)


def world(nb, orc, n, seed, eps=SD["g_soft"]):
    rec = nb.plummer(n, seed=seed, f64=True).astype(orc.P64)
    rec["mass"] *= np.random.default_rng(seed).uniform(0.5, 1.5, n)
    orc.bf_update_forces(rec, dict(SD, g_soft=eps))
    return rec


@pytest.mark.parametrize("n,eps", [(2, 0.0), (65, 0.0), (700, 1e-2), (2000, 1e-2)])
def test_oracle_passes_the_bound(nb, orc, n, eps):
    rec = world(nb, orc, n, seed=n, eps=eps)
    # (the oracle's sequential sum in f64 reaches ~3e-15 at 2 000 bodies: the same order as the fast kernels)
    check_bound(rec["acceleration"], rec["position"], rec["mass"], SD["g"], eps, what="oracle")


def pair_term(rec, i, j, g, eps, mass=None):
    d = rec["position"][j] - rec["position"][i]
    r2 = float(d @ d) + eps * eps
    return g * (rec["mass"][j] if mass is None else mass) * d / (r2 * np.sqrt(r2))


@pytest.mark.parametrize("n", [300, 2000])
def test_single_corruptions_fail_the_bound(nb, orc, n):
    eps, g = SD["g_soft"], SD["g"]
    rec = world(nb, orc, n, seed=7 + n)
    acc, pos, mass = rec["acceleration"].astype(np.float64), rec["position"], rec["mass"]
    rng = np.random.default_rng(n)
    for i in rng.choice(n, size=4, replace=False):
        S, T = direct_rows(pos, mass, g, eps, [i])
        # the partner whose term is smallest: the hardest pair to see
        terms = np.array([np.linalg.norm(pair_term(rec, i, j, g, eps)) if j != i else np.inf for j in range(n)])
        j = int(np.argmin(terms))
        t = pair_term(rec, i, j, g, eps)
        bad = {"dropped": acc[i] - t, "doubled": acc[i] + t, "wrong sign": acc[i] - 2 * t,
               "partner's mass": acc[i] - t + pair_term(rec, i, j, g, eps, mass=mass[i])}
        for name, row in bad.items():
            a = acc.copy()
            a[i] = row
            with pytest.raises(AssertionError):
                check_bound(a, pos, mass, g, eps, rows=[i], what=name)
        k = (i + 1 + int(rng.integers(n - 1))) % n
        a = acc.copy()
        a[[i, k]] = a[[k, i]]
        with pytest.raises(AssertionError):
            check_bound(a, pos, mass, g, eps, rows=[i, k], what="swapped")


def test_probe64_bound_holds_for_the_oracle_and_rejects_one_term(nb, orc):
    """PROBE64 on a probe world of PARTICLE_DTYPE64 records (f32-representable positions): the f64 oracle passes, a term
    off by more than PROBE64 does not."""
    n = 700
    pos = nb.plummer(n, seed=3)["position"].astype(np.float64)
    for k in probe_columns(n, set_sizes=(256,), n_random=4, every_below=0)[:12]:
        rec = set_probe(probe_records(orc.P64, pos), k)
        orc.bf_update_forces(rec, dict(SD, g=PROBE_G, g_soft=0.0))
        acc = rec["acceleration"].astype(np.float64)
        assert check_probe(acc, pos, k, PROBE_G, 0.0, rtol=PROBE64, what="oracle") < PROBE64 / 4
        i = (k + 1) % n
        acc[i] *= 1.0 + 4 * PROBE64
        with pytest.raises(AssertionError):
            check_probe(acc, pos, k, PROBE_G, 0.0, rtol=PROBE64, what="off")
