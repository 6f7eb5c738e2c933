"""The probe checker of tests/bf_probe.py, on the CPU: the f32 oracle passes it, and the errors a kernel makes at a
boundary (one pair dropped, doubled or sent with the wrong sign) fail it -- while the full-sum tolerances of the fast
kernels' tests (1e-5 or 3e-5 of max |a|, 1e-4 per body) still accept the same errors in 20 000- and 65 536-body
Plummer spheres."""
import numpy as np
import pytest

from bf_probe import PROBE_G, PROBE_RTOL, check_probe, probe_columns, probe_records, set_probe
from conftest import rel_err


def probe_oracle(nb, orc, pos, k, eps):
    rec = set_probe(probe_records(orc.P32, pos), k)
    orc.bf_update_forces_rows(rec, dict(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5), threads=2)
    return rec["acceleration"].astype(np.float64)


def corruptions(acc, i):
    """(name, accelerations with body i's only term dropped / doubled / of the wrong sign)."""
    out = []
    for name, f in (("dropped", 0.0), ("doubled", 2.0), ("wrong sign", -1.0)):
        a = acc.copy()
        a[i] *= f
        out.append((name, a))
    return out


@pytest.mark.parametrize("n,eps", [(1, 0.0), (2, 0.0), (65, 0.0), (300, 1e-2), (1500, 0.0)])
def test_oracle_passes_the_probe(nb, orc, n, eps):
    pos = nb.plummer(n, seed=n)["position"]
    worst = 0.0
    for k in probe_columns(n, set_sizes=(256, 512), n_random=8, every_below=80):
        worst = max(worst, check_probe(probe_oracle(nb, orc, pos, k, eps), pos, k, PROBE_G, eps, what="oracle"))
    assert worst < PROBE_RTOL / 4


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_probe_rejects_single_pair_errors(nb, orc, eps):
    n = 1500
    pos = nb.plummer(n, seed=7)["position"]
    for k in (0, 511, 512, n - 1):
        acc = probe_oracle(nb, orc, pos, k, eps)
        for i in (k - 1, (k + 1) % n):
            i %= n
            for name, bad in corruptions(acc, i):
                with pytest.raises(AssertionError):
                    check_probe(bad, pos, k, PROBE_G, eps, what=name)
        # the self pair (0 * inf at eps = 0) or any term landing on the probe body itself
        bad = acc.copy()
        bad[k] = acc[(k + 1) % n]
        with pytest.raises(AssertionError):
            check_probe(bad, pos, k, PROBE_G, eps, what="self")
        bad[k] = np.nan
        with pytest.raises(AssertionError):
            check_probe(bad, pos, k, PROBE_G, eps, what="nan")
        # a pair counted with the probe mass twice over (one of the two masses of a symmetric update mixed up)
        bad = acc * 1.0
        bad[(k + 7) % n] *= 1.0 + 4 * PROBE_RTOL
        with pytest.raises(AssertionError):
            check_probe(bad, pos, k, PROBE_G, eps, what="slightly off")


@pytest.mark.parametrize("n,seed,radius_q,whole_bound,kinds", [
    (20000, 20000, 0.9, 1e-5, ("dropped", "doubled")),                  # test_bf_gpu.py: 1e-5 of max |a|, 1e-4 per body
    (65536, 5, 0.5, 3e-5, ("dropped", "doubled", "wrong sign")),      # test_sharded_gpu.py at 65 536 bodies: 3e-5
])
def test_full_sum_tolerance_misses_what_the_probe_catches(nb, orc, n, seed, radius_q, whole_bound, kinds):
    """At sizes the fast kernels' tests use (Plummer, eps = 1e-2), drop, double or flip the sign of one typical pair
    (the partner of median share, not a nearest neighbour) of one body: the existing per-body (1e-4) and whole-field
    bounds accept it, the probe of the same pair rejects it.  (At 20 000 bodies the whole-field bound does see a median
    pair of a body inside the half-mass radius, ~3e-5 of max |a|; it misses one of the outer tenth's bodies, and the
    per-body bound misses both.  At 65 536 a median pair of a median body is ~1.5e-5 of its acceleration.)"""
    eps = 1e-2
    sd = dict(g=1.0, g_soft=eps, dt=1e-3, theta2=0.5)
    ics = nb.plummer(n, seed=seed)
    pos64 = ics["position"].astype(np.float64)
    r = np.linalg.norm(pos64, axis=1)
    i = int(np.argsort(r)[int(radius_q * n)])
    # the rows the bounds look at: body i and the 64 bodies nearest the radius where a Plummer sphere's acceleration
    # peaks, which bound max |a| from below (the whole-field check here is then stricter than the real one); the
    # oracle computes rows [0, m) of a reordered copy
    rows = [i] + [int(j) for j in np.argsort(np.abs(r - 0.45))[:64] if j != i]
    order = np.concatenate([rows, np.setdiff1d(np.arange(n), rows)])
    rec = ics[order].copy().astype(orc.P32)
    orc.bf_update_forces_range(rec, sd, 0, len(rows), threads=4)
    ref = rec["acceleration"][: len(rows)].astype(np.float64)
    # the pair terms of body i (f64); a typical partner: the median share
    d = pos64 - pos64[i]
    r2 = (d * d).sum(1) + float(np.float32(eps)) ** 2
    r2[i] = np.inf
    term = ics["mass"].astype(np.float64)[:, None] * d / (r2 * np.sqrt(r2))[:, None]
    share = np.linalg.norm(term, axis=1) / np.linalg.norm(ref[0])
    share[i] = np.nan
    j = int(np.nanargmin(np.abs(share - np.nanmedian(share))))
    assert share[j] < 1e-4 / 2 and j != int(np.nanargmax(share))
    deltas = {"dropped": -term[j], "doubled": term[j], "wrong sign": -2 * term[j]}
    for name in kinds:
        got = ref.copy()
        got[0] += deltas[name]
        per_body = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
        assert per_body.max() < 1e-4, name                   # the existing per-body bound accepts it ...
        assert rel_err(got, ref) < whole_bound, name         # ... and so does the whole-field one
    # the probe of column j: the same errors of the pair (j -> i) are O(1).  Massless bodies act on nothing, so the
    # probe world restricted to bodies j, i and a few hundred others gives those bodies the same accelerations.
    sub = np.concatenate([[j, i], np.setdiff1d(np.arange(0, n, n // 254), [i, j])])
    pos = ics["position"][sub]
    acc = probe_oracle(nb, orc, pos, 0, eps)
    check_probe(acc, pos, 0, PROBE_G, eps, what="oracle")
    for name, bad in corruptions(acc, 1):
        with pytest.raises(AssertionError):
            check_probe(bad, pos, 0, PROBE_G, eps, what=name)


def test_probe_columns_rule():
    assert probe_columns(5) == [0, 1, 2, 3, 4]
    cols = probe_columns(4097, set_sizes=(256,), n_random=0)
    assert {0, 1, 63, 64, 255, 256, 511, 512, 4095, 4096} <= set(cols)
    assert {3839, 3840, 4095} <= set(cols) and all(0 <= c < 4097 for c in cols)
    # sharded: every block's ends, its set boundaries counted from the block's start, extra block offsets
    cols = set(probe_columns(6001, blocks=[(0, 3001), (3001, 6001)], set_sizes=(512,), offsets=(1536,), n_random=0))
    assert {0, 3000, 3001, 6000, 511, 512, 3001 + 511, 3001 + 512, 1535, 1536, 3001 + 1536, 2560, 3001 + 2560} <= cols
    assert len(probe_columns(33000, set_sizes=(512,), n_random=24)) < 200
    assert probe_columns(3000, n_random=24, seed=3) == probe_columns(3000, n_random=24, seed=3)
