"""What the tracer GPU tests rest on, checked on the CPU: the plan of the fast tracer pass (host-only entry), the strict
restatement against the oracle on the zero-mass-appended world, and the fast bound's power to see a single pair."""
import numpy as np
import pytest

import tracer_ref
from bf_probe import PROBE_G, probe_records, set_probe


@pytest.mark.parametrize("n", [1, 2, 63, 65, 1025, 65536])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 5000, 2 ** 20])
def test_host_tracer_plan_covers(nb, m, n):
    p = nb.host_tracer_plan(m, n)
    ipt, groups, K, length = p["tracers_per_lane"], p["groups"], p["slices"], p["slice_len"]
    assert ipt in (1, 2, 4) and groups >= 1 and K >= 1 and length >= 1
    # the groups cover [0, m) and none is wholly beyond it
    assert groups * 256 * ipt >= m > (groups - 1) * 256 * ipt
    # the slices tile [0, n): slice k = [k * length, min(n, (k + 1) * length)), no overlap by construction, none empty
    lo = [k * length for k in range(K)]
    hi = [min(n, (k + 1) * length) for k in range(K)]
    assert lo[0] == 0 and hi[-1] == n
    assert all(hi[k] == lo[k + 1] for k in range(K - 1))
    if n >= K:
        assert all(h > l for l, h in zip(lo, hi))


@pytest.mark.parametrize("g_soft", [0.0, 0.01])
def test_strict_restatement_is_the_oracle_on_the_appended_world(nb, orc, g_soft):
    n, m = 64, 65
    bodies = nb.plummer(n, seed=11).astype(orc.P32)
    rng = np.random.default_rng(5)
    tracers = np.zeros(m, orc.P32)
    tracers["position"] = rng.uniform(-2, 2, (m, 3))
    st = dict(g=1.25, g_soft=g_soft, dt=1e-3, theta2=0.5)
    world = tracer_ref.with_zero_mass(bodies, tracers)
    orc.bf_update_forces(world, st)
    ref_b, ref_t = tracer_ref.split_back(world)
    assert len(ref_b) == n and len(ref_t) == m
    got = tracer_ref.strict_tracer_acc(bodies, tracers["position"], st["g"], g_soft)
    assert np.array_equal(got.view(np.uint32), ref_t["acceleration"].view(np.uint32))
    # and the bodies do not feel the appended records
    alone = bodies.copy()
    orc.bf_update_forces(alone, st)
    assert np.array_equal(alone["acceleration"].view(np.uint32), ref_b["acceleration"].view(np.uint32))


def test_bound_flags_a_dropped_and_a_doubled_term(nb, orc):
    """Probe world: every body mass 0 except body k's, so a tracer's sum is one term."""
    n, m, k = 1500, 7, 700
    pos = nb.plummer(n, seed=3)["position"]
    tpos = np.random.default_rng(9).uniform(-1, 1, (m, 3)).astype(np.float32)
    bodies = set_probe(probe_records(orc.P32, pos), k)
    S, T = tracer_ref.pair_sums(bodies, tpos, PROBE_G, 0.01)
    good = (np.longdouble(np.float32(PROBE_G)) * S).astype(np.float32)
    assert tracer_ref.check_fast(good, S, T, n, PROBE_G, "exact sums") <= 1.0
    for name, f in (("dropped", 0.0), ("doubled", 2.0)):
        bad = good.copy()
        bad[3] *= np.float32(f)
        with pytest.raises(AssertionError):
            tracer_ref.check_fast(bad, S, T, n, PROBE_G, name)
    # T == 0 demands an exact zero
    empty = probe_records(orc.P32, pos)
    S, T = tracer_ref.pair_sums(empty, tpos, PROBE_G, 0.01)
    assert (T == 0).all()
    assert tracer_ref.check_fast(np.zeros((m, 3), np.float32), S, T, n, PROBE_G) == 0.0
    with pytest.raises(AssertionError):
        tracer_ref.check_fast(np.full((m, 3), 1e-30, np.float32), S, T, n, PROBE_G)
