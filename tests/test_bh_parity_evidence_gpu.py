"""Fast-math Barnes-Hut against the oracle, PER BODY: every body's acceleration error relative to its OWN |a| (the other
tests bound the error by the largest acceleration of the field, which a halo body whose acceleration is 100x below the
core's passes while being off by 1e-3 of itself).  Both tree builds, both leaf rules, at the size the metric is quoted on
(configs[2], 65 536 bodies) and at 2^20; the figures are printed (pytest -s) and bounded.
Reference: src/manual/barnes_hut.rs:185-203 (leaf rule REFERENCE), src/llm/barnes_hut.rs:915-997 (DIRECT), restated in oracle/.

What the bounds say:
  * host-built tree (bit-equal to the oracle's): every lane evaluates exactly the oracle's opening tests (node counts are
    asserted equal), so the error is rounding only -- v_rsq_f32 + FMA per term, one running f32 sum per node-range segment
    instead of the reference's nested sums: a few 1e-7 of |a| in the median, and below 1e-4 of |a| for EVERY body (the largest
    relative errors belong to bodies near the centre whose partial forces cancel: |a| is small against the sum of |terms|);
  * device-built tree: same cells and links, centres of mass from f64 prefix sums instead of the reference's sequential
    f32 folds (they differ by the fold's own rounding, n * 2^-24): an opening test that sits on its threshold can flip, and
    the body concerned then differs by the truncation error of ONE cell (monopole against its children).  So: the same
    median, and a handful of bodies (asserted: < 1 in 2 000) beyond 1e-5 of their own |a|, none beyond 5e-3.
Measured (round 3, Plummer seed 20250523, theta = 0.5, g_soft = 0.01; median / 99.9th percentile / max of |da|/|a|, bodies beyond 1e-5):
  65 536  host   REFERENCE 1.1e-7 / 1.3e-6 / 4.8e-6,   0     DIRECT 5.2e-7 / 3.9e-6 / 1.8e-5,   6
  65 536  device REFERENCE 1.3e-7 / 1.4e-6 / 8.9e-6,   0     DIRECT 5.2e-7 / 4.0e-6 / 1.7e-5,   6     (accepted nodes: +7 of 1.0e8)
  2^20    host   REFERENCE 5.9e-7 / 4.4e-6 / 3.7e-5, 109     DIRECT 7.7e-8 / 6.5e-7 / 4.0e-6,   0
  2^20    device REFERENCE 6.2e-7 / 4.7e-6 / 4.9e-4, 217     DIRECT 2.5e-7 / 1.6e-6 / 4.8e-4, 120     (accepted nodes: -46 of 2.1e9)
At 2^20 with the device tree one flipped test near the core moves a body by 2e-4 of the FIELD's largest acceleration: "<= 1e-5 of
max|a|" holds for the host tree at every size and for the device tree at 65 536, not for the device tree at 2^20.
SURVEY section 8(d)'s criterion, relative L2 over the field ||a - a_oracle||_2 / ||a_oracle||_2 <= 1e-5, holds in every case and is
asserted; measured on an MI355X (same seed, theta2 = 0.25): 1.4e-7 to 8.7e-7 on the host tree, 1.5e-7 to 7.4e-7 on the device tree at
65 536 bodies and 1.0e-6 (REFERENCE) / 1.3e-6 (DIRECT) on the device tree at 2^20."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
_oracle_cache = {}


def oracle_acc(nb, orc, n, leaf):
    key = (n, leaf)
    if key not in _oracle_cache:
        sd = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
        ref = nb.plummer(n, seed=20250523).astype(orc.P32)
        acc_n, vis_n = orc.bh_update_forces(ref, sd, BOX[0], BOX[1], threads=16, leaf_mode=1 if leaf == "direct" else 0)
        _oracle_cache[key] = (ref["acceleration"].astype(np.float64), acc_n, vis_n)
    return _oracle_cache[key]


@pytest.mark.parametrize("n", [65536, 1 << 20])
@pytest.mark.parametrize("leaf", ["reference", "direct"])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_fast_walk_error_relative_to_each_bodys_own_acceleration(gpu, orc, n, leaf, tree):
    nb = gpu
    ref, acc_n, vis_n = oracle_acc(nb, orc, n, leaf)
    ics = nb.plummer(n, seed=20250523)
    with nb.Simulation(ics, *BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE if tree == "device" else nb.TREE_HOST,
                       leaf_mode=nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE) as sim:
        sim.settings = nb.Settings(1.0, 0.01, 1e-3, 0.25)
        sim.update_forces()
        got = sim.get_points()["acceleration"].astype(np.float64)
        s = sim.stats()
    own = np.linalg.norm(ref, axis=1)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(own, 1e-30)
    med, p999, worst = float(np.median(err)), float(np.quantile(err, 0.999)), float(err.max())
    beyond5, beyond3 = int(np.count_nonzero(err > 1e-5)), int(np.count_nonzero(err > 1e-3))
    field = float(np.abs(got - ref).max() / np.abs(ref).max())
    l2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"\nbh fast parity n={n} tree={tree} leaf={leaf}: per-body |da|/|a| median {med:.2e} p99.9 {p999:.2e} max {worst:.2e}; "
          f"bodies beyond 1e-5: {beyond5}, beyond 1e-3: {beyond3}; max|da|/max|a| {field:.2e}; L2 {l2:.2e}; "
          f"accepted {s.interactions} (oracle {acc_n}), visited {s.node_visits} (oracle {vis_n})")
    assert own.min() > 0
    assert med < 1e-6 and p999 < 2e-5 and beyond3 == 0
    assert l2 <= 1e-5
    if tree == "host":   # the oracle's tree bit for bit: the same opening tests, rounding only
        assert (s.interactions, s.node_visits) == (acc_n, vis_n)
        assert worst < 1e-4 and field < 1e-5
    else:                # centres of mass to the fold's rounding: a threshold test may flip, one cell's truncation error each
        assert abs(s.interactions - acc_n) <= 1e-6 * acc_n and abs(s.node_visits - vis_n) <= 1e-6 * vis_n
        assert beyond5 <= max(8, n // 2000) and worst < 5e-3
        assert field < (1e-5 if n <= 65536 else 1e-3)
