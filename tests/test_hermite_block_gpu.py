"""Block individual time steps of a Hermite handle (nbody_set_block_steps; kernels_hermite.hip k_hmb_*, k_hm_act, k_hm_act_strict).

Strict math: whole macro steps bit for bit beside tests/hermite_block_ref.py (levels, counters and the retain included), and
the shared step as the eta -> infinity limit.  Fast math: every row of the active-set kernels within the per-row bounds over
every shape of the id list and the slice count, trajectories beside a strict handle (same levels, same schedule),
determinism, clone, steps(k), and the accuracy bought per pair term.  Then the refusals and the validity of the levels.
Prints its figures under pytest -s."""
import numpy as np
import pytest

import hermite_block_ref as br
import hermite_ref as hr
from bf64_bound import bound_errors

pytestmark = pytest.mark.gpu
G_SOFT = 0.005
ETA, L = 0.02, 6
MACRO = [1 / 16, 1 / 16, -1 / 16, 1 / 32]


def eq(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make(nb, x, v, m, math, block=(ETA, L), eps=G_SOFT, dt=1 / 16, hermite=True, box=hr.BOX, **tuning):
    sim = nb.Simulation(hr.records(nb.PARTICLE_DTYPE64, x, v, m), *box, method=nb.BRUTE_FORCE, math_mode=math, f64=True, tuning=tuning)
    sim.settings = nb.Settings(g=hr.G, g_soft=eps, dt=dt, theta2=0.5)
    if hermite:
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
    return sim


def state_of(sim):
    p = sim.get_points()
    return p["position"], p["velocity"], p["acceleration"], sim.jerk(), p["mass"]


def same_state(got, want):
    return all(eq(g, w) for g, w in zip(got, want))


def refused(nb, call, needle="nbody_"):
    with pytest.raises(nb.NbodyError) as e:
        call()
    assert e.value.code == nb.NBODY_ERR_INVALID and needle in str(e.value), str(e.value)


def trajectory_world(leaver):
    x, v, m = br.tight_pair_world(130)
    if leaver:   # 31.5 + 6 / 16 = 31.875 is inside, 31.5 + 2 * 6 / 16 = 32.25 is not: out during the second macro step
        x = np.insert(x, 100, (31.5, 0.3, -0.2), axis=0)
        v = np.insert(v, 100, (6.0, 0.0, 0.0), axis=0)
        m = np.insert(m, 100, 1.0 / 256)
    return x, v, m


_runs = {}


def reference_run(leaver):
    """The restatement's run over MACRO, computed once: [(state, levels, counters ...) after every macro step], the log."""
    if leaver not in _runs:
        x, v, m = trajectory_world(leaver)
        h = br.Handle(x, v, m, ETA, L, eps=G_SOFT)
        snaps = []
        for dt in MACRO:
            h.step_by(dt)
            snaps.append((h.state, h.levels.copy(), h.log["block_steps"], h.log["updates"], h.interactions, h.elapsed))
        _runs[leaver] = (snaps, h.log)
    return _runs[leaver]


# ---------------------------------------------------------------------------------------------- 1. strict trajectory
@pytest.mark.parametrize("leaver", [False, True])
def test_strict_macro_steps_bit_for_bit(gpu, leaver):
    nb = gpu
    x, v, m = trajectory_world(leaver)
    snaps, log = reference_run(leaver)
    assert log["all_at_T"] and log["off_grid"] == 0
    with make(nb, x, v, m, nb.STRICT) as sim:
        assert sim.block_steps == (ETA, L)
        for k, (dt, (state, levels, bsteps, updates, inter, elapsed)) in enumerate(zip(MACRO, snaps)):
            sim.step_by(dt)
            assert same_state(state_of(sim), state), f"macro step {k + 1}"
            assert np.array_equal(sim.levels(), levels), f"macro step {k + 1}"
            assert sim.block_step_counts() == (bsteps, updates), f"macro step {k + 1}"
            assert sim.stats().interactions == inter and sim.elapsed() == elapsed, f"macro step {k + 1}"
            assert len(sim) == len(x) - (1 if leaver and k >= 1 else 0)
        assert sim.stats().steps == len(MACRO)
        print(f"\n[hermite block] strict n={len(x)}: {bsteps} block steps, {updates} body updates, levels up to {levels.max()}")
        assert levels.max() >= 3 and bsteps > len(MACRO)       # the pair does step below the field


def test_strict_levels_move_with_their_bodies_across_a_tile_boundary(gpu):
    """The retain with the block-step levels as a fifth array, over two tiles: 1 100 bodies, a box of width 2.4 that about an
    eighth of the bodies on either side of index 1 024 are outside of at the end of the first macro step (the restatement's
    mask is asserted to say so).  The second macro step has the same |dt|, so it runs on the levels that were moved.
    (The restatement takes about 4.5 s a macro step at this size.)"""
    nb = gpu
    x, v, m = br.tight_pair_world(1100)
    box = ((0.0, 0.0, 0.0), 2.4)
    ref = br.Handle(x, v, m, ETA, L, eps=G_SOFT, box=box)
    ref.update_forces()
    unbounded, _ = br.macro_step(ref.state, None, 1 / 16, ETA, L, eps=G_SOFT, box=((0.0, 0.0, 0.0), np.inf))
    keep = hr.contains(unbounded[0], *box)
    for part in (keep[:1024], keep[1024:]):
        assert part.any() and not part.all(), "needs leavers and survivors on both sides of index 1 024"
    with make(nb, x, v, m, nb.STRICT, box=box) as sim:
        for k in range(2):
            sim.step_by(1 / 16)
            ref.step_by(1 / 16)
            assert len(sim) == len(ref.levels) == (int(keep.sum()) if k == 0 else len(sim)), f"macro step {k + 1}"
            assert same_state(state_of(sim), ref.state), f"macro step {k + 1}"
            assert np.array_equal(sim.levels(), ref.levels), f"macro step {k + 1}"
            assert sim.block_step_counts() == (ref.log["block_steps"], ref.log["updates"]), f"macro step {k + 1}"
            assert sim.stats().interactions == ref.interactions and sim.elapsed() == ref.elapsed, f"macro step {k + 1}"
            if k == 0:   # the survivors from beyond index 1 024 are the last ones now, and they differ in level
                assert len(np.unique(ref.levels[-int(keep[1024:].sum()):])) >= 3
        assert ref.log["all_at_T"] and ref.log["off_grid"] == 0


# ---------------------------------------------------------------------------------------------- 2. eta -> infinity
def test_strict_huge_eta_gives_the_shared_steps_bits(gpu):
    nb = gpu
    x, v, m = br.tight_pair_world(130)
    with make(nb, x, v, m, nb.STRICT, block=(1e30, L)) as blk, make(nb, x, v, m, nb.STRICT, block=None) as shared:
        for k, dt in enumerate((1 / 64, 1 / 64, -1 / 128)):
            blk.step_by(dt)
            shared.step_by(dt)
            assert same_state(state_of(blk), state_of(shared)), f"step {k + 1}"
            assert not blk.levels().any()
        assert blk.block_step_counts() == (3, 390) and shared.block_step_counts() == (0, 0)
        assert blk.stats().interactions == shared.stats().interactions == 4 * 130 * 129


# ---------------------------------------------------------------------------------------------- 3. fast, per row
def id_lists(n):
    rng = np.random.default_rng(n)
    lists = {"first": [0], "last": [n - 1], "all": np.arange(n), "shuffled half": rng.permutation(n)[: max(1, n // 2)]}
    for k in (63, 64, 65):
        if k <= n:
            lists[f"{k} ids"] = np.sort(rng.permutation(n)[:k])
    return lists


@pytest.mark.parametrize("n", [1, 2, 65, 257, 1500])
def test_forces_of_listed_bodies_every_row(gpu, n):
    nb = gpu
    x, v, m = hr.world(n)
    every = np.arange(n)
    Sa, Ta, Sj, Tj = hr.direct_aj(x, v, m, hr.G, hr.EPS, every)
    sa, sj = br.strict_rows(x, v, m, hr.G, hr.EPS, every)        # (a row's sum does not depend on which other rows are listed)
    worst_a = worst_j = 0.0
    for tuning in (dict(bf64_waves=64), {}):
        with make(nb, x, v, m, nb.FAST, block=None, eps=hr.EPS, **tuning) as sim:
            before = state_of_xv(sim)
            for name, ids in id_lists(n).items():
                ids = np.asarray(ids)
                a, j = sim.hermite_forces_of(ids)
                ea, ej = bound_errors(a, Sa[ids], Ta[ids]), bound_errors(j, Sj[ids], Tj[ids])
                worst_a, worst_j = max(worst_a, ea.max()), max(worst_j, ej.max())
                assert ea.max() <= hr.R, (name, tuning, ids[~(ea <= hr.R)][:8], ea.max())
                assert ej.max() <= hr.RJ, (name, tuning, ids[~(ej <= hr.RJ)][:8], ej.max())
                a2, j2 = sim.hermite_forces_of(ids)
                assert eq(a, a2) and eq(j, j2), (name, "the same input gives the same bits")
            assert sim.stats().interactions == 0 and sim.block_step_counts() == (0, 0)
            assert all(eq(p, q) for p, q in zip(before, state_of_xv(sim)))
            refused(nb, lambda: sim.hermite_forces_of([0, 0]), "nbody_debug_hermite_forces_of")
            refused(nb, lambda: sim.hermite_forces_of([n]), "nbody_debug_hermite_forces_of")
            refused(nb, lambda: sim.hermite_forces_of([-1]), "nbody_debug_hermite_forces_of")
    print(f"\n[hermite block] k_hm_act n={n}: worst |a - S_a| / T_a {worst_a:.3e}, |j - S_j| / T_j {worst_j:.3e}")
    with make(nb, x, v, m, nb.STRICT, block=None, eps=hr.EPS) as sim:
        for name, ids in id_lists(n).items():
            ids = np.asarray(ids)
            a, j = sim.hermite_forces_of(ids)
            assert eq(a, sa[ids]) and eq(j, sj[ids]), name
        refused(nb, lambda: sim.hermite_forces_of([0, 0]), "nbody_debug_hermite_forces_of")
        refused(nb, lambda: sim.hermite_forces_of([n]), "nbody_debug_hermite_forces_of")
    if n == 1:
        assert not a.any() and not j.any()


def state_of_xv(sim):
    p = sim.get_points()
    return p["position"], p["velocity"]


# ---------------------------------------------------------------------------------------------- 4. fast trajectory
def test_fast_trajectory_beside_strict_repeat_clone_and_steps(gpu):
    nb = gpu
    x, v, m = trajectory_world(False)
    snaps, log = reference_run(False)
    # a fast handle's dtc differs from the strict one's in its last bits (1e-13 or so); it takes the same levels as long as
    # no dtc of the run comes that close to a threshold.  The world's seed is chosen so that none does.
    assert log["min_gap"] > 1e-6, log["min_gap"]
    with make(nb, x, v, m, nb.STRICT) as strict, make(nb, x, v, m, nb.FAST) as fast:
        for dt in MACRO:
            strict.step_by(dt)
            fast.step_by(dt)
            assert np.array_equal(fast.levels(), strict.levels())
            assert fast.block_step_counts() == strict.block_step_counts()
        assert fast.stats().interactions == strict.stats().interactions
        want, got = state_of(strict), state_of(fast)
        evals = fast.block_step_counts()[0] + 1
    # tests/test_hermite_gpu.py allows 1e-11 of the box width after 16 steps' 17 evaluations of F: the same per evaluation
    err = np.abs(got[0] - want[0]).max() / hr.BOX[1]
    print(f"\n[hermite block] fast beside strict after {evals} evaluations of F: position error {err:.3e} of the box width "
          f"(allowed {1e-11 * evals / 17:.3e}); smallest threshold distance of the run {log['min_gap']:.3e}")
    assert err <= 1e-11 * evals / 17
    with make(nb, x, v, m, nb.FAST) as sim:                # a second run repeats; a clone after one macro step ends like its source
        sim.step_by(MACRO[0])
        with sim.clone() as twin:
            assert twin.block_steps == (ETA, L) and np.array_equal(twin.levels(), sim.levels())
            for dt in MACRO[1:]:
                sim.step_by(dt)
                twin.step_by(dt)
            assert same_state(state_of(sim), got) and same_state(state_of(twin), got)
            assert np.array_equal(twin.levels(), sim.levels())
    with make(nb, x, v, m, nb.FAST) as a, make(nb, x, v, m, nb.FAST) as b:   # steps(3): the bits of three step_by calls
        a.steps(3)
        for _ in range(3):
            b.step_by(1 / 16)
        assert same_state(state_of(a), state_of(b)) and a.block_step_counts() == b.block_step_counts()
        assert a.stats().steps == 3 and a.elapsed() == b.elapsed()


# ---------------------------------------------------------------------------------------------- 5. accuracy for work
def test_fast_block_steps_buy_accuracy_for_work(gpu):
    """The proposal's table world (n = 64, L = 8, T = 1): against the handle's own shared-step run at 1/16 2^-6 the block run
    must spend less than a quarter of the pair terms and end with less than a tenth of the energy error (numpy: 6.05e5
    against 4.13e6 terms, 2.1e-6 against 5.9e-4)."""
    nb = gpu
    x, v, m = br.tight_pair_world(64)

    def run(block, dt, steps):
        with make(nb, x, v, m, nb.FAST, block=block, dt=dt) as sim:
            e0 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
            sim.steps(steps)
            e1 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
            return sim.stats().interactions, abs((e1 - e0) / e0), sim.block_step_counts()

    terms_b, err_b, counts = run((0.02, 8), 1 / 16, 16)
    terms_s, err_s, _ = run(None, 1 / 1024, 1024)
    print(f"\n[hermite block] T = 1, n = 64: block steps {terms_b} pair terms, energy error {err_b:.3e} ({counts[0]} block steps, "
          f"{counts[1]} body updates); shared step 1/1024 {terms_s} pair terms, energy error {err_s:.3e}")
    assert terms_b < terms_s / 4
    assert err_b < err_s / 10


# ---------------------------------------------------------------------------------------------- 6. semantics
def test_refusals_on_every_kind_of_handle_and_argument(gpu):
    nb = gpu
    x, v, m = hr.world(64)
    rec64 = hr.records(nb.PARTICLE_DTYPE64, x, v, m)
    rec32 = hr.records(nb.PARTICLE_DTYPE, x, v, m)
    others = [
        lambda: nb.Simulation(rec32, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST),
        lambda: nb.Simulation(rec64, *hr.BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, f64=True),
        lambda: nb.Simulation(rec64, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.STRICT, f64=True, rank=0, world_size=2),
        lambda: make(nb, x, v, m, nb.STRICT, hermite=False),          # a leapfrog handle that could run Hermite
    ]
    for ctor in others:
        with ctor() as sim:
            refused(nb, lambda: setattr(sim, "block_steps", (0.02, 6)), "nbody_set_block_steps")
            refused(nb, lambda: setattr(sim, "block_steps", (0.0, 0)), "nbody_set_block_steps")
            refused(nb, lambda: sim.block_steps, "nbody_get_block_steps")
            refused(nb, sim.levels, "nbody_download_levels")
            refused(nb, sim.block_step_counts, "nbody_block_step_counts")
            refused(nb, lambda: sim.hermite_forces_of([0]), "nbody_debug_hermite_forces_of")
    with make(nb, x, v, m, nb.FAST, block=None) as sim:
        assert sim.block_steps == (0.0, 0)
        for bad in [(0.0, 6), (-0.02, 6), (float("nan"), 6), (0.02, 0), (0.02, 21), (0.02, -1), (0.0, 3)]:
            refused(nb, lambda: setattr(sim, "block_steps", bad), "nbody_set_block_steps")
        assert sim.block_steps == (0.0, 0)
        refused(nb, sim.levels, "nbody_download_levels")           # block steps are off
        sim.block_steps = (0.02, 20)
        sim.block_steps = (0.0, 0)                                 # valid on any Hermite handle
        sim.block_steps = (0.02, 1)
        assert sim.block_steps == (0.02, 1)
        sim.integrator = nb.LEAPFROG                               # selecting the leapfrog switches them off
        refused(nb, lambda: sim.block_steps, "nbody_get_block_steps")
        sim.integrator = nb.HERMITE4
        assert sim.block_steps == (0.0, 0)


@pytest.mark.parametrize("math", ["strict", "fast"])
def test_levels_are_refused_while_stale_and_reassigned(gpu, math):
    nb = gpu
    mode = nb.STRICT if math == "strict" else nb.FAST
    x, v, m = br.tight_pair_world(40)
    with make(nb, x, v, m, mode, dt=1 / 32) as sim:
        refused(nb, sim.levels, "nbody_download_levels")           # stale after the upload
        sim.update_forces()                                        # F, and start levels for the settings' dt
        a, j = sim.get_points()["acceleration"], sim.jerk()
        assert np.array_equal(sim.levels(), br.start_levels(a, j, ETA, 1 / 32, L))
        assert sim.levels().max() > sim.levels().min()
        sim.block_steps = (ETA, L)                                 # nbody_set_block_steps makes them invalid again
        refused(nb, sim.levels, "nbody_download_levels")
        sim.update_forces()
        sim.settings = nb.Settings(g=hr.G, g_soft=G_SOFT, dt=1 / 32, theta2=0.5)
        refused(nb, sim.levels, "nbody_download_levels")           # wherever (a0, j0) are stale
        if math == "strict":                                       # a changed |dt| reassigns start levels: beside the restatement
            ref = br.Handle(x, v, m, ETA, L, eps=G_SOFT)
            for dt in (1 / 32, -1 / 32, 1 / 128):
                sim.step_by(dt)
                ref.step_by(dt)
                assert np.array_equal(sim.levels(), ref.levels) and same_state(state_of(sim), ref.state)
            a, j = ref.state[2], ref.state[3]
            sim.update_forces()
            assert np.array_equal(sim.levels(), br.start_levels(sim.get_points()["acceleration"], sim.jerk(), ETA, 1 / 32, L))


@pytest.mark.parametrize("math", ["strict", "fast"])
def test_on_then_off_leaves_no_trace_in_the_shared_step(gpu, math):
    nb = gpu
    mode = nb.STRICT if math == "strict" else nb.FAST
    x, v, m = br.tight_pair_world(130)
    runs = []
    for toggle in (False, True):
        with make(nb, x, v, m, mode, block=None, dt=1 / 256) as sim:
            if toggle:
                sim.block_steps = (ETA, L)
                sim.block_steps = (0.0, 0)
            sim.steps(3)
            sim.step_by(-1 / 256)
            runs.append(state_of(sim) + (np.array([sim.stats().interactions], np.float64),))
            assert sim.block_step_counts() == (0, 0)
    assert same_state(runs[0], runs[1])


def test_degenerate_worlds_step(gpu):
    nb = gpu
    for mode in (nb.STRICT, nb.FAST):
        for n in (0, 1, 2):
            x, v, m = hr.world(n)
            with make(nb, x, v, m, mode) as sim:
                sim.step_by(1 / 16)
                sim.steps(2)
                assert len(sim) == n and sim.stats().steps == 3 and sim.elapsed() == 3 / 16
                assert sim.levels().shape == (n,)
                if n == 1:
                    assert not sim.levels().any()
                    assert sim.block_step_counts() == (3, 3) and sim.stats().interactions == 0
                    assert eq(sim.get_points()["position"], x + v * (3 / 16))
