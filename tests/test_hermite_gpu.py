"""The fourth-order Hermite integrator of brute-force f64 handles (nbody_set_integrator, kernels_hermite.hip).

Strict math: forces, jerks and whole trajectories bit for bit beside tests/hermite_ref.py, the retain included.  Fast math:
every row of a and j within the per-row bounds (bf64_bound.R, hermite_ref.RJ) over every path of the pair-jerk kernels,
trajectories beside a strict handle, determinism, steps(k), clone, the order of the scheme, staleness of the held
derivatives, nbody_suggest_dt, no trace in the leapfrog, and the refusals.  Prints its worst ratios under pytest -s."""
import ctypes

import numpy as np
import pytest

import hermite_ref as hr
from bf64_bound import bound_errors

pytestmark = pytest.mark.gpu
DT = 1.0 / 128


def eq(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make(nb, x, v, m, math, hermite=True, capacity=None, dt=DT, box=hr.BOX, **tuning):
    sim = nb.Simulation(hr.records(nb.PARTICLE_DTYPE64, x, v, m), *box, method=nb.BRUTE_FORCE, math_mode=math, f64=True,
                        capacity=capacity, tuning=tuning)
    sim.settings = nb.Settings(g=hr.G, g_soft=hr.EPS, dt=dt, theta2=0.5)
    if hermite:
        sim.integrator = nb.HERMITE4
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


# ---------------------------------------------------------------------------------------------- 1. strict math
def test_strict_forces_are_the_restatement_bit_for_bit(gpu):
    nb = gpu
    x, v, m = hr.world(256)
    a, j = hr.strict_aj(x, v, m, hr.G, hr.EPS)
    with make(nb, x, v, m, nb.STRICT) as sim:
        assert sim.integrator == nb.HERMITE4
        sim.update_forces()
        assert eq(sim.get_points()["acceleration"], a) and eq(sim.jerk(), j)
        assert sim.stats().interactions == 256 * 255


@pytest.mark.parametrize("leaver", [False, True])
def test_strict_trajectory_bit_for_bit(gpu, leaver):
    """Eight step_by calls (one with a negative dt) beside hermite_step; with `leaver` a 257th body, at index 100, crosses the
    wall during step 3: the count drops, order is preserved, survivors keep their held (a0, j0)."""
    nb = gpu
    x, v, m = hr.world(256)
    if leaver:
        x = np.insert(x, 100, (31.9, 0.3, -0.2), axis=0)
        v = np.insert(v, 100, (6.0, 0.0, 0.0), axis=0)      # 31.9 + 3 * 6 / 128 > 32: out during step 3
        m = np.insert(m, 100, 1.0 / 256)
    n0 = len(x)
    dts = [DT, DT, DT, 0.5 * DT, -DT, DT, 2.0 * DT, DT]
    ref = hr.start(x, v, m)
    with make(nb, x, v, m, nb.STRICT) as sim:
        sim.init()
        t, evals = 0.0, 1                                     # the first step evaluates F at the uploaded state first
        for k, dt in enumerate(dts):
            sim.step_by(dt)
            ref = hr.hermite_step(ref, dt)
            t += dt
            evals += 1
            assert same_state(state_of(sim), ref), f"step {k + 1}"
            assert len(sim) == len(ref[0]) == (n0 - 1 if leaver and k >= 2 else n0), f"step {k + 1}"
            assert sim.elapsed() == t
        st = sim.stats()
        assert st.steps == 8
        if not leaver:
            assert st.interactions == evals * n0 * (n0 - 1)
        else:   # steps 1..3 (and the first pass) saw 257 bodies, the five after them 256
            assert st.interactions == 4 * 257 * 256 + 5 * 256 * 255
    if leaver:
        assert eq(ref[4], np.delete(m, 100))


def test_strict_retain_across_tile_boundaries_bit_for_bit(gpu):
    """The retain's look-back over several tiles with the Hermite payload (four arrays): 2 304 bodies are tiles of
    1 024 + 1 024 + 256, and a box of width 2.4 (two standard deviations of the cluster a side) drops about an eighth of every
    tile in the first step_by and a few more bodies of both remaining tiles in the second, longer one.  The masks the
    restatement retains by are asserted to do so, then state and count are compared bit for bit."""
    nb = gpu
    x, v, m = hr.world(2304)
    box = ((0.0, 0.0, 0.0), 2.4)
    ref = hr.start(x, v, m)
    with make(nb, x, v, m, nb.STRICT, box=box) as sim:
        sim.init()
        for k, (dt, tiles) in enumerate(((DT, 3), (4.0 * DT, 2))):
            unbounded = hr.hermite_step(ref, dt, box=((0.0, 0.0, 0.0), np.inf))
            keep = hr.contains(unbounded[0], *box)
            assert len(keep) > 1024 * (tiles - 1), f"step {k + 1}: the state no longer spans {tiles} tiles"
            for t in range(tiles):
                part = keep[1024 * t:1024 * (t + 1)]
                assert part.any() and not part.all(), f"step {k + 1}, tile {t}: needs leavers and survivors"
            ref = hr.hermite_step(ref, dt, box=box)
            assert eq(ref[0], unbounded[0][keep])
            sim.step_by(dt)
            assert len(sim) == len(ref[0]) == int(keep.sum()), f"step {k + 1}"
            assert same_state(state_of(sim), ref), f"step {k + 1}"


# ---------------------------------------------------------------------------------------------- 2. fast math, every row
FAST_CASES = [
    (1, {}, "degenerate"),
    (2, {}, "degenerate"),
    (200, {}, "one-sided, mode 0"),
    (300, dict(bf64_min_bodies=2), "A = 2: left-over pairs only"),
    (700, dict(bf64_min_bodies=2), "A = 3: one symmetric set distance"),
    (1000, dict(bf64_min_bodies=2), "A = 4: opposite set in the left-over kernel"),
    (1000, dict(bf64_min_bodies=2, bf64_rot=1), "A = 4, rotation scheme"),
    (1500, dict(bf64_min_bodies=2, bf64_waves=64), "few slices"),
]
_direct = {}


def direct(n):
    if n not in _direct:
        x, v, m = hr.world(n)
        _direct[n] = (x, v, m, hr.direct_aj(x, v, m, hr.G, hr.EPS, np.arange(n)))
    return _direct[n]


@pytest.mark.parametrize("n,tuning,what", FAST_CASES, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in t.items()) or 'default'}" for n, t, _ in FAST_CASES])
def test_fast_forces_every_row_within_the_bounds(gpu, n, tuning, what):
    nb = gpu
    x, v, m, (Sa, Ta, Sj, Tj) = direct(n)
    with make(nb, x, v, m, nb.FAST, **tuning) as sim:
        sim.update_forces()
        a, j = sim.get_points()["acceleration"], sim.jerk()
        assert sim.stats().interactions == n * (n - 1)
    ea, ej = bound_errors(a, Sa, Ta), bound_errors(j, Sj, Tj)
    print(f"\n[hermite fast] n={n} {what}: worst |a - S_a| / T_a {ea.max():.3e}, |j - S_j| / T_j {ej.max():.3e}")
    assert ea.max() <= hr.R, (what, np.flatnonzero(~(ea <= hr.R))[:8], ea.max())
    assert ej.max() <= hr.RJ, (what, np.flatnonzero(~(ej <= hr.RJ))[:8], ej.max())
    if n == 1:
        assert not a.any() and not j.any()


def test_degenerate_worlds_step_and_suggest_infinity(gpu):
    nb = gpu
    for math in (nb.STRICT, nb.FAST):
        for n in (0, 1):
            x, v, m = hr.world(n)
            with make(nb, x, v, m, math) as sim:
                assert sim.suggest_dt(0.02) == float("inf")
                sim.step_by(DT)
                sim.steps(2)
                p = sim.get_points()
                assert len(p) == n and sim.jerk().shape == (n, 3)
                assert not p["acceleration"].any() and not sim.jerk().any()
                if n:
                    assert eq(p["position"], hr.hermite_step(hr.hermite_step(hr.hermite_step(hr.start(x, v, m), DT), DT), DT)[0])
                assert sim.stats().steps == 3 and sim.stats().interactions == 0


# ---------------------------------------------------------------------------------------------- 3. fast trajectory
def test_fast_trajectory_beside_strict_steps_repeat_and_clone(gpu):
    nb = gpu
    x, v, m = hr.world(700)
    knobs = dict(bf64_min_bodies=2)   # the symmetric path
    with make(nb, x, v, m, nb.STRICT) as strict, make(nb, x, v, m, nb.FAST, **knobs) as fast:
        for _ in range(16):
            strict.step_by(DT)
            fast.step_by(DT)
        want, got = state_of(strict), state_of(fast)
    err = np.abs(got[0] - want[0]).max() / hr.BOX[1]
    print(f"\n[hermite fast] 16 steps beside strict: position error {err:.3e} of the box width")
    assert len(got[0]) == 700 and err <= 1e-11
    with make(nb, x, v, m, nb.FAST, **knobs) as sim:      # steps(16): the bits of 16 step_by calls
        sim.steps(16)
        assert same_state(state_of(sim), got) and sim.stats().steps == 16
        assert sim.stats().interactions == 17 * 700 * 699
    with make(nb, x, v, m, nb.FAST, **knobs) as sim:      # a second run repeats; a clone after step 5 ends like its source
        for _ in range(5):
            sim.step_by(DT)
        with sim.clone() as twin:
            assert twin.integrator == nb.HERMITE4 and eq(twin.jerk(), sim.jerk())
            for _ in range(11):
                sim.step_by(DT)
                twin.step_by(DT)
            assert same_state(state_of(sim), got)
            assert same_state(state_of(twin), got)
            assert twin.stats().interactions == 11 * 700 * 699     # the held derivatives came along: no extra pass


# ---------------------------------------------------------------------------------------------- 4. order
def test_fourth_order_and_energy_against_the_leapfrog(gpu):
    nb = gpu
    x, v, m = hr.world(64)
    T = 0.5

    def run(steps, hermite=True):
        with make(nb, x, v, m, nb.FAST, hermite=hermite, dt=T / steps) as sim:
            e0 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
            sim.steps(steps)
            e1 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
            return sim.get_points()["position"], abs((e1 - e0) / e0)

    ref, _ = run(1024)
    p64, _ = run(64)
    p128, de_h = run(128)
    _, de_l = run(128, hermite=False)
    e64, e128 = np.abs(p64 - ref).max(), np.abs(p128 - ref).max()
    print(f"\n[hermite order] position error 64 steps {e64:.3e}, 128 steps {e128:.3e}: ratio {e64 / e128:.2f}; "
          f"relative energy error at 128 steps: Hermite {de_h:.3e}, leapfrog {de_l:.3e}")
    assert e64 / e128 >= 12.0
    assert de_h < 0.1 * de_l


# ---------------------------------------------------------------------------------------------- 5. staleness, suggest_dt
ACTIONS = ["upload", "add_point", "remove_point", "settings", "init"]


@pytest.mark.parametrize("math", ["strict", "fast"])
@pytest.mark.parametrize("action", ACTIONS)
def test_stale_derivatives_are_refused_and_re_evaluated(gpu, action, math):
    nb = gpu
    mode = nb.STRICT if math == "strict" else nb.FAST
    x, v, m = hr.world(256)
    g = hr.G
    with make(nb, x, v, m, mode, capacity=300) as sim:
        sim.step_by(DT)
        sim.step_by(DT)
        assert sim.jerk().shape == (256, 3)
        before = sim.stats().interactions
        if action == "upload":
            sim.upload(hr.records(nb.PARTICLE_DTYPE64, *hr.world(200, seed=9)))
        elif action == "add_point":
            sim.add_point(hr.records(nb.PARTICLE_DTYPE64, [(0.2, 0.1, -0.3)], [(0.01, 0.0, 0.02)], [0.01]))
        elif action == "remove_point":
            sim.remove_point(5)
        elif action == "settings":
            g = 1.25
            sim.settings = nb.Settings(g=g, g_soft=hr.EPS, dt=DT, theta2=0.5)
        else:
            sim.init()
        refused(nb, sim.jerk, "nbody_download_jerk")
        now = sim.get_points()
        n = len(now)
        assert n == {"upload": 200, "add_point": 257, "remove_point": 255}.get(action, 256)
        sim.step_by(DT)
        got = state_of(sim)
        assert sim.stats().interactions - before == 2 * n * (n - 1)     # the extra pass is counted
        with make(nb, now["position"], now["velocity"], now["mass"], mode) as fresh:
            fresh.settings = nb.Settings(g=g, g_soft=hr.EPS, dt=DT, theta2=0.5)
            fresh.step_by(DT)
            assert same_state(state_of(fresh), got)
        if math == "strict":
            assert same_state(got, hr.hermite_step(hr.start(now["position"], now["velocity"], now["mass"], g=g), DT, g=g))


@pytest.mark.parametrize("math", ["strict", "fast"])
def test_suggest_dt_is_the_numpy_expression_bit_for_bit(gpu, math):
    nb = gpu
    x, v, m = hr.world(700)
    with make(nb, x, v, m, nb.STRICT if math == "strict" else nb.FAST, bf64_min_bodies=2) as sim:
        refused(nb, sim.jerk, "nbody_download_jerk")          # stale after the upload
        dt = sim.suggest_dt(0.02)                             # evaluates F first
        a, j = sim.get_points()["acceleration"], sim.jerk()
        assert dt == hr.suggest_dt(a, j, 0.02) and 0 < dt < 1
        assert sim.stats().interactions == 700 * 699
        sim.step_by(DT)
        dt = sim.suggest_dt(0.01)
        assert dt == hr.suggest_dt(sim.get_points()["acceleration"], sim.jerk(), 0.01)
        assert sim.stats().interactions == 2 * 700 * 699      # valid derivatives: no pass of its own
        refused(nb, lambda: sim.suggest_dt(0.0), "eta")
        refused(nb, lambda: sim.suggest_dt(-1.0), "eta")
        print(f"\n[hermite suggest_dt] {math}: eta = 0.01 -> {dt:.6e}")


# ---------------------------------------------------------------------------------------------- 6. no trace in the leapfrog
@pytest.mark.parametrize("math", ["strict", "fast"])
def test_selecting_and_deselecting_leaves_no_trace_in_the_leapfrog(gpu, math):
    nb = gpu
    mode = nb.STRICT if math == "strict" else nb.FAST
    x, v, m = hr.world(700)
    runs = []
    for toggle in (False, True):
        with make(nb, x, v, m, mode, hermite=False, bf64_min_bodies=2) as sim:
            if toggle:
                sim.integrator = nb.HERMITE4
                sim.integrator = nb.LEAPFROG
            assert sim.integrator == nb.LEAPFROG
            sim.steps(3)
            sim.step_by(DT)
            sim.step_by(-DT)
            p = sim.get_points()
            runs.append((p["position"], p["velocity"], p["acceleration"], sim.stats().interactions))
    assert all(eq(a, b) for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(gpu):
    nb = gpu
    x, v, m = hr.world(64)
    rec64 = hr.records(nb.PARTICLE_DTYPE64, x, v, m)
    rec32 = hr.records(nb.PARTICLE_DTYPE, x, v, m)
    others = [
        lambda: nb.Simulation(rec32, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST),                       # f32
        lambda: nb.Simulation(rec64, *hr.BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, f64=True),              # Barnes-Hut
        lambda: nb.Simulation(rec64, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.STRICT, f64=True, rank=0, world_size=2),
    ]
    for ctor in others:
        with ctor() as sim:
            refused(nb, lambda: setattr(sim, "integrator", nb.HERMITE4), "nbody_set_integrator")
            sim.integrator = nb.LEAPFROG                      # valid on every handle, a no-op
            assert sim.integrator == nb.LEAPFROG
            refused(nb, sim.jerk, "nbody_download_jerk")
            refused(nb, lambda: sim.suggest_dt(0.02), "nbody_suggest_dt")
    with make(nb, x, v, m, nb.STRICT, hermite=False) as sim:
        refused(nb, lambda: setattr(sim, "integrator", 2), "nbody_set_integrator")
        refused(nb, lambda: setattr(sim, "integrator", -1), "nbody_set_integrator")
        refused(nb, sim.jerk, "nbody_download_jerk")          # a leapfrog handle
        refused(nb, lambda: sim.suggest_dt(0.02), "nbody_suggest_dt")
        sim.integrator = nb.HERMITE4
        refused(nb, sim.jerk, "nbody_download_jerk")          # stale until the first evaluation
        n = ctypes.c_size_t(0)
        assert nb.lib.nbody_download_jerk(sim._h, None, 0, ctypes.byref(n)) == nb.NBODY_ERR_INVALID   # a NULL buffer too
        sim.update_forces()
        assert sim.jerk().shape == (64, 3)
        sim.integrator = nb.LEAPFROG                          # a change of integrator makes them stale again
        sim.integrator = nb.HERMITE4
        refused(nb, sim.jerk, "nbody_download_jerk")
