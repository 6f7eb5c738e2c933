"""Exact pair coverage of the Hermite fast-math force pass (kernels_hermite.hip) on the plans a user gets.

Probe worlds (tests/hermite_probe.py: one massive body, every body moving) through nbody_update_forces -- k_hm_sym<IPT, ROT>,
k_hm_os<MODE>, k_hm_reduce<false> -- at the default thresholds (the one-sided kernel alone up to 10 239 bodies, the symmetric
scheme with A >= 40 sets of 256 from 10 240 on, four bodies a lane beyond 16 384 too) and at every knob value, and through
nbody_debug_hermite_forces_of -- k_hm_act, k_hmb_finish<true, false> -- with id lists that reach both arms of make_hm_act_plan.
Then full sums at production plans on sampled rows (the plane reduce over many non-zero planes), and the fused corrector of
k_hm_reduce<true> bit for bit from the handle's own (a1, j1), the retain included.  Which kernel a case launches is asserted from
the plan: NbodyStats::force_kernel_interactions of a profiled pass counts the symmetric kernel's directed pairs.
Every test prints its worst ratios (pytest -s)."""
import numpy as np
import pytest

import hermite_ref as hr
from bf64_bound import bound_errors
from hermite_probe import PROBE_G, check_probe_aj, probe_columns, probe_records64, probe_reference_aj, probe_velocities, set_probe

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
EPS = 2.0 ** -7              # a softening length f32 can hold exactly
MIN_BODIES = 10240           # Tuning::bf64_min_bodies (kernels.h)
SMALL_IPT_BELOW = 16384      # kBf64SmallIptBelow (kernels_f64.h): where the leapfrog pass goes from 4 to 8 bodies a lane
WAVES = 2048                 # what bf64_waves = 0 means
DT = 1.0 / 128


def eq(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def positions(nb, n, seed):
    """n f32-representable Plummer positions (as f64), all well inside BOX."""
    pos = nb.plummer(2 * n + 64, seed=seed)["position"]
    pos = pos[np.abs(pos).max(1) < 30.0][:n]
    assert len(pos) == n
    return np.ascontiguousarray(pos, dtype=np.float64)


def hermite(nb, rec, g, eps, box=BOX, **tuning):
    sim = nb.Simulation(rec, *box, method=nb.BRUTE_FORCE, math_mode=nb.FAST, f64=True, tuning=tuning)
    sim.settings = nb.Settings(g=g, g_soft=eps, dt=DT, theta2=0.5)
    sim.integrator = nb.HERMITE4
    return sim


# ---------------------------------------------------------------------------------------------- the plans, restated
def sym_plan(n, min_bodies=MIN_BODIES, ipt=0, waves=0):
    """make_bf64_plan(n, 0, 1, hermite_ipt(ipt)) (kernels_bf64.hip, kernels_hermite.h): the shape of a Hermite handle's pass."""
    want = waves if waves > 0 else WAVES
    groups = (n + 63) // 64
    if n < max(2, min_bodies):
        return dict(sym=False, ipt=0, A=0, sym_sets=0, K=0, k_own=max(1, min((n + 127) // 128, (want + groups - 1) // groups)))
    ipt = 8 if ipt == 8 else 4
    A = (n + 64 * ipt - 1) // (64 * ipt)
    sym_sets = (A + 1) // 2 - 1
    K = max(1, min(ipt * sym_sets, (want + A - 1) // A)) if sym_sets > 0 else 0
    return dict(sym=True, ipt=ipt, A=A, sym_sets=sym_sets, K=K, k_own=max(1, min(16, (want + A * ipt - 1) // (A * ipt))))


def sym_directed_pairs(n, plan):
    """What a profiled pass of that plan adds to force_kernel_interactions (nbody_f64.cpp hm_eval): the symmetric kernel's pairs,
    both directions; every pair where the one-sided kernel is the only one (no plan, or one or two sets)."""
    if not plan["sym"] or plan["sym_sets"] == 0:
        return n * (n - 1)
    size = 64 * plan["ipt"]
    sizes = [max(0, min(size, n - a * size)) for a in range(plan["A"])]
    return 2 * sum(sizes[a] * sizes[(a + d) % plan["A"]] for a in range(plan["A"]) for d in range(1, plan["sym_sets"] + 1))


def act_plan(n_act, n, waves=0):
    """make_hm_act_plan: (groups, K)."""
    groups = (n_act + 63) // 64
    return groups, max(1, min((waves if waves > 0 else WAVES) // max(1, groups), (n + 63) // 64))


def assert_plan(sim, n, plan, what):
    """One profiled force pass of the handle's current world: its symmetric kernel met exactly the plan's pairs."""
    sim.set_profiling(1)
    before = sim.stats().force_kernel_interactions
    sim.update_forces()
    got = sim.stats().force_kernel_interactions - before
    sim.set_profiling(0)
    assert got == sym_directed_pairs(n, plan), (what, got, plan)


# ---------------------------------------------------------------------------------------------- probes, update_forces
def probe_update_forces(nb, sim, pos, vel, cols, what):
    """Probe columns `cols` through update_forces, eps = 0 and 2^-7 alternately; returns the worst ratios."""
    rec = probe_records64(nb.PARTICLE_DTYPE64, pos, vel)
    worst_a = worst_j = 0.0
    for c, k in enumerate(cols):
        eps = (0.0, EPS)[c % 2]
        sim.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=DT, theta2=0.5)
        sim.upload(set_probe(rec, k))
        sim.update_forces()
        ea, ej = check_probe_aj(sim.get_points()["acceleration"], sim.jerk(), pos, vel, k, PROBE_G, eps, what=what)
        worst_a, worst_j = max(worst_a, ea), max(worst_j, ej)
    return worst_a, worst_j


def report(what, plan, cols, worst, rot=0):
    shape = (f"k_hm_sym<{plan['ipt']}, {rot}> A={plan['A']} sym_sets={plan['sym_sets']} K={plan['K']} + k_hm_os<1> k_own={plan['k_own']}"
             if plan["sym"] and plan["sym_sets"] else f"k_hm_os<{1 if plan['sym'] else 0}> alone, k_own={plan['k_own']}")
    print(f"\n[hermite probe] {what} ({len(cols)} columns; {shape}): worst |a - S_a| / |S_a| {worst[0]:.3e}, |j - S_j| / T_j {worst[1]:.3e}")


def test_the_restated_plans_are_the_issue_s():
    """The shapes this file's cases are chosen for, from the restated plan arithmetic (no GPU work)."""
    assert not sym_plan(MIN_BODIES - 1)["sym"] and sym_plan(MIN_BODIES - 1)["k_own"] == 13   # slices of >= 128 partners
    p = sym_plan(MIN_BODIES)
    assert (p["ipt"], p["A"], p["sym_sets"], p["K"]) == (4, 40, 19, 52)
    for n in (SMALL_IPT_BELOW + 1, 20000):                                                   # four bodies a lane at every size
        assert sym_plan(n)["ipt"] == 4 and sym_directed_pairs(n, sym_plan(n)) != sym_directed_pairs(n, sym_plan(n, ipt=8))
    assert [sym_plan(n, 2)["A"] for n in (300, 700, 1000)] == [2, 3, 4]
    n = 12033
    assert [act_plan(k, n) for k in (1, 64, 65, 704, 4096, n)] == [(1, 189), (1, 189), (2, 189), (11, 186), (64, 32), (189, 10)]
    lens = {n * (s + 1) // 186 - n * s // 186 for s in range(186)}
    assert lens == {64, 65}                                                                   # slices of one and of two tiles


@pytest.mark.parametrize("n", [65, MIN_BODIES - 1, MIN_BODIES, MIN_BODIES + 1, 12033, SMALL_IPT_BELOW, SMALL_IPT_BELOW + 1, 20000])
def test_probe_every_pair_direction_default_tuning(gpu, n):
    nb = gpu
    pos, vel = positions(nb, n, seed=n), probe_velocities(n)
    plan = sym_plan(n)
    cols = probe_columns(n, set_sizes=(256,), n_random=12, every_below=70)
    with hermite(nb, probe_records64(nb.PARTICLE_DTYPE64, pos, vel), PROBE_G, 0.0) as sim:
        worst = probe_update_forces(nb, sim, pos, vel, cols, f"n={n}")
        if n > SMALL_IPT_BELOW:    # sets of 256: the Hermite pass does not follow the leapfrog's switch to eight bodies a lane
            assert plan["ipt"] == 4 and sym_directed_pairs(n, plan) != sym_directed_pairs(n, sym_plan(n, ipt=8))
        assert_plan(sim, n, plan, f"n={n}")
    report(f"n={n} default tuning", plan, cols, worst)


KNOBS = [
    (1500, dict(bf64_min_bodies=2, bf64_ipt=8)), (1500, dict(bf64_min_bodies=2, bf64_ipt=8, bf64_rot=1)),
    (5000, dict(bf64_min_bodies=2, bf64_ipt=8)), (5000, dict(bf64_min_bodies=2, bf64_ipt=8, bf64_rot=1)),
    (20000, dict(bf64_ipt=8)), (20000, dict(bf64_rot=1)),
    (3001, dict(bf64_min_bodies=2, bf64_waves=64)), (3001, dict(bf64_min_bodies=2, bf64_waves=20000)),
    (20000, dict(bf64_min_bodies=100000)),                                     # the one-sided kernel alone on a large world
    (300, dict(bf64_min_bodies=2)), (700, dict(bf64_min_bodies=2)), (1000, dict(bf64_min_bodies=2)),   # A = 2, 3, 4
]


@pytest.mark.parametrize("n,knobs", KNOBS, ids=[f"{n}-{'-'.join(f'{k[5:]}{v}' for k, v in t.items())}" for n, t in KNOBS])
def test_probe_knobs(gpu, n, knobs):
    nb = gpu
    pos, vel = positions(nb, n, seed=n + 1), probe_velocities(n, seed=1)
    plan = sym_plan(n, knobs.get("bf64_min_bodies", MIN_BODIES), knobs.get("bf64_ipt", 0), knobs.get("bf64_waves", 0))
    cols = probe_columns(n, set_sizes=(512 if plan["ipt"] == 8 else 256,), n_random=12, every_below=70)
    with hermite(nb, probe_records64(nb.PARTICLE_DTYPE64, pos, vel), PROBE_G, 0.0, **knobs) as sim:
        worst = probe_update_forces(nb, sim, pos, vel, cols, f"n={n} {knobs}")
        assert_plan(sim, n, plan, f"n={n} {knobs}")
    report(f"n={n} {knobs}", plan, cols, worst, rot=knobs.get("bf64_rot", 0))


# ---------------------------------------------------------------------------------------------- the two pair laws
LAW_CASES = [(65, {}), (1025, {}), (257, dict(bf64_min_bodies=2)), (513, dict(bf64_min_bodies=2)), (1025, dict(bf64_min_bodies=2))]


@pytest.mark.parametrize("n,knobs", LAW_CASES, ids=[f"{n}-{'min2' if t else 'default'}" for n, t in LAW_CASES])
def test_acceleration_half_of_the_hermite_law_is_the_gravity_law(gpu, n, knobs):
    """The same f64 bodies (every body moving) through nbody_update_forces on a leapfrog handle (kernels_bf64.hip: k_bf64_sym,
    k_bf64_os, k_bf64_reduce) and on a HERMITE4 handle (k_hm_sym, k_hm_os, k_hm_reduce), fast math: the accelerations are
    bit-equal wherever the two plans coincide -- up to kBf64SmallIptBelow bodies both keep four bodies a lane.  Both laws form
    rsqrt, the cube, the mass product and the three FMAs a side in the same order, over the same planes in the same order.
    Default tuning: the one-sided kernels alone (MODE 0); bf64_min_bodies = 2: A = 2 (no symmetric part, two windows), 3 and 5
    (one window, a last set of one body).  That the plans coincide: each handle's profiled pass must report the restated plan's
    symmetric pairs, which pins ipt, A and sym_sets in the bf64_min_bodies = 2 cases.  In the two default cases that count is
    n (n - 1) for any plan; there the equality of the plans (k_own, the plane count) rests on reading make_bf64_plan, which both
    handles call and which does not look at the bodies per lane when it plans no symmetric part -- the library has no host
    call that returns this plan."""
    nb = gpu
    assert n <= SMALL_IPT_BELOW
    plan = sym_plan(n, knobs.get("bf64_min_bodies", MIN_BODIES))
    if knobs:
        assert plan["sym"] and (plan["ipt"], plan["A"], plan["sym_sets"]) == {257: (4, 2, 0), 513: (4, 3, 1), 1025: (4, 5, 2)}[n]
    else:
        assert not plan["sym"]
    x, v, m = hr.world(n)
    assert np.abs(v).min() > 0.0
    rec = hr.records(nb.PARTICLE_DTYPE64, x, v, m)
    with nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, f64=True, tuning=knobs) as sim:
        sim.settings = nb.Settings(g=hr.G, g_soft=hr.EPS, dt=DT, theta2=0.5)
        sim.update_forces()
        a_leapfrog = sim.get_points()["acceleration"]
        assert_plan(sim, n, plan, f"leapfrog n={n} {knobs}")
    with hermite(nb, rec, hr.G, hr.EPS, **knobs) as sim:
        sim.update_forces()
        a_hermite = sim.get_points()["acceleration"]
        assert_plan(sim, n, plan, f"hermite n={n} {knobs}")
    differ = int((np.asarray(a_leapfrog) != np.asarray(a_hermite)).any(1).sum())
    print(f"\n[pair laws] n={n} {knobs}: {differ} of {n} accelerations differ between the leapfrog and the Hermite handle")
    assert eq(a_leapfrog, a_hermite), f"{differ} accelerations differ"


# ---------------------------------------------------------------------------------------------- probes, hermite_forces_of
def act_id_lists(n, k):
    """Ascending draws (fixed seed) that reach each arm of make_hm_act_plan, and one shuffled list; body k is in three of them."""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    lists = {"1 id": perm[:1], "the probe body alone": np.array([k]), "all ids": np.arange(n)}
    for m in (64, 65, 704, 4096):
        lists[f"{m} ids"] = np.sort(perm[:m])
    with_k = np.concatenate([[k], perm[perm != k][:64]])
    lists["65 ids with k"] = np.sort(with_k)
    lists["2000 ids, shuffled"] = rng.permutation(np.concatenate([[k], perm[perm != k][:1999]]))
    return lists


def test_probe_forces_of_listed_bodies_every_plan_arm(gpu):
    """n = 12 033, default tuning (K = 189 capped by ceil(n / 64) for up to 65 ids; 186 = want / groups for 704 ids, partner
    slices of 64 and 65 bodies, i.e. of one and two tiles; 32 for 4 096 ids; 10 for all) and bf64_waves = 64 (K = 64, 64, 32, 5, 1, 1)."""
    nb = gpu
    n = 12033
    pos, vel = positions(nb, n, seed=n), probe_velocities(n)
    # 0, 63 | 64: the first slice boundary of K = 186..189; 128: the one partner of slice [64, 129)'s second tile; 1202 | 1203: the
    # first boundary of K = 10; 600, 6500, 11500: inside its first, a middle and its last slice
    cols = [0, 63, 64, 128, 129, 600, 1202, 1203, 6500, 11500, n - 1]
    assert n // 10 == 1203 and (n * 1 // 186, n * 2 // 186) == (64, 129)
    rec = probe_records64(nb.PARTICLE_DTYPE64, pos, vel)
    worst_a = worst_j = 0.0
    for tuning in ({}, dict(bf64_waves=64)):
        with hermite(nb, rec, PROBE_G, 0.0, **tuning) as sim:
            for c, k in enumerate(cols):
                eps = (0.0, EPS)[c % 2]
                sim.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=DT, theta2=0.5)
                sim.upload(set_probe(rec, k))
                ref = probe_reference_aj(pos, vel, k, PROBE_G, eps)
                for name, ids in act_id_lists(n, k).items():
                    a, j = sim.hermite_forces_of(ids)
                    what = f"k_hm_act n={n} {tuning} {name} (groups, K) = {act_plan(len(ids), n, tuning.get('bf64_waves', 0))}"
                    ea, ej = check_probe_aj(a, j, pos, vel, k, PROBE_G, eps, rows=ids, ref=ref, what=what)
                    worst_a, worst_j = max(worst_a, ea), max(worst_j, ej)
            assert sim.stats().interactions == 0
    print(f"\n[hermite probe] k_hm_act n={n} ({len(cols)} columns x 9 id lists x 2 tunings): worst |a - S_a| / |S_a| {worst_a:.3e}, "
          f"|j - S_j| / T_j {worst_j:.3e}")


# ---------------------------------------------------------------------------------------------- full sums, sampled rows
CASES = {"12033-default": (12033, {}), "5000-ipt8": (5000, dict(bf64_min_bodies=2, bf64_ipt=8))}
_worlds = {}


def rj_n(n):
    """|j - S_j| <= RJ_n T_j whatever the order of summation: 12 roundings a term and n - 1 additions, 2^-53 each."""
    return (12 + n - 1) * 2.0 ** -53


def case_world(case):
    """(x, v, m, rows, direct_aj of the rows), computed once."""
    if case not in _worlds:
        n = CASES[case][0]
        x, v, m = hr.world(n)
        rows = np.unique(np.concatenate([np.random.default_rng(n).choice(n, 96, replace=False), [0, 255, 256, 511, 512, n - 1]]))
        _worlds[case] = (x, v, m, rows, hr.direct_aj(x, v, m, hr.G, hr.EPS, rows))
    return _worlds[case]


def check_rows(a, j, ref, n, what):
    Sa, Ta, Sj, Tj = ref
    ea, ej = bound_errors(a, Sa, Ta), bound_errors(j, Sj, Tj)
    print(f"\n[hermite full sums] {what}: worst |a - S_a| / T_a {ea.max():.3e} (R = {hr.R:g}), |j - S_j| / T_j {ej.max():.3e} "
          f"(RJ_n = {rj_n(n):.3e})")
    assert ea.max() <= hr.R, (what, np.flatnonzero(~(ea <= hr.R))[:8], ea.max())
    assert ej.max() <= rj_n(n), (what, np.flatnonzero(~(ej <= rj_n(n)))[:8], ej.max())


@pytest.mark.parametrize("case", list(CASES))
def test_full_sums_at_production_plans_sampled_rows(gpu, case):
    nb = gpu
    n, tuning = CASES[case]
    x, v, m, rows, ref = case_world(case)
    assert rj_n(n) < 1e-11
    with hermite(nb, hr.records(nb.PARTICLE_DTYPE64, x, v, m), hr.G, hr.EPS, **tuning) as sim:
        sim.update_forces()
        a, j = sim.get_points()["acceleration"], sim.jerk()
        assert sim.stats().interactions == n * (n - 1)
        assert_plan(sim, n, sym_plan(n, tuning.get("bf64_min_bodies", MIN_BODIES), tuning.get("bf64_ipt", 0)), case)
    check_rows(a[rows], j[rows], ref, n, f"{case}, {len(rows)} rows")


# ---------------------------------------------------------------------------------------------- the fused corrector
def state_of(sim):
    p = sim.get_points()
    return p["position"], p["velocity"], p["acceleration"], sim.jerk()


_steps = {}


def one_wide_step(nb, case):
    """(state before, state after) of one step_by(DT) in a box nobody leaves, after update_forces; run once per case."""
    if case not in _steps:
        n, tuning = CASES[case]
        x, v, m = case_world(case)[:3]
        with hermite(nb, hr.records(nb.PARTICLE_DTYPE64, x, v, m), hr.G, hr.EPS, **tuning) as sim:
            sim.update_forces()
            s0 = state_of(sim)
            sim.step_by(DT)
            s1 = state_of(sim)
            assert len(sim) == n and sim.stats().interactions == 2 * n * (n - 1)
        _steps[case] = (s0, s1)
    return _steps[case]


def corrected(s0, a1, j1):
    """hermite_ref.hermite_step's corrector lines on the held (x0, v0, a0, j0) and the new (a1, j1)."""
    x0, v0, a0, j0 = s0
    _, _, _, h, c12 = hr.coef(DT)
    v1 = (v0 + (a0 + a1) * h) + (j0 - j1) * c12
    x1 = (x0 + (v0 + v1) * h) + (a0 - a1) * c12
    return x1, v1


@pytest.mark.parametrize("case", list(CASES))
def test_fused_corrector_bit_for_bit_from_the_handles_own_derivatives(gpu, case):
    """k_hm_reduce<true>: x1 and v1 are the corrector's expressions on the a1 and j1 the handle reports, bit for bit (the library
    builds with -ffp-contract=off and the fused reduce calls the strict path's correct_one); a1 and j1 themselves are F at the
    predicted state within the per-row bounds."""
    nb = gpu
    n = CASES[case][0]
    x, v, m, rows, ref0 = case_world(case)
    s0, s1 = one_wide_step(nb, case)
    assert eq(s0[0], x) and eq(s0[1], v)
    check_rows(s0[2][rows], s0[3][rows], ref0, n, f"{case}: held (a0, j0)")
    x1, v1 = corrected(s0, s1[2], s1[3])
    assert eq(s1[1], v1), f"{int((s1[1] != v1).any(1).sum())} velocities differ"
    assert eq(s1[0], x1), f"{int((s1[0] != x1).any(1).sum())} positions differ"
    x0, v0, a0, j0 = s0
    dt, c2, c3, _, _ = hr.coef(DT)
    xp = ((x0 + v0 * dt) + a0 * c2) + j0 * c3
    vp = (v0 + a0 * dt) + j0 * c2
    check_rows(s1[2][rows], s1[3][rows], hr.direct_aj(xp, vp, m, hr.G, hr.EPS, rows), n, f"{case}: (a1, j1) at the predicted state")


@pytest.mark.parametrize("case", list(CASES))
def test_fused_corrector_retain_in_a_tight_box(gpu, case):
    """The same step in a box a few bodies leave.  The width comes from the CPU: hermite_step with force = fast_aj from the
    handle's held (a0, j0), F evaluated for the 256 outermost bodies only (nobody else is near a wall; rows without F are NaN and
    drop out), the wall halfway between the 24th and the 25th largest |x1|_inf.  Count, order and the survivors' bits then follow
    `contains` on the numpy x1 formed from the handle's own a1 and j1."""
    nb = gpu
    n, tuning = CASES[case]
    x, v, m = case_world(case)[:3]
    s0, s1 = one_wide_step(nb, case)
    far = np.sort(np.argsort(np.abs(s0[0]).max(1))[-256:])

    def force(xp, vp, mm, g, eps):
        a, j = np.full_like(xp, np.nan), np.full_like(xp, np.nan)
        a[far], j[far] = hr.fast_aj(xp, vp, mm, g, eps, rows=far)
        return a, j

    cpu_x1 = hr.hermite_step(s0 + (m,), DT, box=((0.0, 0.0, 0.0), np.inf), force=force)[0]
    assert len(cpu_x1) == 256
    r = np.sort(np.abs(cpu_x1).max(1))
    box = ((0.0, 0.0, 0.0), float(r[-25] + r[-24]))
    x1, v1 = corrected(s0, s1[2], s1[3])
    keep = hr.contains(x1, *box)
    lost = n - int(keep.sum())
    assert 1 <= lost <= n // 8, lost
    with hermite(nb, hr.records(nb.PARTICLE_DTYPE64, x, v, m), hr.G, hr.EPS, box=box, **tuning) as sim:
        sim.update_forces()
        assert all(eq(p, q) for p, q in zip(state_of(sim), s0)), "the same input gives the same bits"
        sim.step_by(DT)
        got = state_of(sim)
        assert len(sim) == len(got[0]) == n - lost
        assert eq(sim.get_points()["mass"], m[keep])
    for name, g, want in zip(("position", "velocity", "acceleration", "jerk"), got, (x1, v1, s1[2], s1[3])):
        assert eq(g, want[keep]), name
    print(f"\n[hermite corrector] {case}: box width {box[1]:.6f}, {lost} of {n} bodies left, the survivors bit for bit")
