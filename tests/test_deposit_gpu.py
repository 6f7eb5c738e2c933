"""nbody_deposit on the device (include/nbody_hip.h, "grid deposit") against the numpy restatement (tests/deposit_ref.py): grid
and counts equal byte for byte on both dtypes, every world, the three schemes, the six quantities, periodic and not and both
projections; every plan of the knobs, the plain-atomics variant included, gives the same bytes; 65 536 bodies on 64^3 against
nbody_host_deposit on a device-built Barnes-Hut handle; handle states, no trace, refusals, the command line and the Python
mirror.  What makes these worlds worth looking at is asserted on the CPU in tests/test_deposit_checker.py."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import deposit_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER, WIDTH = (0.0, 0.0, 0.0), 1.0e6   # (far_periodic's bodies stand 12 000 away)
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
PLANS = list(itertools.product((0, 1), (0, 1), (0, 1)))   # deposit_sort, deposit_combine, deposit_lds


def settings(**kw):
    return dict(dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5), **kw)


def make(nb, rec, method="bf", st=None, width=WIDTH, hermite=False, block=None, **kw):
    bh = method == "bh"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO, capacity=max(len(rec), 4), **kw)
    sim.settings = nb.Settings(**(st or settings()))
    sim.init()
    if hermite:
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
    return sim


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


@functools.lru_cache(maxsize=None)
def world(name, f64):
    return ref.world(_nb(), name, f64)


@functools.lru_cache(maxsize=None)
def expected(name, f64, which, grid, scheme, periodic):
    """(grid, counts) of the restatement, computed once and left unchanged"""
    rec = world(name, f64)
    origin, spacing, dims, axis = ref.GRIDS[grid]
    return ref.deposit(ref.bodies(rec)[0], ref.quantity(rec, which), origin, spacing, dims, scheme, periodic, axis)


def dep(sim, grid, scheme, which=ref.MASS, periodic=False):
    origin, spacing, dims, axis = ref.GRIDS[grid]
    return sim.deposit(origin, spacing, dims, scheme=scheme, quantity=which, periodic=periodic, project_axis=axis)


def restated(rec, grid, scheme, which=ref.MASS, periodic=False):
    origin, spacing, dims, axis = ref.GRIDS[grid]
    return ref.deposit(ref.bodies(rec)[0], ref.quantity(rec, which), origin, spacing, dims, scheme, periodic, axis)


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def set_plan(sim, plan):
    for knob, v in zip(("deposit_sort", "deposit_combine", "deposit_lds"), plan):
        sim.set_tuning(knob, v)


# ------------------------------------------------------------------------------------------------ 1. the restatement
@DTYPES
@pytest.mark.parametrize("name", ref.WORLDS)
def test_grid_and_counts_are_the_restatement_s_byte_for_byte(gpu, name, f64):
    nb = gpu
    rec = world(name, f64)
    quantities = ref.QUANTITIES if name in ("plummer4099", "holed") else (ref.MASS,)
    with make(nb, rec) as sim:
        for which in quantities:
            grids = ref.GRIDS if which == ref.MASS else ("16^3", "32x32x1_z")
            for grid, scheme, periodic in itertools.product(grids, ref.SCHEMES, (False, True)):
                what = f"{name} quantity {which} {grid} scheme {scheme} periodic {periodic}"
                got = dep(sim, grid, scheme, which, periodic)
                ref.same_bits(got, expected(name, f64, which, grid, scheme, periodic), what)
                assert got[0].shape == ref.GRIDS[grid][2] and int(got[1].sum()) == len(rec), what
        same_records(sim.get_points(), rec, "a read-only call")


# ------------------------------------------------------------------------------------------------ 2. the plan does not show
@DTYPES
@pytest.mark.parametrize("name", ["one_cell", "plummer4099"])
def test_every_plan_gives_the_same_bytes(gpu, name, f64):
    nb = gpu
    rec = world(name, f64)
    with make(nb, rec) as sim:
        assert [sim.get_tuning(k) for k in ("deposit_sort", "deposit_combine", "deposit_lds")] == [1, 1, 1]
        for grid, scheme, periodic in (("16^3", ref.NGP, False), ("16^3", ref.CIC, True), ("16^3", ref.TSC, False), ("32x32x1_z", ref.TSC, False),
                                       ("5x3x2", ref.CIC, False)):
            want = expected(name, f64, ref.MASS, grid, scheme, periodic)
            issued = {}
            for plan in PLANS:
                set_plan(sim, plan)
                ref.same_bits(dep(sim, grid, scheme, ref.MASS, periodic), want, f"{name} {grid} scheme {scheme} plan {plan}")
                stats = sim.deposit_stats()
                assert stats[0] == 1 and stats[1] == plan[0] | plan[1] << 1 | plan[2] << 2
                issued[plan] = (int(stats[2]), int(stats[3]))
            terms = {v[0] for v in issued.values()}
            assert len(terms) == 1, issued   # the terms on the grid are the state's, not the plan's
            # the plain variant sends one atomic per term that is not zero; sorting and combining only ever send fewer
            assert issued[(0, 0, 0)][1] <= issued[(0, 0, 0)][0] and issued[(1, 1, 0)][1] <= issued[(0, 0, 0)][1], issued
            if name == "one_cell" and scheme == ref.NGP:   # 4 099 bodies in one cell: one atomic a wave
                assert issued[(1, 1, 0)][1] == -(-len(rec) // 64), issued


# ------------------------------------------------------------------------------------------------ 3. a larger world, device against host
def test_65536_bodies_on_64_cubed_against_the_host_call(gpu):
    nb = gpu
    rec = nb.plummer(65536, seed=3)
    rec["mass"] = rec["mass"] * np.random.default_rng(3).uniform(0.5, 1.5, len(rec)).astype(np.float32)
    origin, spacing, dims = (-2.0, -2.0, -2.0), 0.0625, (64, 64, 64)
    with make(nb, rec, method="bh", width=64.0) as sim:
        for scheme in ref.SCHEMES:
            got = sim.deposit(origin, spacing, dims, scheme=scheme)
            want = nb.host_deposit(ref.bodies(rec)[0], ref.quantity(rec, ref.MASS), origin, spacing, dims, scheme=scheme)
            ref.same_bits(got, want, f"65 536 bodies scheme {scheme}")
            assert got[1][0] > 0 and got[1][2] > 0


# ------------------------------------------------------------------------------------------------ 4. handle states
def test_hermite_with_block_steps_and_no_trace_there(gpu):
    """the bodies are the held (x0, v0), what get_points reports; derivatives, levels and later steps are a twin's that never called"""
    nb = gpu
    rec = nb.plummer(257, seed=5, f64=True)
    st = settings(dt=1.0 / 64)
    with make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as sim, make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as never:
        sim.steps(3)
        never.steps(3)
        now = never.get_points()
        for scheme in ref.SCHEMES:
            for which in (ref.MASS, ref.MOMENTUM_X, ref.MV2):
                ref.same_bits(dep(sim, "16^3", scheme, which), restated(now, "16^3", scheme, which), f"hermite scheme {scheme} quantity {which}")
        assert len(sim.jerk()) == 257 and len(sim.levels()) == 257   # the held derivatives and the levels are still valid
        sim.steps(3)
        never.steps(3)
        same_records(sim.get_points(), never.get_points(), "three steps later")
        assert sim.jerk().tobytes() == never.jerk().tobytes() and np.array_equal(sim.levels(), never.levels())
        assert sim.block_step_counts() == never.block_step_counts()


def test_tracers_and_the_external_field_play_no_part(gpu):
    nb = gpu
    rec = world("n257", False)
    tracers = nb.plummer(100, seed=6)
    with make(nb, rec, width=64.0) as sim:
        sim.set_tracers(tracers)
        sim.external_field = [nb.external_component(nb.EXT_PLUMMER, (2.0, 1.5), (0.5, 0.0, 0.0))]
        before = sim.get_tracers()
        for scheme in ref.SCHEMES:
            ref.same_bits(dep(sim, "16^3", scheme), expected("n257", False, ref.MASS, "16^3", scheme, False), f"scheme {scheme}")
        assert len(before) == 100 and sim.get_tracers().tobytes() == before.tobytes()


@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_right_after_a_retain_inside_unsynchronised_steps(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies inside steps(k) and no nbody_count follows: the launches are sized from
    the stale upper bound and the live count is read on the device"""
    nb = gpu
    n = 700
    rec = nb.plummer(n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = {s: dep(sim, "5x3x2", s) for s in ref.SCHEMES}   # (no count before them)
        now = twin.get_points()
        assert 0 < len(now) < n - 10
        for s in ref.SCHEMES:
            ref.same_bits(got[s], restated(now, "5x3x2", s), f"after a retain, scheme {s}")
            assert int(got[s][1].sum()) == len(now)
        same_records(sim.get_points(), now, "the state after the calls")


# ------------------------------------------------------------------------------------------------ 5. no trace
@pytest.mark.parametrize("method", ["bf", "bh"])
def test_no_trace_in_state_stats_or_later_steps(gpu, method):
    nb = gpu
    rec = world("plummer4099", False)

    def state(sim):
        s = sim.stats()
        return sim.get_points(), (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)

    with make(nb, rec, method, width=64.0) as sim, make(nb, rec, method, width=64.0) as never:
        sim.steps(2)
        never.steps(2)
        for plan in ((1, 1, 0), (0, 0, 0), (1, 1, 1)):
            set_plan(sim, plan)
            for scheme in ref.SCHEMES:
                dep(sim, "16^3", scheme, ref.MV2, True)
        set_plan(sim, (1, 1, 1))
        for when in ("right after the calls", "three steps later"):
            a, b = state(sim), state(never)
            same_records(a[0], b[0], when)
            assert a[1] == b[1], when
            sim.steps(3)
            never.steps(3)


# ------------------------------------------------------------------------------------------------ 6. capacity and refusals
def test_capacity_and_refusals(gpu):
    nb = gpu
    rec = world("n257", False)
    with make(nb, rec, width=64.0) as sim:
        spec = nb.grid_spec((-2, -2, -2), 0.25, (16, 16, 16))
        grid = np.full(4096, 7.0)
        counts = np.zeros(4, np.uint64)
        assert nb.lib.nbody_deposit(sim._h, C.byref(spec), grid.ctypes.data, 4095, counts.ctypes.data) == nb.NBODY_ERR_CAPACITY
        assert (grid == 7.0).all() and b"nbody_deposit" in nb.lib.nbody_last_error(sim._h)
        assert nb.lib.nbody_deposit(sim._h, C.byref(spec), None, 0, counts.ctypes.data) == nb.NBODY_OK   # grid == NULL: only counts
        assert [int(v) for v in counts] == [int(v) for v in restated(rec, "16^3", ref.CIC)[1]]
        assert nb.lib.nbody_deposit(sim._h, C.byref(spec), grid.ctypes.data, 4096, None) == nb.NBODY_OK   # counts == NULL
        assert grid.tobytes() == restated(rec, "16^3", ref.CIC)[0].tobytes()
        assert nb.lib.nbody_deposit(sim._h, None, grid.ctypes.data, 4096, None) == nb.NBODY_ERR_INVALID
        bad = [dict(origin=(np.nan, 0, 0)), dict(spacing=0.0), dict(spacing=np.inf), dict(dims=(0, 2, 2)), dict(dims=(1024, 1024, 129)),
               dict(scheme=3), dict(quantity=6), dict(quantity=-1), dict(project_axis=3), dict(project_axis=0)]
        for kw in bad:
            args = dict(dict(origin=(0.0, 0.0, 0.0), spacing=1.0, dims=(2, 2, 2)), **kw)
            s = nb.grid_spec(**args)
            assert nb.lib.nbody_deposit(sim._h, C.byref(s), grid.ctypes.data, 4096, None) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_deposit" in nb.lib.nbody_last_error(sim._h), kw
        s = nb.grid_spec((0, 0, 0), 1.0, (2, 2, 2))
        s.reserved = 5
        assert nb.lib.nbody_deposit(sim._h, C.byref(s), grid.ctypes.data, 4096, None) == nb.NBODY_ERR_INVALID
        with pytest.raises(nb.NbodyError):
            sim.deposit((0, 0, 0), 1.0, (2, 2, 2), scheme=9)


def test_multi_rank_and_spatial_handles_are_refused(gpu):
    nb = gpu
    rec = world("n257", False)
    spec = nb.grid_spec((-2, -2, -2), 0.25, (16, 16, 16))
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, 64.0, **kw) as sim:
            grid = np.full(4096, 7.0)
            counts = np.full(4, 99, np.uint64)
            out = (C.c_uint64 * 4)(9, 9, 9, 9)
            assert nb.lib.nbody_deposit(sim._h, C.byref(spec), grid.ctypes.data, 4096, counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_deposit:" in nb.lib.nbody_last_error(sim._h), kw
            assert (grid == 7.0).all() and (counts == 99).all(), "a refused call writes nothing"
            assert nb.lib.nbody_deposit(sim._h, C.byref(spec), None, 0, None) == nb.NBODY_ERR_INVALID, kw   # counts only: refused as well
            assert nb.lib.nbody_deposit_stats(sim._h, out) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_deposit_stats:" in nb.lib.nbody_last_error(sim._h) and list(out) == [9, 9, 9, 9], kw


# ------------------------------------------------------------------------------------------------ 7. the command line and the mirror
def test_the_command_line_option(gpu):
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        for name, scheme in (("ngp", nb.DEPOSIT_NGP), ("cic", nb.DEPOSIT_CIC), ("tsc", nb.DEPOSIT_TSC)):
            out = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--deposit", f"{name}:16:2"],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            grid, counts = sim.deposit((-2.0, -2.0, -2.0), 0.25, (16, 16, 16), scheme=scheme)
            m = re.search(r"^Deposit: scheme (\d) dims 16 16 16 spacing (\S+) inside (\d+) partial (\d+) outside (\d+) skipped (\d+)$", out.stdout, flags=re.M)
            assert m, out.stdout
            assert int(m.group(1)) == scheme and float(m.group(2)) == 0.25 and [int(m.group(k)) for k in (3, 4, 5, 6)] == [int(v) for v in counts]
            m = re.search(r"^Deposit sum (\S+) max (\S+) at (\d+) (\d+) (\d+)$", out.stdout, flags=re.M)
            assert m, out.stdout
            total = 0.0
            for v in grid.reshape(-1):   # the cells in order, as the tool adds them
                total += float(v)
            top = np.unravel_index(int(np.argmax(grid)), grid.shape)
            assert float(m.group(1)) == total and float(m.group(2)) == grid[top] and tuple(int(m.group(k)) for k in (3, 4, 5)) == top
    assert subprocess.run([cli, "--deposit", "pcs:16:2"], capture_output=True, text=True, timeout=60).returncode == 2


def test_the_mirror_s_shapes(gpu):
    nb = gpu
    with make(nb, world("n257", True), width=64.0) as sim:
        grid, counts = sim.deposit((-2, -2, 0), 0.125, (32, 32, 1), scheme=nb.DEPOSIT_TSC, quantity=nb.DEPOSIT_NUMBER, project_axis=2)
        assert grid.shape == (32, 32, 1) and grid.dtype == np.float64 and counts.shape == (4,) and counts.dtype == np.uint64
        assert abs(grid.sum() - (counts[0] + counts[1])) < 257   # NUMBER: every body inside carries weight 1
        grid, counts = sim.deposit((-2, -2, -2), 4.0, (1, 1, 1), scheme=nb.DEPOSIT_NGP, periodic=True)
        assert grid.shape == (1, 1, 1) and counts[0] == 257
