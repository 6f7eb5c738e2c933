"""nbody_pm_field and nbody_pm_field_at on the device (include/nbody_hip.h, "particle-mesh field") against nbody_host_pm_field,
byte for byte: acc, phi, cls and the eight counts on both dtypes, both methods and a device-tree handle; every plan of the knobs
gives the same bytes and the stats tell the plans apart; the fused call against the three device calls on the same handle; caller
points, an empty handle; no trace; right after a retain; Hermite; tracers and the external field; capacity and refusals; the
command line and the mirrors.  That the host call is the composition of the three restatements is asserted on the CPU in
tests/test_pm_checker.py."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import pm_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 4.0e3
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
ALL_WORLDS = ("n1", "n63", "n64", "n65", "n257", "w4099")
ALL_GRIDS = ref.CPU_GRIDS + ("i32x32x32",)
#: (world, its grids) of test 1: every world on every grid above, and the grids whose ignored axis is x or y under their own world
WORLD_GRIDS = tuple((w, ALL_GRIDS) for w in ALL_WORLDS) + ((ref.AXIS_WORLD, ref.AXIS_GRIDS),)
PHI_NULL = (("p16x8x4", ref.TSC, ref.GRADIENT4), ("i8x4x2", ref.NGP, ref.GRADIENT2), ("i16x16x1_z", ref.CIC, ref.GRADIENT2))
AXIS_PHI_NULL = (("i1x8x8_x", ref.TSC, ref.GRADIENT4), ("p1x8x8_x", ref.CIC, ref.GRADIENT2), ("p8x1x8_y", ref.NGP, ref.GRADIENT2),
                 ("i8x1x8_y", ref.CIC, ref.GRADIENT4))
KNOBS = ("pm_gather", "pm_share_sort", "deposit_sort", "sample_sort", "poisson_lds", "sample_pregrad")
G = 1.25


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


def poisson_of(grid_name, gradient):
    if ref.GRIDS[grid_name][3]:
        return dict(green=ref.DIFF2, deconvolve=0, soften=0.0) if gradient == ref.GRADIENT2 else dict(green=ref.SPECTRAL, deconvolve=1, soften=0.0)
    return dict(green=0, deconvolve=0, soften=0.0 if gradient == ref.GRADIENT2 else 0.05)


def host(rec, grid_name, scheme, gradient, points=None):
    """what nbody_host_pm_field gives for the records' bodies (widened exactly)"""
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid_name]
    xyz, m = ref.bodies(rec)
    return _nb().host_pm_field(xyz, m, origin, spacing, dims, G, scheme, gradient, periodic, project_axis=axis, points=points,
                               **poisson_of(grid_name, gradient))


@functools.lru_cache(maxsize=None)
def expected(world_name, f64, grid_name, scheme, gradient):
    """computed once and left unchanged"""
    return host(world(world_name, f64), grid_name, scheme, gradient)


def field(sim, grid_name, scheme, gradient, points=None, phi=True):
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid_name]
    return sim.pm_field(origin, spacing, dims, G, scheme, gradient, periodic, project_axis=axis, points=points, phi=phi, **poisson_of(grid_name, gradient))


def same_call(got, want, what):
    ref.same_bits(got[0], want[0], f"{what}: acc")
    if got[1] is not None:
        ref.same_bits(got[1], want[1], f"{what}: phi")
    assert got[2].tobytes() == want[2].tobytes(), f"{what}: cls"
    assert [int(v) for v in got[3]] == [int(v) for v in want[3]], f"{what}: counts {got[3]} vs {want[3]}"


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def same_classes(got, want, what):
    """every class the host call reports appears on the device, among the deposit's counts, the rows' counts and the rows (that
    AXIS_WORLD meets every class there is on the isolated grids of AXIS_GRIDS is asserted on the CPU: tests/test_pm_checker.py)"""
    for k in range(4):
        assert int(want[3][k]) == 0 or int(got[3][k]) > 0, f"{what}: class {k} of the deposit is missing"
        assert int(want[3][4 + k]) == 0 or (int(got[3][4 + k]) > 0 and (got[2] == k).any()), f"{what}: class {k} of the rows is missing"


def set_plan(sim, plan):
    for knob, v in zip(KNOBS, plan):
        sim.set_tuning(knob, v)


# ------------------------------------------------------------------------------------------------ 1. the host call's bytes
@DTYPES
@pytest.mark.parametrize("name,grids", WORLD_GRIDS, ids=[w for w, _ in WORLD_GRIDS])
def test_acc_phi_cls_and_counts_are_the_host_call_s_byte_for_byte(gpu, name, grids, f64):
    nb = gpu
    rec = world(name, f64)
    n = len(rec)
    with make(nb, rec) as sim:
        for grid, scheme, gradient in itertools.product(grids, ref.SCHEMES, ref.GRADIENTS):
            what = f"{name} {grid} scheme {scheme} gradient {gradient}"
            got = field(sim, grid, scheme, gradient)
            want = expected(name, f64, grid, scheme, gradient)
            same_call(got, want, what)
            same_classes(got, want, what)
            assert got[0].shape == (n, 3) and got[1].shape == (n,) and int(got[3][:4].sum()) == n and int(got[3][4:].sum()) == n, what
            if ref.GRIDS[grid][4] >= 0:   # nothing along the ignored axis: +0.0 on every row
                along = got[0][:, ref.GRIDS[grid][4]]
                assert not along.any() and not np.signbit(along).any(), what
        # phi NULL, cls and counts NULL
        for grid, scheme, gradient in (AXIS_PHI_NULL if grids is ref.AXIS_GRIDS else PHI_NULL):
            want = expected(name, f64, grid, scheme, gradient)
            got = field(sim, grid, scheme, gradient, phi=False)
            assert got[1] is None
            same_call(got, want, f"{name} {grid}: phi NULL")
            origin, spacing, dims, periodic, axis = ref.GRIDS[grid]
            spec = nb.grid_spec(origin, spacing, dims, scheme, nb.DEPOSIT_MASS, periodic, axis)
            pm = nb.pm_spec(G, gradient, **poisson_of(grid, gradient))
            acc, phi = np.zeros((n, 3)), np.zeros(n)
            assert nb.lib.nbody_pm_field(sim._h, C.byref(spec), C.byref(pm), acc.ctypes.data, phi.ctypes.data, None, n, None, None) == nb.NBODY_OK
            ref.same_bits(acc, want[0], "cls, n_out and counts NULL: acc")
            ref.same_bits(phi, want[1], "cls, n_out and counts NULL: phi")
        same_records(sim.get_points(), rec, "a read-only call")


@pytest.mark.parametrize("method,f64", [("bf", True), ("bh", False)], ids=["bf-f64", "bh-f32"])
def test_both_methods_and_a_device_tree_handle(gpu, method, f64):
    nb = gpu
    rec = nb.plummer(4099, seed=7, f64=f64)
    with make(nb, rec, method=method, width=64.0) as sim:
        sim.steps(2)
        now = sim.get_points()
        for grid, scheme, gradient in itertools.product(("p16x8x4", "i32x32x32"), ref.SCHEMES, ref.GRADIENTS):
            same_call(field(sim, grid, scheme, gradient), host(now, grid, scheme, gradient), f"{method} {grid} scheme {scheme} gradient {gradient}")


# ------------------------------------------------------------------------------------------------ 2. the plan does not show
def plans():
    out = []
    for gather, share, dsort, ssort, lds in itertools.product((1, 0), repeat=5):
        for pregrad in ((0,) if gather else (0, 1)):
            out.append((gather, share, dsort, ssort, lds, pregrad))
    return out


@DTYPES
def test_every_plan_gives_the_same_bytes_and_the_stats_tell_them_apart(gpu, f64):
    nb = gpu
    name = "w4099"
    rec = world(name, f64)
    # the grids whose ignored axis is x or y, under their own world: every scheme and both gradients under every plan
    with make(nb, world(ref.AXIS_WORLD, f64)) as sim:
        for grid, scheme, gradient in itertools.product(ref.AXIS_GRIDS, ref.SCHEMES, ref.GRADIENTS):
            want = expected(ref.AXIS_WORLD, f64, grid, scheme, gradient)
            reads = {}
            for plan in plans():
                set_plan(sim, plan)
                what = f"{grid} scheme {scheme} gradient {gradient} plan {plan}"
                got = field(sim, grid, scheme, gradient)
                same_call(got, want, what)
                same_classes(got, want, what)
                gather, share, dsort, ssort, lds, pregrad = plan
                shared = share and dsort and ssort
                stats = [int(v) for v in sim.pm_field_stats()]
                assert stats[0] == 1 and stats[1] == (gather | (2 if shared else 0)), (what, stats)
                assert stats[3] == (1 if shared else dsort + ssort), (what, stats)
                reads.setdefault((gather, pregrad), set()).add(stats[2])
                if plan[1:] == (1, 1, 1, 1, 0):   # phi NULL under both gathers
                    same_call(field(sim, grid, scheme, gradient, phi=False), want, f"{what}: phi NULL")
            assert all(len(v) == 1 for v in reads.values()), reads
            assert 0 < min(reads[(1, 0)]) <= min(reads[(0, 0)]), reads
    with make(nb, rec) as sim:
        assert [sim.get_tuning(k) for k in KNOBS] == [1, 1, 1, 1, 1, 0]
        for grid, scheme, gradient in (("p16x8x4", ref.TSC, ref.GRADIENT2), ("i32x32x32", ref.CIC, ref.GRADIENT4), ("i16x16x1_z", ref.NGP, ref.GRADIENT2),
                                       ("i8x4x2", ref.TSC, ref.GRADIENT4)):
            want = expected(name, f64, grid, scheme, gradient)
            live = int(want[3][4:7].sum())   # the points that are not skipped
            reads = {}
            for plan in plans():
                set_plan(sim, plan)
                what = f"{grid} scheme {scheme} gradient {gradient} plan {plan}"
                same_call(field(sim, grid, scheme, gradient), want, what)
                gather, share, dsort, ssort, lds, pregrad = plan
                shared = share and dsort and ssort
                stats = [int(v) for v in sim.pm_field_stats()]
                assert stats[0] == 1 and stats[1] == (gather | (2 if shared else 0)), (what, stats)
                assert stats[3] == (1 if shared else dsort + ssort), (what, stats)   # one sort against two
                reads.setdefault((gather, pregrad), set()).add(stats[2])
            assert all(len(v) == 1 for v in reads.values()), reads   # the reads depend on the gather's plan alone
            fused, two = min(reads[(1, 0)]), min(reads[(0, 0)])
            assert 0 < fused <= two, reads   # the fused gather reads no more than the gradient launch plus the value launch
            if grid == "p16x8x4":   # periodic TSC order 2: 5 x 9 cells a component, and phi rides on the x component's
                assert fused == 135 * live and two == (135 + 27) * live, (reads, live)
            if grid == "i16x16x1_z":   # NGP: the own cell is one read more than the differences'
                phi_less = field(sim, grid, scheme, gradient, phi=False)
                same_call(phi_less, want, "phi NULL")
        set_plan(sim, (1, 1, 1, 1, 1, 0))
        field(sim, "p16x8x4", ref.TSC, ref.GRADIENT2, phi=False)
        assert int(sim.pm_field_stats()[2]) == 135 * int(expected(name, f64, "p16x8x4", ref.TSC, ref.GRADIENT2)[3][4:7].sum())


# ------------------------------------------------------------------------------------------------ 3. the three device calls
@DTYPES
def test_the_fused_call_is_deposit_poisson_and_two_samples_on_the_same_handle(gpu, f64):
    nb = gpu
    rec = world("w4099", f64)
    with make(nb, rec) as sim:
        for grid, scheme, gradient in itertools.product(("p8x8x8", "i32x32x32", "i16x16x1_z"), ref.SCHEMES, ref.GRADIENTS):
            origin, spacing, dims, periodic, axis = ref.GRIDS[grid]
            kw = poisson_of(grid, gradient)
            mass, c_dep = sim.deposit(origin, spacing, dims, scheme=scheme, periodic=periodic, project_axis=axis)
            pot = sim.grid_poisson(mass, spacing, G, periodic, kw["green"], kw["soften"], kw["deconvolve"], scheme)
            grad, cls, c_smp = sim.grid_sample(pot, origin, spacing, scheme=scheme, op=gradient, periodic=periodic, project_axis=axis)
            val = sim.grid_sample(pot, origin, spacing, scheme=scheme, op=nb.SAMPLE_VALUE, periodic=periodic, project_axis=axis)[0][:, 0]
            same_call(field(sim, grid, scheme, gradient), (0.0 - grad, val, cls, np.concatenate([c_dep, c_smp])),
                      f"{grid} scheme {scheme} gradient {gradient}")


# ------------------------------------------------------------------------------------------------ 4. caller points
@pytest.mark.parametrize("n_bodies", [0, 257])
def test_caller_points(gpu, n_bodies):
    nb = gpu
    rec = world("n257", True)[:n_bodies]
    with make(nb, rec) as sim:
        before = sim.get_points()
        for grid, scheme, gradient in itertools.product(ALL_GRIDS, ref.SCHEMES, ref.GRADIENTS):
            pts = ref.caller_points(grid, 300)
            for m in (0, 1, 300):
                what = f"{n_bodies} bodies {m} points {grid} scheme {scheme} gradient {gradient}"
                got = field(sim, grid, scheme, gradient, points=pts[:m])
                want = host(rec, grid, scheme, gradient, points=pts[:m])
                same_call(got, want, what)
                assert got[0].shape == (m, 3) and int(got[3][:4].sum()) == n_bodies and int(got[3][4:].sum()) == m, what
                if not n_bodies:   # a handle that holds no body: every output is +0.0
                    assert not got[0].any() and not got[1].any() and not np.signbit(got[0]).any() and not np.signbit(got[1]).any(), what
            if not ref.GRIDS[grid][3]:   # points off the grid: the classes and counts are the sampler's
                assert got[3][5] + got[3][6] > 0 and got[3][7] == 1, (grid, got[3])
                smp = sim.grid_sample(np.zeros(ref.GRIDS[grid][2]), ref.GRIDS[grid][0], ref.GRIDS[grid][1], scheme=scheme, op=gradient,
                                      project_axis=ref.GRIDS[grid][4], points=pts)
                assert got[2].tobytes() == smp[1].tobytes() and [int(v) for v in got[3][4:]] == [int(v) for v in smp[2]], grid
        same_records(sim.get_points(), before, "the state after the calls")
        for plan in plans()[::5]:   # the plans on points as well
            set_plan(sim, plan)
            pts = ref.caller_points("i32x32x32", 300)
            same_call(field(sim, "i32x32x32", ref.TSC, ref.GRADIENT4, points=pts), host(rec, "i32x32x32", ref.TSC, ref.GRADIENT4, points=pts), f"plan {plan}")
            stats = [int(v) for v in sim.pm_field_stats()]
            assert stats[1] == plan[0] and stats[3] == (plan[2] if n_bodies else 0) + plan[3], (plan, stats)   # bodies and points sort apart


# ------------------------------------------------------------------------------------------------ 5. read-only
@pytest.mark.parametrize("method", ["bf", "bh"])
def test_no_trace_in_state_stats_older_records_or_later_steps(gpu, method):
    nb = gpu
    rec = nb.plummer(4099, seed=7)
    pts = np.random.default_rng(8).uniform(-2.0, 2.0, (300, 3))

    def state(sim):
        s = sim.stats()
        return sim.get_points(), (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)

    def records(sim):
        return [[int(v) for v in f()] for f in (sim.deposit_stats, sim.grid_sample_stats, sim.grid_poisson_stats)]

    with make(nb, rec, method, width=64.0) as sim, make(nb, rec, method, width=64.0) as never:
        sim.steps(2)
        never.steps(2)
        assert records(sim) == [[0, 0, 0, 0]] * 3 and [int(v) for v in sim.pm_field_stats()] == [0, 0, 0, 0]
        for plan in plans()[::7]:
            set_plan(sim, plan)
            for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
                field(sim, "p16x8x4", scheme, gradient)
                field(sim, "i32x32x32", scheme, gradient, points=pts)
        assert records(sim) == [[0, 0, 0, 0]] * 3, "the three older records are untouched"
        assert int(sim.pm_field_stats()[0]) == 1
        # ... and they keep what their own calls left
        mass, _ = sim.deposit((-2, -2, -2), 0.25, (16, 16, 16))
        sim.grid_sample(mass, (-2, -2, -2), 0.25, op=nb.SAMPLE_GRADIENT2)
        sim.grid_poisson(mass, 0.25, 1.0)
        older = records(sim)
        field(sim, "p16x8x4", ref.TSC, ref.GRADIENT4)
        assert records(sim) == older and all(r[0] == 1 for r in older)
        set_plan(sim, (1, 1, 1, 1, 1, 0))
        for when in ("right after the calls", "three steps later"):
            a, b = state(sim), state(never)
            same_records(a[0], b[0], when)
            assert a[1] == b[1], when
            sim.steps(3)
            never.steps(3)


@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_right_after_a_retain_inside_unsynchronised_steps(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies inside steps(k) and no nbody_count follows: the launches are sized from
    the stale upper bound, the live count is read on the device, rows and n_out are the live bodies'"""
    nb = gpu
    n = 700
    rec = nb.plummer(n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    cases = [("p8x8x8", ref.TSC, ref.GRADIENT2), ("i8x4x2", ref.CIC, ref.GRADIENT4), ("i32x32x32", ref.NGP, ref.GRADIENT2)]
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = [field(sim, *c) for c in cases]   # (no count before them)
        set_plan(sim, (0, 0, 1, 1, 1, 1))
        got += [field(sim, *c) for c in cases]
        now = twin.get_points()
        assert 0 < len(now) < n - 10
        for c, g in zip(cases + cases, got):
            same_call(g, host(now, *c), f"after a retain, {c}")
            assert len(g[0]) == len(now) and int(g[3][4:].sum()) == len(now)
        same_records(sim.get_points(), now, "the state after the calls")


def test_hermite_with_block_steps_and_no_trace_there(gpu):
    """the bodies are the held (x0, v0), what get_points reports; derivatives, levels and later steps are a twin's that never called"""
    nb = gpu
    rec = nb.plummer(257, seed=5, f64=True)
    st = settings(dt=1.0 / 64)
    with make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as sim, make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as never:
        sim.steps(3)
        never.steps(3)
        now = never.get_points()
        for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
            same_call(field(sim, "i32x32x32", scheme, gradient), host(now, "i32x32x32", scheme, gradient), f"hermite scheme {scheme} gradient {gradient}")
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
        for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
            same_call(field(sim, "p16x8x4", scheme, gradient), expected("n257", False, "p16x8x4", scheme, gradient), f"scheme {scheme} gradient {gradient}")
        at = np.ascontiguousarray(before["position"], np.float64)
        same_call(field(sim, "i32x32x32", ref.CIC, ref.GRADIENT2, points=at), host(rec, "i32x32x32", ref.CIC, ref.GRADIENT2, points=at), "at the tracers")
        assert len(before) == 100 and sim.get_tracers().tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ 6. capacity and refusals
def test_capacity_and_refusals(gpu):
    nb = gpu
    rec = world("n257", False)
    with make(nb, rec, width=64.0) as sim:
        def good_spec(**kw):
            a = dict(origin=(-2.0, -2.0, -2.0), spacing=0.5, dims=(8, 8, 8), scheme=ref.CIC, quantity=nb.DEPOSIT_MASS, periodic=True, project_axis=-1)
            a.update(kw)
            return nb.grid_spec(**a)

        def bad_pm(**kw):
            pm = nb.pm_spec(1.0, ref.GRADIENT2)
            for k, v in kw.items():
                if k == "reserved":
                    pm.reserved[v] = 1
                elif k == "gradient":
                    pm.gradient = v
                else:
                    setattr(pm.poisson, k, v)
            return pm

        ok_pm = nb.pm_spec(1.0, ref.GRADIENT2)
        acc, phi = np.full((257, 3), 7.0), np.full(257, 7.0)
        cls = np.full(257, 9, np.uint8)
        counts = np.full(8, 99, np.uint64)
        n = C.c_size_t(0)
        pts = np.zeros((2, 3))

        def call(spec=good_spec(), pm=ok_pm, a=acc, cap=257):
            return nb.lib.nbody_pm_field(sim._h, None if spec is None else C.byref(spec), None if pm is None else C.byref(pm),
                                         None if a is None else a.ctypes.data, phi.ctypes.data, cls.ctypes.data, cap, C.byref(n), counts.ctypes.data)

        def call_at(spec=good_spec(), pm=ok_pm, a=acc, p=pts, m=2):
            return nb.lib.nbody_pm_field_at(sim._h, None if spec is None else C.byref(spec), None if pm is None else C.byref(pm),
                                            None if p is None else p.ctypes.data, m, None if a is None else a.ctypes.data, phi.ctypes.data,
                                            cls.ctypes.data, counts.ctypes.data)

        assert call(cap=256) == nb.NBODY_ERR_CAPACITY and n.value == 257
        assert b"nbody_pm_field" in nb.lib.nbody_last_error(sim._h)
        n.value = 5
        bad = [dict(spec=None), dict(pm=None), dict(a=None)]
        bad += [dict(spec=good_spec(**kw)) for kw in (dict(origin=(np.nan, 0, 0)), dict(spacing=0.0), dict(dims=(0, 8, 8)), dict(dims=(8, 6, 8)),
                                                      dict(scheme=3), dict(project_axis=3), dict(project_axis=0), dict(quantity=nb.DEPOSIT_NUMBER),
                                                      dict(quantity=nb.DEPOSIT_MV2), dict(quantity=9), dict(periodic=False, dims=(4096, 8, 8)))]
        bad += [dict(pm=bad_pm(**kw)) for kw in (dict(g=np.inf), dict(soften=0.1), dict(green=2), dict(deconvolve=3), dict(gradient=nb.SAMPLE_VALUE),
                                                 dict(gradient=3), dict(reserved=0), dict(reserved=1), dict(reserved=2))]
        bad += [dict(spec=good_spec(periodic=False), pm=bad_pm(green=1)), dict(spec=good_spec(periodic=False), pm=bad_pm(soften=-1.0))]
        for kw in bad:
            assert call(**kw) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_pm_field:" in nb.lib.nbody_last_error(sim._h), kw
            if "a" not in kw:
                assert call_at(**kw) == nb.NBODY_ERR_INVALID, kw
                assert b"nbody_pm_field_at:" in nb.lib.nbody_last_error(sim._h), kw
        assert call_at(p=None) == nb.NBODY_ERR_INVALID and call_at(a=None) == nb.NBODY_ERR_INVALID and call_at(m=2 ** 31) == nb.NBODY_ERR_INVALID
        assert b"nbody_pm_field_at:" in nb.lib.nbody_last_error(sim._h)
        assert (acc == 7.0).all() and (phi == 7.0).all() and (cls == 9).all() and (counts == 99).all(), "a refused call writes nothing"
        assert n.value in (5, 257)   # (acc NULL is found after the live count is known)
        assert [int(v) for v in sim.pm_field_stats()] == [0, 0, 0, 0]
        assert nb.lib.nbody_pm_field_stats(sim._h, None) == nb.NBODY_ERR_INVALID
        with pytest.raises(nb.NbodyError):
            sim.pm_field((-2, -2, -2), 0.5, (8, 8, 8), 1.0, gradient=nb.SAMPLE_VALUE)
    with make(nb, rec[:0]) as sim:   # no body: NBODY_OK, counts zeroed, nothing else written
        spec, pm = nb.grid_spec((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), periodic=True), nb.pm_spec(1.0, ref.GRADIENT2)
        acc, counts, n = np.full((4, 3), 7.0), np.full(8, 99, np.uint64), C.c_size_t(5)
        assert nb.lib.nbody_pm_field(sim._h, C.byref(spec), C.byref(pm), acc.ctypes.data, None, None, 4, C.byref(n), counts.ctypes.data) == nb.NBODY_OK
        assert n.value == 0 and not counts.any() and (acc == 7.0).all()
        assert nb.lib.nbody_pm_field(sim._h, C.byref(spec), C.byref(pm), None, None, None, 0, None, None) == nb.NBODY_OK


def test_multi_rank_and_spatial_handles_are_refused(gpu):
    nb = gpu
    rec = world("n257", False)
    spec, pm = nb.grid_spec((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), periodic=True), nb.pm_spec(1.0, ref.GRADIENT2)
    pts = np.zeros((2, 3))
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, 64.0, **kw) as sim:
            acc = np.full((257, 3), 7.0)
            counts = np.full(8, 99, np.uint64)
            stats = (C.c_uint64 * 4)(9, 9, 9, 9)
            n = C.c_size_t(5)
            assert nb.lib.nbody_pm_field(sim._h, C.byref(spec), C.byref(pm), acc.ctypes.data, None, None, 257, C.byref(n),
                                         counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_pm_field:" in nb.lib.nbody_last_error(sim._h), kw
            assert nb.lib.nbody_pm_field_at(sim._h, C.byref(spec), C.byref(pm), pts.ctypes.data, 2, acc.ctypes.data, None, None,
                                            counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_pm_field_at:" in nb.lib.nbody_last_error(sim._h), kw
            assert (acc == 7.0).all() and (counts == 99).all() and n.value == 5, "a refused call writes nothing"
            assert nb.lib.nbody_pm_field_stats(sim._h, stats) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_pm_field_stats:" in nb.lib.nbody_last_error(sim._h) and list(stats) == [9, 9, 9, 9], kw


# ------------------------------------------------------------------------------------------------ 7. the command line and the mirrors
def test_the_command_line_option(gpu):
    """nbody_cli goes through the C++ mirror (host/simulation.hpp pm_field): its rows are the Python mirror's"""
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        for arg, periodic, green, gradient in (("isolated:grad2", False, 0, nb.SAMPLE_GRADIENT2), ("diff2:grad2", True, nb.POISSON_DIFF2, nb.SAMPLE_GRADIENT2),
                                               ("spectral:grad4", True, nb.POISSON_SPECTRAL, nb.SAMPLE_GRADIENT4)):
            run = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--deposit", "cic:8:2",
                                  "--pm", arg], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr
            acc, phi, cls, counts = sim.pm_field((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), 1.0, nb.DEPOSIT_CIC, gradient, periodic, green)
            m = re.search(r"^PM: .* gradient (\d) g \S+ bodies (\d+) deposited (\d+) (\d+) (\d+) (\d+) sampled (\d+) (\d+) (\d+) (\d+)$", run.stdout, flags=re.M)
            assert m, run.stdout
            assert int(m.group(1)) == gradient and int(m.group(2)) == len(acc) and [int(m.group(k)) for k in range(3, 11)] == [int(v) for v in counts]
            rows = re.findall(r"^PM body (\d+) class (\d)((?: \S+)+)$", run.stdout, flags=re.M)
            assert len(rows) == 8, run.stdout
            for i, (index, kind, values) in enumerate(rows):
                assert int(index) == i and int(kind) == cls[i]
                assert np.array([float(v) for v in values.split()]).tobytes() == np.append(acc[i], phi[i]).tobytes()
    assert subprocess.run([cli, "--deposit", "cic:8:2", "--pm", "isolated:grad3"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([cli, "--pm", "isolated:grad2"], capture_output=True, text=True, timeout=60).returncode == 2


def test_the_mirror_s_shapes(gpu):
    nb = gpu
    with make(nb, world("n257", True), width=64.0) as sim:
        acc, phi, cls, counts = sim.pm_field((-2, -2, 0), 0.25, (16, 16, 1), 1.0, scheme=nb.DEPOSIT_TSC, project_axis=2)
        assert acc.shape == (257, 3) and acc.dtype == np.float64 and phi.shape == (257,) and phi.dtype == np.float64
        assert cls.shape == (257,) and cls.dtype == np.uint8 and counts.shape == (8,) and counts.dtype == np.uint64
        assert int(counts[:4].sum()) == 257 and int(counts[4:].sum()) == 257 and not acc[:, 2].any()   # nothing along the ignored axis
        assert (phi[cls == 0] < 0).all()   # an attractive potential
        acc, phi, cls, counts = sim.pm_field((-2, -2, -2), 0.5, (8, 8, 8), 1.0, periodic=True, points=np.zeros((5, 3)), phi=False)
        assert acc.shape == (5, 3) and phi is None and cls.shape == (5,) and int(counts[4]) == 5
        assert sim.pm_field_stats().shape == (4,) and sim.pm_field_stats().dtype == np.uint64
        assert C.sizeof(nb.NbodyPmSpec) == 48
