"""nbody_grid_sample and nbody_grid_sample_at on the device (include/nbody_hip.h, "grid sample") against the numpy restatement
(tests/sample_ref.py): out, cls and counts equal byte for byte on both dtypes, every world, grid, scheme and op; the four plans of
the knobs give the same bytes and the stats show the shared reads; caller points; right after a retain; handle variants; no
trace; capacity and refusals; deposit-then-sample against the same two calls on the host; the command line and the mirror.  What
makes the worlds worth looking at is asserted on the CPU in tests/test_sample_checker.py."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import sample_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER, WIDTH = (0.0, 0.0, 0.0), 4.0e9   # (holed's bodies stand up to 7.5e8 away)
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
PLANS = list(itertools.product((0, 1), (0, 1)))   # sample_sort, sample_pregrad
CASES = ((ref.VALUE, 1), (ref.VALUE, 4), (ref.GRADIENT2, 1), (ref.GRADIENT4, 1))   # (op, fields)


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
def grid_of(name, fields):
    return ref.make_grid(name, fields)


def restated(xyz, name, scheme, op, fields, periodic):
    origin, spacing, _, axis = ref.GRIDS[name]
    return ref.sample(xyz, grid_of(name, fields), origin, spacing, scheme, op, periodic, axis)


@functools.lru_cache(maxsize=None)
def expected(world_name, f64, name, scheme, op, fields, periodic):
    """(out, cls, counts) of the restatement, computed once and left unchanged"""
    return restated(ref.points(world(world_name, f64)), name, scheme, op, fields, periodic)


def samp(sim, name, scheme, op=ref.VALUE, fields=1, periodic=False, points=None):
    origin, spacing, _, axis = ref.GRIDS[name]
    return sim.grid_sample(grid_of(name, fields), origin, spacing, scheme=scheme, op=op, periodic=periodic, project_axis=axis, points=points)


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def set_plan(sim, plan):
    for knob, v in zip(("sample_sort", "sample_pregrad"), plan):
        sim.set_tuning(knob, v)


# ------------------------------------------------------------------------------------------------ 1. the restatement
@DTYPES
@pytest.mark.parametrize("name", ref.WORLDS)
def test_out_cls_and_counts_are_the_restatement_s_byte_for_byte(gpu, name, f64):
    nb = gpu
    rec = world(name, f64)
    with make(nb, rec) as sim:
        for grid, scheme, periodic, (op, fields) in itertools.product(ref.GRIDS, ref.SCHEMES, (False, True), CASES):
            what = f"{name} {grid} scheme {scheme} op {op} fields {fields} periodic {periodic}"
            got = samp(sim, grid, scheme, op, fields, periodic)
            ref.same_bits(got, expected(name, f64, grid, scheme, op, fields, periodic), what)
            assert got[0].shape == (len(rec), fields if op == ref.VALUE else 3) and int(got[2].sum()) == len(rec), what
        same_records(sim.get_points(), rec, "a read-only call")


# ------------------------------------------------------------------------------------------------ 2. the plan does not show
@DTYPES
@pytest.mark.parametrize("name", ["one_cell", "plummer4099"])
def test_every_plan_gives_the_same_bytes(gpu, name, f64):
    nb = gpu
    rec = world(name, f64)
    n = len(rec)
    with make(nb, rec) as sim:
        assert [sim.get_tuning(k) for k in ("sample_sort", "sample_pregrad")] == [1, 0]
        for grid, scheme, periodic, (op, fields) in (("16^3", ref.NGP, False, CASES[2]), ("16^3", ref.CIC, True, CASES[3]), ("16^3", ref.TSC, True, CASES[2]),
                                                     ("16^3", ref.TSC, False, CASES[3]), ("64x64x1_z", ref.TSC, False, CASES[2]),
                                                     ("5x7x3", ref.CIC, False, CASES[1]), ("4x3x4", ref.TSC, False, CASES[3])):
            want = expected(name, f64, grid, scheme, op, fields, periodic)
            reads = {}
            for plan in PLANS:
                set_plan(sim, plan)
                ref.same_bits(samp(sim, grid, scheme, op, fields, periodic), want, f"{name} {grid} scheme {scheme} op {op} plan {plan}")
                stats = sim.grid_sample_stats()
                used = plan[0] | (plan[1] if op != ref.VALUE else 0) << 1   # (the plan used: a value has no differences)
                assert stats[0] == 1 and stats[1] == used and stats[3] == 0, (plan, stats)
                reads[plan] = int(stats[2])
            assert reads[(0, 0)] == reads[(1, 0)] and reads[(0, 1)] == reads[(1, 1)], reads   # the order of the visit reads no more
            if name == "one_cell" and grid == "16^3" and scheme == ref.TSC and periodic:
                # every point inside: order 2 reads 5 cells along the axis for each of the 9 others, not 6: 135 a point, not
                # 162; from the difference grids 27 a component
                assert op == ref.GRADIENT2 and reads[(1, 0)] == 135 * n < 162 * n and reads[(1, 1)] == 81 * n, reads
        set_plan(sim, (1, 0))
        for scheme, op, per_point in ((ref.TSC, ref.GRADIENT4, 3 * 7 * 9), (ref.CIC, ref.GRADIENT2, 3 * 4 * 4), (ref.NGP, ref.GRADIENT4, 3 * 4),
                                      (ref.TSC, ref.VALUE, 27)):
            if name == "one_cell":
                samp(sim, "16^3", scheme, op, 1, True)
                assert int(sim.grid_sample_stats()[2]) == per_point * n, (scheme, op)


def test_the_difference_grids_are_not_used_past_the_cell_limit(gpu):
    """3 cells > NBODY_DEPOSIT_MAX_CELLS: sample_pregrad is treated as 0 and the stats say so (a 2^26-cell column of zeros)"""
    nb = gpu
    with make(nb, world("n65", True)) as sim:
        set_plan(sim, (1, 1))
        grid = np.zeros((1 << 26, 1, 1))
        spacing = 4.0 / (1 << 26)   # (y and z in the middle of their one cell: CIC's second cell there is off the grid)
        out, cls, counts = sim.grid_sample(grid, (-2.0, -1.0, -1.0), spacing, scheme=nb.DEPOSIT_CIC, op=nb.SAMPLE_GRADIENT2,
                                           points=np.array([[0.1, -1.0 + 0.5 * spacing, -1.0 + 0.5 * spacing], [5.0, 0.0, 0.0]]))
        assert not out.any() and [int(c) for c in cls] == [ref.PARTIAL, ref.OUTSIDE] and int(sim.grid_sample_stats()[1]) == 1


# ------------------------------------------------------------------------------------------------ 3. caller points
@pytest.mark.parametrize("n_bodies", [0, 257])
def test_caller_points(gpu, n_bodies):
    nb = gpu
    rng = np.random.default_rng(4)
    pts = rng.uniform(-2.5, 2.5, (1000, 3))
    pts[7] = (np.nan, 0.0, 0.0)
    with make(nb, world("n257", True)[:n_bodies]) as sim:
        before = sim.get_points()
        for m in (0, 1, 1000):
            for scheme, periodic, (op, fields) in itertools.product(ref.SCHEMES, (False, True), CASES):
                for grid in ("16^3", "64x64x1_z"):
                    what = f"{m} points {grid} scheme {scheme} op {op} fields {fields} periodic {periodic}"
                    got = samp(sim, grid, scheme, op, fields, periodic, points=pts[:m])
                    ref.same_bits(got, restated(pts[:m], grid, scheme, op, fields, periodic), what)
                    assert got[0].shape == (m, fields if op == ref.VALUE else 3) and int(got[2].sum()) == m, what
        same_records(sim.get_points(), before, "the handle lends its stream and its memory only")
        for plan in PLANS:   # the plans on points as well
            set_plan(sim, plan)
            ref.same_bits(samp(sim, "16^3", ref.TSC, ref.GRADIENT4, 1, False, points=pts), restated(pts, "16^3", ref.TSC, ref.GRADIENT4, 1, False), f"plan {plan}")


# ------------------------------------------------------------------------------------------------ 4. handle states
@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_right_after_a_retain_inside_unsynchronised_steps(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies inside steps(k) and no nbody_count follows: the launches are sized from
    the stale upper bound, the live count is read on the device, rows and n_out are the live bodies'"""
    nb = gpu
    n = 700
    rec = nb.plummer(n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = {(s, op): samp(sim, "5x7x3", s, op) for s in ref.SCHEMES for op in ref.OPS}   # (no count before them)
        now = twin.get_points()
        assert 0 < len(now) < n - 10
        for (s, op), g in got.items():
            ref.same_bits(g, restated(ref.points(now), "5x7x3", s, op, 1, False), f"after a retain, scheme {s} op {op}")
            assert len(g[0]) == len(now) and int(g[2].sum()) == len(now)
        same_records(sim.get_points(), now, "the state after the calls")


def test_a_device_tree_handle(gpu):
    nb = gpu
    rec = world("plummer4099", False)
    with make(nb, rec, method="bh", width=64.0) as sim:
        sim.steps(2)
        now = ref.points(sim.get_points())
        for scheme, (op, fields) in itertools.product(ref.SCHEMES, CASES):
            ref.same_bits(samp(sim, "16^3", scheme, op, fields), restated(now, "16^3", scheme, op, fields, False), f"bh scheme {scheme} op {op}")


def test_hermite_with_block_steps_and_no_trace_there(gpu):
    """the bodies are the held (x0, v0), what get_points reports; derivatives, levels and later steps are a twin's that never called"""
    nb = gpu
    rec = nb.plummer(257, seed=5, f64=True)
    st = settings(dt=1.0 / 64)
    with make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as sim, make(nb, rec, st=st, width=64.0, hermite=True, block=(0.02, 4)) as never:
        sim.steps(3)
        never.steps(3)
        now = ref.points(never.get_points())
        for scheme, op in itertools.product(ref.SCHEMES, ref.OPS):
            ref.same_bits(samp(sim, "16^3", scheme, op), restated(now, "16^3", scheme, op, 1, False), f"hermite scheme {scheme} op {op}")
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
        for scheme, op in itertools.product(ref.SCHEMES, ref.OPS):
            ref.same_bits(samp(sim, "16^3", scheme, op), expected("n257", False, "16^3", scheme, op, 1, False), f"scheme {scheme} op {op}")
        at = samp(sim, "16^3", ref.CIC, ref.GRADIENT2, points=ref.points(before))   # a field sampled at the tracers' positions
        ref.same_bits(at, restated(ref.points(before), "16^3", ref.CIC, ref.GRADIENT2, 1, False), "at the tracers")
        assert len(before) == 100 and sim.get_tracers().tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ 5. no trace
@pytest.mark.parametrize("method", ["bf", "bh"])
def test_no_trace_in_state_stats_or_later_steps(gpu, method):
    nb = gpu
    rec = world("plummer4099", False)
    pts = np.random.default_rng(8).uniform(-2.0, 2.0, (300, 3))

    def state(sim):
        s = sim.stats()
        return sim.get_points(), (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)

    with make(nb, rec, method, width=64.0) as sim, make(nb, rec, method, width=64.0) as never:
        sim.steps(2)
        never.steps(2)
        for plan in PLANS:
            set_plan(sim, plan)
            for scheme, op in itertools.product(ref.SCHEMES, ref.OPS):
                samp(sim, "16^3", scheme, op, 1, True)
                samp(sim, "16^3", scheme, op, 1, False, points=pts)
        set_plan(sim, (1, 0))
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
    grid = grid_of("16^3", 4)
    with make(nb, rec, width=64.0) as sim:
        spec = nb.grid_spec((-2, -2, -2), 0.25, (16, 16, 16))
        out = np.full((257, 4), 7.0)
        cls = np.full(257, 9, np.uint8)
        counts = np.full(4, 99, np.uint64)
        n = C.c_size_t(0)

        def call(spec=spec, g=grid, fields=1, op=0, o=out, c=cls, cap=257, cnt=counts):
            return nb.lib.nbody_grid_sample(sim._h, C.byref(spec) if spec is not None else None, g.ctypes.data if g is not None else None, fields, op,
                                            o.ctypes.data if o is not None else None, c.ctypes.data if c is not None else None, cap, C.byref(n),
                                            cnt.ctypes.data if cnt is not None else None)
        assert call(cap=256) == nb.NBODY_ERR_CAPACITY and n.value == 257
        assert (out == 7.0).all() and (cls == 9).all() and b"nbody_grid_sample" in nb.lib.nbody_last_error(sim._h)
        want = restated(ref.points(rec), "16^3", ref.CIC, ref.VALUE, 4, False)
        assert call(fields=4, c=None, cnt=None) == nb.NBODY_OK and n.value == 257 and out.tobytes() == want[0].tobytes()   # cls, counts NULL
        assert (cls == 9).all()
        assert call(fields=4) == nb.NBODY_OK and cls.tobytes() == want[1].tobytes() and [int(v) for v in counts] == [int(v) for v in want[2]]
        before = (out.copy(), cls.copy(), counts.copy())
        bad = [dict(spec=None), dict(g=None), dict(o=None), dict(fields=0), dict(fields=5), dict(fields=2, op=1), dict(op=3), dict(op=-1)]
        bad += [dict(spec=nb.grid_spec(**dict(dict(origin=(0.0, 0.0, 0.0), spacing=1.0, dims=(2, 2, 2)), **kw)))
                for kw in (dict(origin=(np.nan, 0, 0)), dict(spacing=0.0), dict(dims=(0, 2, 2)), dict(dims=(1024, 1024, 129)), dict(scheme=3),
                           dict(project_axis=3), dict(project_axis=0))]
        bad += [dict(spec=nb.grid_spec((0, 0, 0), 1.0, (1024, 1024, 64)), fields=4)]   # fields times the cells
        for kw in bad:
            assert call(**kw) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_sample" in nb.lib.nbody_last_error(sim._h), kw
        pts = np.zeros((2, 3))
        assert nb.lib.nbody_grid_sample_at(sim._h, C.byref(spec), grid.ctypes.data, 1, 0, None, 2, out.ctypes.data, None, None) == nb.NBODY_ERR_INVALID
        assert nb.lib.nbody_grid_sample_at(sim._h, C.byref(spec), grid.ctypes.data, 1, 0, pts.ctypes.data, 2, None, None, None) == nb.NBODY_ERR_INVALID
        assert b"nbody_grid_sample_at" in nb.lib.nbody_last_error(sim._h)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (out, cls, counts))), "a refused call writes nothing"
        with pytest.raises(nb.NbodyError):
            sim.grid_sample(grid[0], (0, 0, 0), 1.0, scheme=9)


def test_multi_rank_and_spatial_handles_are_refused(gpu):
    nb = gpu
    rec = world("n257", False)
    spec = nb.grid_spec((-2, -2, -2), 0.25, (16, 16, 16))
    grid = grid_of("16^3", 1)
    pts = np.zeros((2, 3))
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, 64.0, **kw) as sim:
            out = np.full((257, 3), 7.0)
            counts = np.full(4, 99, np.uint64)
            stats = (C.c_uint64 * 4)(9, 9, 9, 9)
            n = C.c_size_t(5)
            assert nb.lib.nbody_grid_sample(sim._h, C.byref(spec), grid.ctypes.data, 1, 0, out.ctypes.data, None, 257, C.byref(n),
                                            counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_sample:" in nb.lib.nbody_last_error(sim._h), kw
            assert nb.lib.nbody_grid_sample_at(sim._h, C.byref(spec), grid.ctypes.data, 1, 0, pts.ctypes.data, 2, out.ctypes.data, None,
                                               counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_sample_at:" in nb.lib.nbody_last_error(sim._h), kw
            assert (out == 7.0).all() and (counts == 99).all() and n.value == 5, "a refused call writes nothing"
            assert nb.lib.nbody_grid_sample_stats(sim._h, stats) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_sample_stats:" in nb.lib.nbody_last_error(sim._h) and list(stats) == [9, 9, 9, 9], kw


# ------------------------------------------------------------------------------------------------ 7. a closed loop
@DTYPES
def test_deposit_then_sample_is_the_host_s_byte_for_byte(gpu, f64):
    """the dyadic world of tests/test_sample_checker.py as bodies: positions on quarter cells and integer masses are exact in f32 too"""
    nb = gpu
    rng = np.random.default_rng(9)
    n = 4096
    rec = nb.plummer(n, seed=3, f64=f64)
    rec["position"] = -2.0 + 0.0625 * rng.integers(-16, 80, (n, 3))
    rec["mass"] = rng.integers(1, 17, n)
    xyz, m = ref.points(rec), np.ascontiguousarray(rec["mass"], np.float64)
    origin, spacing, dims = (-2.0, -2.0, -2.0), 0.25, (16, 16, 16)
    with make(nb, rec, width=64.0) as sim:
        for scheme, periodic in itertools.product(ref.SCHEMES, (False, True)):
            grid, counts = sim.deposit(origin, spacing, dims, scheme=scheme, periodic=periodic)
            host_grid, host_counts = nb.host_deposit(xyz, m, origin, spacing, dims, scheme=scheme, periodic=periodic)
            assert grid.tobytes() == host_grid.tobytes() and grid.any()
            for op in ref.OPS:
                got = sim.grid_sample(grid, origin, spacing, scheme=scheme, op=op, periodic=periodic)
                want = nb.host_grid_sample(xyz, host_grid, origin, spacing, scheme=scheme, op=op, periodic=periodic)
                ref.same_bits(got, want, f"scheme {scheme} op {op} periodic {periodic}")
                assert [int(v) for v in got[2]] == [int(v) for v in counts] or op != ref.VALUE


# ------------------------------------------------------------------------------------------------ 8. the command line and the mirror
def test_the_command_line_option(gpu):
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        grid, _ = sim.deposit((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), scheme=nb.DEPOSIT_CIC)
        for name, op in (("value", nb.SAMPLE_VALUE), ("grad2", nb.SAMPLE_GRADIENT2), ("grad4", nb.SAMPLE_GRADIENT4)):
            run = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--deposit", "cic:8:2",
                                  "--sample", name], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr
            out, cls, counts = sim.grid_sample(grid, (-2.0, -2.0, -2.0), 0.5, scheme=nb.DEPOSIT_CIC, op=op)
            m = re.search(r"^Sample: op (\d) bodies (\d+) inside (\d+) partial (\d+) outside (\d+) skipped (\d+)$", run.stdout, flags=re.M)
            assert m, run.stdout
            assert int(m.group(1)) == op and int(m.group(2)) == len(out) and [int(m.group(k)) for k in (3, 4, 5, 6)] == [int(v) for v in counts]
            rows = re.findall(r"^Sample body (\d+) class (\d)((?: \S+)+)$", run.stdout, flags=re.M)
            assert len(rows) == 8, run.stdout
            for i, (index, kind, values) in enumerate(rows):
                assert int(index) == i and int(kind) == cls[i]
                assert np.array([float(v) for v in values.split()]).tobytes() == out[i].tobytes()
    assert subprocess.run([cli, "--deposit", "cic:8:2", "--sample", "grad3"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([cli, "--sample", "grad2"], capture_output=True, text=True, timeout=60).returncode == 2


def test_the_mirror_s_shapes(gpu):
    nb = gpu
    with make(nb, world("n257", True), width=64.0) as sim:
        out, cls, counts = sim.grid_sample(np.ones((2, 32, 32, 1)), (-2, -2, 0), 0.125, scheme=nb.DEPOSIT_TSC, project_axis=2)
        assert out.shape == (257, 2) and out.dtype == np.float64 and cls.shape == (257,) and cls.dtype == np.uint8
        assert counts.shape == (4,) and counts.dtype == np.uint64 and int(counts.sum()) == 257
        assert np.abs(out[cls == ref.INSIDE] - 1.0).max() < 1e-15   # the weights of a point inside sum to one
        out, cls, counts = sim.grid_sample(np.full((1, 1, 1), 3.0), (-2, -2, -2), 4.0, scheme=nb.DEPOSIT_NGP, op=nb.SAMPLE_GRADIENT4, periodic=True)
        assert out.shape == (257, 3) and not out.any() and counts[0] == 257
        assert sim.grid_sample_stats().shape == (4,)
