"""nbody_p3m_field and nbody_p3m_field_at on the device (include/nbody_hip.h, "P3M field") against nbody_host_p3m_field, bit for
bit: both dtypes, both methods, both plans of p3m_lds, the three values of terms; exactly four chain cells on an axis, unequal
dims, one crowded chain cell among empty ones, bodies on the faces and periods outside the box, coincident bodies, a NaN body and
one with |u| >= 2^31, n = 0, 1 and 257; the pair counts of the stats; the read-only contract; nbody_pm_field's bits as they were.
That the host call is the numpy restatement, that its walk is complete and that it beats PM against an Ewald sum is asserted on
the CPU in tests/test_p3m_checker.py."""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import p3m_ref as ref
import pm_ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 4.0e3
G = 1.25
TERMS = (ref.BOTH, ref.MESH_ONLY, ref.SHORT_ONLY)


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


def make(nb, rec, method="bf", width=WIDTH, st=None):
    bh = method == "bh"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO, capacity=max(len(rec), 4))
    sim.settings = nb.Settings(**(st or dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5)))
    sim.init()
    return sim


def cut_of(grid, cells=4):
    spacing = ref.GRIDS[grid][1]
    r_cut = cells * spacing * (1.0 - 2.0 ** -10)
    return r_cut / 3.2, r_cut


def records_of(nb, xyz, m, f64):
    rec = nb.plummer(max(len(m), 1), seed=1, f64=f64)[: len(m)]
    rec["position"] = xyz
    rec["mass"] = m
    rec["velocity"] = 0.0
    return rec


@functools.lru_cache(maxsize=None)
def world(name, f64):
    """the records of a world in the handle's dtype (the host call then widens what the handle holds)"""
    nb = _nb()
    if name == "edge257":     # faces, periods outside, coincident bodies, a NaN body, |u| >= 2^31, a crowded corner
        xyz, m = ref.uniform_world("p16", 257, outside=True)
        lo, hi = ref.box_of("p16")
        xyz[0], xyz[1], xyz[2] = lo, hi, (lo[0], hi[1], 0.0)            # on the box's faces and corners
        xyz[3] = (0.25, -1.0, 1.75)                                      # on cell faces
        xyz[10] = xyz[11] = xyz[12] = (0.3, 0.4, -0.6)                   # coincident
        xyz[20, 1] = np.nan
        xyz[21, 0] = 0.25 * 2.0 ** 31 * 1.5                              # |u| >= 2^31
    elif name == "crowd":      # 300 bodies in one chain cell (more than two tiles of 128), 40 elsewhere: most cells are empty
        rng = np.random.default_rng(2)
        xyz = np.concatenate([rng.uniform(-0.95, -0.05, (300, 3)), ref.uniform_world("p16", 40)[0]])
        m = rng.uniform(0.5, 1.5, len(xyz)) / len(xyz)
    elif name == "wide1500":
        xyz, m = ref.uniform_world("p16x32x64", 1500, outside=True)
    elif name == "n1":
        xyz, m = np.array([[0.3, -0.2, 1.1]]), np.array([0.75])
    else:
        raise KeyError(name)
    return records_of(nb, xyz, m, f64)


CASES = {   # name -> (world, grid, (r_split, r_cut), scheme, gradient, green, deconvolve)
    "four-chain-cells": ("edge257", "p16", cut_of("p16"), ref.TSC, ref.GRADIENT4, ref.SPECTRAL, 2),
    "crowded-cell": ("crowd", "p16", (0.3, 0.9), ref.CIC, ref.GRADIENT2, ref.DIFF2, 0),
    "unequal-dims": ("wide1500", "p16x32x64", (0.1, 0.425), ref.TSC, ref.GRADIENT2, ref.SPECTRAL, 1),
    "one-body": ("n1", "p16", (0.3, 0.9), ref.CIC, ref.GRADIENT2, ref.SPECTRAL, 0),
}


def keywords(case, soften, terms, points=None):
    _, _, _, scheme, gradient, green, deconvolve = CASES[case]
    return dict(scheme=scheme, gradient=gradient, green=green, deconvolve=deconvolve, soften=soften, terms=terms, points=points)


def caller_points(grid, rec):
    pts = ref.uniform_world(grid, 97, seed=21, outside=True)[0]
    pts[3] = pm_ref.bodies(rec)[0][0]          # on a body
    pts[5, 2] = np.inf
    pts[6, 0] = 1.0e12
    return pts


@functools.lru_cache(maxsize=None)
def expected(case, f64, soften, terms, at_points):
    """computed once and left unchanged"""
    name, grid, (r_split, r_cut), *_ = CASES[case]
    rec = world(name, f64)
    xyz, m = pm_ref.bodies(rec)
    origin, spacing, dims = ref.GRIDS[grid]
    pts = caller_points(grid, rec) if at_points else None
    return _nb().host_p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, **keywords(case, soften, terms, pts))


def field(sim, case, soften, terms, points=None, phi=True):
    _, grid, (r_split, r_cut), *_ = CASES[case]
    origin, spacing, dims = ref.GRIDS[grid]
    return sim.p3m_field(origin, spacing, dims, G, r_split, r_cut, phi=phi, **keywords(case, soften, terms, points))


def same_call(got, want, what):
    ref.same_bits(got[0], want[0], f"{what}: acc")
    if got[1] is not None:
        ref.same_bits(got[1], want[1], f"{what}: phi")
    assert got[2].tobytes() == want[2].tobytes(), f"{what}: cls"
    assert [int(v) for v in got[3]] == [int(v) for v in want[3]], f"{what}: counts {got[3]} vs {want[3]}"


# ------------------------------------------------------------------------------------------------ 1. the host call's bits
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("method", ["bf", "bh"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_device_calls_are_the_host_call_bit_for_bit(gpu, case, method, f64):
    nb = gpu
    name, grid, *_ = CASES[case]
    rec = world(name, f64)
    pts = caller_points(grid, rec)
    with make(nb, rec, method) as sim:
        for lds in (1, 0):
            sim.set_tuning("p3m_lds", lds)
            for terms, soften in itertools.product(TERMS, (0.0, 0.02)):
                what = f"{case} {method} p3m_lds {lds} terms {terms} soften {soften}"
                same_call(field(sim, case, soften, terms), expected(case, f64, soften, terms, False), what + " at the bodies")
                same_call(field(sim, case, soften, terms, points=pts), expected(case, f64, soften, terms, True), what + " at points")
                assert int(sim.p3m_field_stats()[1]) & 1 == lds
        bare = field(sim, case, 0.0, ref.BOTH, phi=False)
        assert bare[1] is None
        ref.same_bits(bare[0], expected(case, f64, 0.0, ref.BOTH, False)[0], "phi NULL")


def test_a_handle_without_bodies(gpu):
    nb = gpu
    rec = world("n1", True)
    pts = caller_points("p16", rec)
    with make(nb, rec) as sim:
        sim.remove_point(0)
        acc, phi, cls, counts = field(sim, "one-body", 0.0, ref.BOTH)
        assert len(acc) == 0 and len(cls) == 0 and not counts.any()
        acc, phi, cls, counts = field(sim, "one-body", 0.0, ref.BOTH, points=pts)
        for v in (acc, phi):
            assert not v.any() and not np.signbit(v).any()
        assert int(counts[:4].sum()) == 0 and int(counts[4:].sum()) == len(pts)


# ------------------------------------------------------------------------------------------------ 2. the pair counts
@pytest.mark.parametrize("case", ["four-chain-cells", "crowded-cell"])
def test_the_stats_pair_counts_are_the_restatement_s(gpu, case):
    nb = gpu
    name, grid, (r_split, r_cut), *_ = CASES[case]
    rec = world(name, True)
    xyz, m = pm_ref.bodies(rec)
    origin, spacing, dims = ref.GRIDS[grid]
    pts = caller_points(grid, rec)
    T = nb.host_p3m_table(r_split, r_cut)
    want = {p is not None: ref.short_range(xyz, m, origin, spacing, dims, G, r_cut, 0.0, T, points=p)[1:3] for p in (None, pts)}
    assert all(w[1] > 0 for w in want.values())
    with make(nb, rec) as sim:
        assert [int(v) for v in sim.p3m_field_stats()] == [0, 0, 0, 0]
        for lds, p in itertools.product((1, 0), (None, pts)):
            sim.set_tuning("p3m_lds", lds)
            field(sim, case, 0.0, ref.BOTH, points=p)
            s = [int(v) for v in sim.p3m_field_stats()]
            assert s[0] == 1 and s[1] & 1 == lds and s[1] >> 1 == (1 if p is not None else 3)   # (pm_gather | shared order << 1)
            assert (s[2], s[3]) == want[p is not None], f"p3m_lds {lds} points {p is not None}: {s} against {want[p is not None]}"
        field(sim, case, 0.0, ref.MESH_ONLY)
        assert [int(v) for v in sim.p3m_field_stats()][2:] == [0, 0]


# ------------------------------------------------------------------------------------------------ 3. read-only
@pytest.mark.parametrize("method", ["bf", "bh"])
def test_no_trace_in_state_stats_older_records_or_later_steps(gpu, method):
    nb = gpu
    rec = nb.plummer(1031, seed=7)
    pts = np.random.default_rng(8).uniform(-2.0, 2.0, (200, 3))

    def state(sim):
        s = sim.stats()
        return sim.get_points(), (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)

    def records(sim):
        return [[int(v) for v in f()] for f in (sim.deposit_stats, sim.grid_sample_stats, sim.grid_poisson_stats, sim.pm_field_stats)]

    with make(nb, rec, method, width=64.0) as sim, make(nb, rec, method, width=64.0) as never:
        sim.steps(2)
        never.steps(2)
        assert records(sim) == [[0, 0, 0, 0]] * 4
        for lds, terms in itertools.product((1, 0), TERMS):
            sim.set_tuning("p3m_lds", lds)
            field(sim, "four-chain-cells", 0.0, terms)
            field(sim, "crowded-cell", 0.01, terms, points=pts)
        assert records(sim) == [[0, 0, 0, 0]] * 4, "the four older records are untouched"
        sim.pm_field((-2, -2, -2), 0.25, (16, 16, 16), G, periodic=True)
        older = records(sim)
        field(sim, "four-chain-cells", 0.0, ref.BOTH)
        assert records(sim) == older and older[3][0] == 1
        sim.set_tuning("p3m_lds", 1)
        for when in ("right after the calls", "three steps later"):
            a, b = state(sim), state(never)
            for f in ("position", "velocity", "acceleration", "mass"):
                assert a[0][f].tobytes() == b[0][f].tobytes(), f"{when}: {f} differs"
            assert a[1] == b[1], when
            sim.steps(3)
            never.steps(3)


@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_right_after_a_retain_inside_unsynchronised_steps(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies inside steps(k) and no nbody_count follows: the launches are sized from the
    stale upper bound, the live count is read on the device, rows and n_out are the live bodies'"""
    nb = gpu
    n = 700
    rec = nb.plummer(n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    origin, spacing, dims = ref.GRIDS["p16"]
    r_split, r_cut = cut_of("p16")
    kw = dict(scheme=ref.TSC, gradient=ref.GRADIENT4, deconvolve=2, soften=0.01)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = sim.p3m_field(origin, spacing, dims, G, r_split, r_cut, **kw)   # (no count before it)
        now = twin.get_points()
        assert 0 < len(now) < n - 10
        xyz, m = pm_ref.bodies(now)
        same_call(got, nb.host_p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, **kw), "after a retain")
        assert len(got[0]) == len(now)
        after = sim.get_points()
        for f in ("position", "velocity", "acceleration", "mass"):
            assert after[f].tobytes() == now[f].tobytes(), f"the state after the call: {f}"


def test_capacity_and_refusals(gpu):
    import ctypes as C
    nb = gpu
    rec = world("edge257", True)
    origin, spacing, dims = ref.GRIDS["p16"]
    spec = nb.grid_spec(origin, spacing, dims, ref.CIC, nb.DEPOSIT_MASS, True, -1)
    good = nb.p3m_spec(G, 0.3, 0.9)
    with make(nb, rec) as sim:
        sim.last_error = lambda: (nb.lib.nbody_last_error(sim._h) or b"").decode()
        acc = np.full((len(rec), 3), 7.0)
        n = C.c_size_t(0)
        rc = nb.lib.nbody_p3m_field(sim._h, C.byref(spec), C.byref(good), acc.ctypes.data, None, None, len(rec) - 1, C.byref(n), None)
        assert rc == nb.NBODY_ERR_CAPACITY and n.value == len(rec) and (acc == 7.0).all()
        for bad in (nb.p3m_spec(G, 0.3, 1.1), nb.p3m_spec(G, 0.0, 0.9), nb.p3m_spec(G, 0.3, 0.9, terms=3), nb.p3m_spec(G, 0.3, 0.9, soften=-1.0)):
            rc = nb.lib.nbody_p3m_field(sim._h, C.byref(spec), C.byref(bad), acc.ctypes.data, None, None, len(rec), C.byref(n), None)
            assert rc == nb.NBODY_ERR_INVALID and "nbody_p3m_field" in sim.last_error() and (acc == 7.0).all()
        open_spec = nb.grid_spec(origin, spacing, dims, ref.CIC, nb.DEPOSIT_MASS, False, -1)
        rc = nb.lib.nbody_p3m_field_at(sim._h, C.byref(open_spec), C.byref(good), acc.ctypes.data, 4, acc.ctypes.data, None, None, None)
        assert rc == nb.NBODY_ERR_INVALID and "nbody_p3m_field_at" in sim.last_error() and "periodic" in sim.last_error()
        assert [int(v) for v in sim.p3m_field_stats()] == [0, 0, 0, 0]


def test_multi_rank_and_spatial_handles_are_refused(gpu):
    import ctypes as C
    nb = gpu
    rec = world("edge257", False)
    origin, spacing, dims = ref.GRIDS["p16"]
    spec, good = nb.grid_spec(origin, spacing, dims, ref.CIC, nb.DEPOSIT_MASS, True, -1), nb.p3m_spec(G, 0.3, 0.9)
    pts = np.zeros((2, 3))
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, 64.0, **kw) as sim:
            acc = np.full((257, 3), 7.0)
            counts = np.full(8, 99, np.uint64)
            stats = (C.c_uint64 * 4)(9, 9, 9, 9)
            n = C.c_size_t(5)
            assert nb.lib.nbody_p3m_field(sim._h, C.byref(spec), C.byref(good), acc.ctypes.data, None, None, 257, C.byref(n),
                                          counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_p3m_field:" in nb.lib.nbody_last_error(sim._h), kw
            assert nb.lib.nbody_p3m_field_at(sim._h, C.byref(spec), C.byref(good), pts.ctypes.data, 2, acc.ctypes.data, None, None,
                                             counts.ctypes.data) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_p3m_field_at:" in nb.lib.nbody_last_error(sim._h), kw
            assert (acc == 7.0).all() and (counts == 99).all() and n.value == 5, "a refused call writes nothing"
            assert nb.lib.nbody_p3m_field_stats(sim._h, stats) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_p3m_field_stats:" in nb.lib.nbody_last_error(sim._h) and list(stats) == [9, 9, 9, 9], kw


# ------------------------------------------------------------------------------------------------ 4. nbody_pm_field as it was
@pytest.mark.parametrize("deconvolve", [0, 2])
def test_pm_field_returns_the_bits_it_returned_before(gpu, deconvolve):
    """nbody_pm_field shares its stages with the new call: before, between and after P3M calls it gives nbody_host_pm_field's bits,
    which tests/test_pm_checker.py ties to the three restatements that this change does not touch"""
    nb = gpu
    rec = world("edge257", True)
    xyz, m = pm_ref.bodies(rec)
    origin, spacing, dims = ref.GRIDS["p16"]
    kw = dict(scheme=ref.TSC, gradient=ref.GRADIENT4, periodic=True, green=ref.SPECTRAL, deconvolve=deconvolve)
    want = nb.host_pm_field(xyz, m, origin, spacing, dims, G, **kw)
    restated = pm_ref.pm_field(xyz, m, origin, spacing, dims, G, **kw)
    ref.same_bits(want[0], restated[0], "the host call is the restatement: acc")
    ref.same_bits(want[1], restated[1], "the host call is the restatement: phi")
    with make(nb, rec) as sim:
        same_call(sim.pm_field(origin, spacing, dims, G, **kw), want, "before")
        field(sim, "four-chain-cells", 0.0, ref.BOTH)
        same_call(sim.pm_field(origin, spacing, dims, G, **kw), want, "after a P3M call")


# ------------------------------------------------------------------------------------------------ 5. the command line
def test_the_command_line_option(gpu):
    """nbody_cli --p3m goes through the C++ mirror (host/simulation.hpp p3m_field): its rows are the Python mirror's"""
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        spacing = 4.0 / 32
        for arg, green, gradient in (("diff2:grad2", nb.POISSON_DIFF2, nb.SAMPLE_GRADIENT2), ("spectral:grad4", nb.POISSON_SPECTRAL, nb.SAMPLE_GRADIENT4)):
            run = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--deposit", "cic:32:2",
                                  "--p3m", arg], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr
            acc, phi, cls, counts = sim.p3m_field((-2.0, -2.0, -2.0), spacing, (32, 32, 32), 1.0, 1.25 * spacing, 4.5 * (1.25 * spacing),
                                                  nb.DEPOSIT_CIC, gradient, green)
            stats = sim.p3m_field_stats()
            m = re.search(r"^P3M: .* gradient (\d) g \S+ r_split \S+ r_cut \S+ bodies (\d+) deposited (\d+) (\d+) (\d+) (\d+) sampled (\d+) (\d+) (\d+) (\d+) "
                          r"partners (\d+) terms (\d+)$", run.stdout, flags=re.M)
            assert m, run.stdout
            assert int(m.group(1)) == gradient and int(m.group(2)) == len(acc) and [int(m.group(k)) for k in range(3, 11)] == [int(v) for v in counts]
            assert [int(m.group(11)), int(m.group(12))] == [int(stats[2]), int(stats[3])] and int(stats[3]) > 0
            rows = re.findall(r"^P3M body (\d+) class (\d)((?: \S+)+)$", run.stdout, flags=re.M)
            assert len(rows) == 8, run.stdout
            for i, (index, kind, values) in enumerate(rows):
                assert int(index) == i and int(kind) == cls[i]
                assert np.array([float(v) for v in values.split()]).tobytes() == np.append(acc[i], phi[i]).tobytes()
    assert subprocess.run([cli, "--deposit", "cic:32:2", "--p3m", "isolated:grad2"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([cli, "--p3m", "spectral:grad2"], capture_output=True, text=True, timeout=60).returncode == 2
