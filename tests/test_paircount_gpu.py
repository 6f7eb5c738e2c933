"""nbody_pair_counts and nbody_pair_counts_at on the device (include/nbody_hip.h, "pair-separation counts") against the numpy
restatement (tests/paircount_ref.py): every integer equal, on both dtypes and under both search modes with a twin handle in
the other mode; the invariants; the statistics against tests/cells_ref.py; independence of the launch shape, of the
contention knob and of the flush interval; 16 384 bodies on a device-built Barnes-Hut handle, the device against the device;
the cumulative counts against nbody_neighbors_within; handle states, no trace, refusals, the command line and the Python
mirror.  What makes these worlds worth looking at is asserted on the CPU in tests/test_paircount_checker.py."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cells_ref
import fof_ref
import merge_ref
import paircount_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 64.0
B = fof_ref.CLUMPY_B
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
ZEROS = (0, 0, 0, 0)


def settings(**kw):
    return dict(dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5), **kw)


def make(nb, rec, method="bf", st=None, width=WIDTH, hermite=False, block=None, cells=True, **kw):
    bh = method == "bh"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO, capacity=max(len(rec), 4), **kw)
    sim.settings = nb.Settings(**(st or settings()))
    sim.init()
    if hermite:
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
    if cells:
        sim.pair_search = nb.SEARCH_CELLS
    return sim


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


@functools.lru_cache(maxsize=None)
def world(name, f64):
    return ref.world(_nb(), name, f64)


@functools.lru_cache(maxsize=None)
def bin_sets(name, f64):
    rec, lengths = world(name, f64)
    sets = ref.bin_sets(lengths, ref.diameter(rec))
    if name == "lattice_edges":
        sets["lattice3"] = np.array(ref.LATTICE_EDGES)
    return sets


@functools.lru_cache(maxsize=None)
def auto_r2(name, f64):
    return ref.auto_r2(world(name, f64)[0])


@functools.lru_cache(maxsize=None)
def expected(name, f64, which):
    """(counts, outside) of the restatement for one bin set of a world, computed once and left unchanged"""
    return ref.pair_counts(world(name, f64)[0], bin_sets(name, f64)[which], r2=auto_r2(name, f64))


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def total(got):
    return int(got[0].sum()) + int(got[1].sum())


def as_bytes(got):
    return got[0].tobytes() + got[1].tobytes()


# ------------------------------------------------------------------------------------------------ 1. the restatement and a twin
@DTYPES
@pytest.mark.parametrize("name", ref.WORLDS)
def test_every_integer_is_the_restatement_s_in_both_modes(gpu, name, f64):
    nb = gpu
    rec, _ = world(name, f64)
    n = len(rec)
    with make(nb, rec) as sim, make(nb, rec, cells=False) as twin:
        assert sim.pair_search == nb.SEARCH_CELLS and twin.pair_search == nb.SEARCH_ALL_PAIRS
        for which, edges in bin_sets(name, f64).items():
            want = expected(name, f64, which)
            want_record = cells_ref.expected_stats(rec, abs(float(edges[-1]))) if n else ZEROS   # (no bodies: the record stays as it was)
            for s, record in ((sim, want_record), (twin, ZEROS)):
                got = s.pair_counts(edges)
                ref.check(got, want, f"{name} {which} {'cells' if s is sim else 'all pairs'}")
                assert total(got) == n * (n - 1) // 2
                assert s.pair_search_stats() == record, (name, which)
            if n:   # the record is what nbody_fof_labels leaves for the same state and length
                sim.fof_labels(abs(float(edges[-1])))
                assert sim.pair_search_stats() == want_record
        same_records(sim.get_points(), rec, "read-only calls")
    if name == "lattice_edges":
        counts, outside = expected(name, f64, "lattice3")
        assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0 and outside[1] > 0
    if name == "clumpy1000":
        assert expected(name, f64, "from_above_zero")[1][0] > 0, "outside[0] != 0"
        assert cells_ref.expected_stats(rec, float(bin_sets(name, f64)["beyond_the_world"][-1]))[2] == 1, "one cell holds every body"


# ------------------------------------------------------------------------------------------------ 2. the launch shape does not show
@DTYPES
def test_the_launch_shape_and_the_knobs_do_not_show(gpu, f64):
    """1000 bodies are 4 groups of 256, 16 waves: bf64_waves = 16 makes K = 1 slice, 48 makes K = 3, the default (2048) K = 16;
    pair_hist_combine 0, 1, 2: how a wave's lanes that hit one slot are combined; pair_hist_flush = 1: the block hands its LDS
    words over after every tile, and a lane of the pass over the cells after its first 256 counts (one cell holds 1000 bodies)"""
    nb = gpu
    rec, _ = world("clumpy1000", f64)
    sets = [(which, bin_sets("clumpy1000", f64)[which], expected("clumpy1000", f64, which))
            for which in ("log1024", "from_above_zero", "beyond_the_world")]
    for waves in (16, 48, None):
        with make(nb, rec, cells=False) as sim:
            if waves:
                sim.set_tuning("bf64_waves", waves)
            for combine in (0, 1, 2):
                for flush in (0, 1):
                    sim.set_tuning("pair_hist_combine", combine)
                    sim.set_tuning("pair_hist_flush", flush)
                    for which, edges, want in sets:
                        ref.check(sim.pair_counts(edges), want, f"{which} waves {waves} combine {combine} flush {flush}")
    with make(nb, rec) as sim:
        for flush in (0, 1, 3):
            sim.set_tuning("pair_hist_flush", flush)
            for which, edges, want in sets:
                ref.check(sim.pair_counts(edges), want, f"{which} cells flush {flush}")
                assert sim.pair_search_stats()[0] == 1


def test_several_tiles_per_slice(gpu):
    """4 097 bodies: 17 groups; bf64_waves = 16 makes K = 1, a slice of 17 tiles, the last of one partner"""
    nb = gpu
    n = 4097
    rec = fof_ref.clumpy(nb, n, seed=n, f64=False)
    edges = ref.log_edges(1e-3, 40.0, 33)
    want = ref.pair_counts(rec, edges)
    assert total(want) == n * (n - 1) // 2 and np.count_nonzero(want[0]) > 20
    seen = []
    for waves, combine, flush in ((16, 0, 0), (16, 2, 5), (None, 1, 0), (64, 0, 1)):
        with make(nb, rec, cells=False) as sim:
            if waves:
                sim.set_tuning("bf64_waves", waves)
            sim.set_tuning("pair_hist_combine", combine)
            sim.set_tuning("pair_hist_flush", flush)
            got = sim.pair_counts(edges)
            ref.check(got, want, f"waves {waves} combine {combine} flush {flush}")
            seen.append(as_bytes(got))
    with make(nb, rec) as sim:
        seen.append(as_bytes(sim.pair_counts(edges)))
    assert len(set(seen)) == 1


# ------------------------------------------------------------------------------------------------ 3. bodies against points
@DTYPES
def test_pair_counts_at(gpu, f64):
    nb = gpu
    rec, _ = world("clumpy1000", f64)
    x = np.ascontiguousarray(rec["position"], np.float64)
    rng = np.random.default_rng(77)
    edge_sets = (np.array([0.0, 1e-6, B, 1.0, 30.0]), ref.log_edges(1e-3, 20.0, 1024), np.array([0.5, 2.0]))
    with make(nb, rec) as sim:
        sim.pair_counts(edge_sets[0])
        record = sim.pair_search_stats()
        assert record[0] == 1
        for m in (0, 1, 255, 257):
            scattered = rng.uniform(-8.0, 8.0, (m, 3))
            on_bodies = x[rng.choice(len(x), m, replace=False)]   # r2 == 0 with edges[0] == 0 lands in bin 0
            far = scattered + 1e6
            holed = scattered.copy()
            if m:
                holed[m // 2, 1] = np.nan
                holed[0, 2] = np.inf
            for what, points in (("scattered", scattered), ("on bodies", on_bodies), ("far", far), ("a NaN point", holed)):
                for edges in edge_sets:
                    got = sim.pair_counts_at(points, edges)
                    ref.check(got, ref.pair_counts_at(rec, points, edges), f"m = {m} {what}")
                    assert total(got) == len(rec) * m
            if m:
                counts, outside = sim.pair_counts_at(on_bodies, edge_sets[0])
                assert counts[0] >= m, "a point on a body is a pair of r2 = 0 in bin 0"
                counts, outside = sim.pair_counts_at(far, edge_sets[0])
                assert not counts.any() and outside[0] == 0 and outside[1] == len(rec) * m
                counts, outside = sim.pair_counts_at(holed, edge_sets[0])
                assert outside[1] >= (2 if m > 1 else 1) * len(rec)
        assert sim.pair_search_stats() == record, "pair_counts_at does not touch the record"
        for combine, flush, waves in ((1, 0, 16), (2, 1, 48)):
            sim.set_tuning("pair_hist_combine", combine)
            sim.set_tuning("pair_hist_flush", flush)
            sim.set_tuning("bf64_waves", waves)
            ref.check(sim.pair_counts_at(scattered, edge_sets[1]), ref.pair_counts_at(rec, scattered, edge_sets[1]), f"combine {combine}")
        same_records(sim.get_points(), rec, "read-only calls")


@DTYPES
def test_one_point_at_the_centre_of_mass_counts_the_shells(gpu, f64):
    nb = gpu
    rec, _ = world("clumpy1000", f64)
    x = np.ascontiguousarray(rec["position"], np.float64)
    m = np.ascontiguousarray(rec["mass"], np.float64)
    com = (m[:, None] * x).sum(axis=0) / m.sum()
    edges = np.linspace(0.0, 16.0, 33)
    r = np.sqrt(((x - com) ** 2).sum(axis=1))   # an independent route; it agrees as long as no body stands on a shell's edge
    assert np.abs(r[:, None] - edges[None, :]).min() > 1e-9
    shells = np.histogram(r, bins=edges)[0]
    with make(nb, rec, cells=False) as sim:
        counts, outside = sim.pair_counts_at(com[None, :], edges)
    assert np.array_equal(counts.astype(np.int64), shells) and outside[0] == 0 and int(outside[1]) == len(rec) - shells.sum()
    assert shells.sum() > 900 and np.count_nonzero(shells) > 10


# ------------------------------------------------------------------------------------------------ 4. 16 384 bodies, the device against the device
@DTYPES
def test_a_larger_clumpy_world_on_a_device_built_tree_handle(gpu, f64):
    nb = gpu
    n = 16384
    rec = fof_ref.clumpy(nb, n, seed=n, f64=f64)
    with make(nb, rec, "bh") as sim, make(nb, rec, "bh", cells=False) as twin:
        for edges in (ref.log_edges(1e-3, 0.5, 33), np.array([0.0, B, 3.0 * B]), ref.log_edges(1e-2, 1.0, 1024)):
            got, other = sim.pair_counts(edges), twin.pair_counts(edges)
            stats = sim.pair_search_stats()
            assert as_bytes(got) == as_bytes(other), "cells == all pairs, integer for integer"
            assert total(got) == n * (n - 1) // 2 and got[0].any()
            assert stats == cells_ref.expected_stats(rec, float(edges[-1])) and stats[0] == 1 and twin.pair_search_stats() == ZEROS
        counts, outside = sim.pair_counts(np.array([0.0, B, 3.0 * B]))
        assert outside[0] == 0
        for edge, pairs in zip((B, 3.0 * B), np.cumsum(counts.astype(np.int64))):
            assert 2 * pairs == len(sim.neighbors_within(edge)[1])
        same_records(sim.get_points(), rec, "read-only calls")


# ------------------------------------------------------------------------------------------------ 5. against the existing calls
@pytest.mark.parametrize("cells", [False, True], ids=["all-pairs", "cells"])
def test_the_cumulative_counts_are_the_neighbour_totals(gpu, cells):
    nb = gpu
    rec, _ = world("clumpy1000", True)
    edges = np.array([0.0, 0.03, 0.051, B, 0.3, 2.0, 9.0])
    with make(nb, rec, cells=cells) as sim:
        counts, outside = sim.pair_counts(edges)
        assert outside[0] == 0
        cumulative = np.cumsum(counts.astype(np.int64))
        for e, pairs in zip(edges[1:], cumulative):
            assert 2 * pairs == len(sim.neighbors_within(e)[1]), e
        assert cumulative[0] > 0 and (np.diff(cumulative) > 0).all()


# ------------------------------------------------------------------------------------------------ 6. handle states
@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_after_a_retain_without_a_count_call(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies, the host's view of the count stays an upper bound"""
    nb = gpu
    n = 700
    edges = ref.log_edges(0.01, 2.0, 33)
    rec = nb.plummer(n, seed=5, f64=f64)
    points = np.random.default_rng(9).uniform(-0.5, 0.5, (70, 3))
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5, cells=False) as twin:
        sim.steps(4)
        twin.steps(4)
        got = [(s.pair_counts(edges), s.pair_counts_at(points, edges)) for s in (sim, twin)]   # (no count before them)
        stats = sim.pair_search_stats()
        pts = twin.get_points()
        live = len(pts)
        assert 0 < live < n - 10
        for auto, cross in got:
            ref.check(auto, ref.pair_counts(pts, edges), "auto")
            ref.check(cross, ref.pair_counts_at(pts, points, edges), "cross")
            assert total(auto) == live * (live - 1) // 2 and total(cross) == live * 70
        assert stats == cells_ref.expected_stats(pts, float(edges[-1])) and stats[1] == live


def test_tracers_and_the_external_field_play_no_part(gpu):
    nb = gpu
    rec, _ = world("clumpy257", False)
    tracers = merge_ref.cloud(nb, 100, seed=41, f64=False)
    with make(nb, rec) as sim:
        sim.set_tracers(tracers)
        sim.external_field = [nb.external_component(nb.EXT_PLUMMER, (2.0, 1.5), (0.5, 0.0, 0.0))]
        before = sim.get_tracers()
        for which, edges in bin_sets("clumpy257", False).items():
            ref.check(sim.pair_counts(edges), expected("clumpy257", False, which), which)
        points = np.ascontiguousarray(tracers["position"], np.float64)
        ref.check(sim.pair_counts_at(points, np.array([0.0, 1.0, 20.0])), ref.pair_counts_at(rec, points, np.array([0.0, 1.0, 20.0])))
        assert len(before) == 100 and sim.get_tracers().tobytes() == before.tobytes()


@pytest.mark.parametrize("which", ["bf-f32", "bh-f32", "hermite-block"])
def test_the_calls_leave_no_trace(gpu, which):
    nb = gpu
    hermite = which == "hermite-block"
    rec, _ = world("clumpy257", hermite)
    st = settings(dt=1.0 / 64 if hermite else 1.0 / 256)
    edges = ref.log_edges(1e-3, 1.0, 33)
    points = np.random.default_rng(2).uniform(-8.0, 8.0, (33, 3))

    def build(cells):
        return make(nb, rec, "bh" if which == "bh-f32" else "bf", st=st, hermite=hermite, block=(0.02, 4), cells=cells)

    def state(sim):
        s = sim.stats()
        out = {"records": sim.get_points(), "stats": (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)}
        if hermite:
            out.update(jerk=sim.jerk(), levels=sim.levels(), block_counts=sim.block_step_counts())
        return out

    with build(True) as a, build(False) as b, build(False) as never:
        for s in (a, b, never):
            s.steps(3)
        pts = never.get_points()
        for s in (a, b):
            ref.check(s.pair_counts(edges), ref.pair_counts(pts, edges), which)
            ref.check(s.pair_counts_at(points, edges), ref.pair_counts_at(pts, points, edges), which)
        assert a.pair_search_stats()[0] == 1 and b.pair_search_stats() == ZEROS
        if hermite:   # the held derivatives and the levels are still valid
            assert len(a.jerk()) == 257 and len(a.levels()) == 257
        for s in (a, b, never):
            s.steps(3)
        sn = state(never)
        for s, what in ((a, which + " cells"), (b, which + " all pairs")):
            ss = state(s)
            same_records(ss["records"], sn["records"], what)
            assert ss["stats"] == sn["stats"], what
            if hermite:
                assert fof_ref.same_bits(ss["jerk"], sn["jerk"]) and np.array_equal(ss["levels"], sn["levels"]), what
                assert ss["block_counts"] == sn["block_counts"], what


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_call(gpu):
    nb = gpu
    lib = nb.lib
    rec, _ = world("clumpy255", False)
    word = np.full(1100, 99, np.uint64)
    out = np.full(2, 99, np.uint64)
    points = np.zeros((3, 3))

    def calls(h, edges, n_bins=None, counts=word, pts=points, m=3):
        edges = np.ascontiguousarray(edges, np.float64)
        n_bins = len(edges) - 1 if n_bins is None else n_bins
        e = edges.ctypes.data if len(edges) else None
        c = counts.ctypes.data if counts is not None else None
        p = pts.ctypes.data if pts is not None else None
        yield lib.nbody_pair_counts(h, e, n_bins, c, out.ctypes.data), b"nbody_pair_counts"
        yield lib.nbody_pair_counts_at(h, p, m, e, n_bins, c, out.ctypes.data), b"nbody_pair_counts_at"

    bad_edges = ([0.0, np.nan], [0.0, np.inf], [-np.inf, 1.0], [-0.5, 1.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [1e-200, 2e-200, 1.0],
                 [0.0, 1.0, 1e200], [0.0])
    with make(nb, rec) as sim:
        h = sim._h
        for edges in bad_edges:
            assert not ref.valid_edges(edges)
            for rc, name in calls(h, edges):
                assert rc == nb.NBODY_ERR_INVALID and name in lib.nbody_last_error(h), (edges, name)
            with pytest.raises(nb.NbodyError) as e:
                sim.pair_counts(edges)
            assert e.value.code == nb.NBODY_ERR_INVALID
        too_many = np.linspace(0.0, 1.0, 1026)   # 1 025 bins
        for rc, name in list(calls(h, too_many)) + list(calls(h, [0.0, 1.0], n_bins=0)) + list(calls(h, [0.0, 1.0], n_bins=-1)):
            assert rc == nb.NBODY_ERR_INVALID and name in lib.nbody_last_error(h)
        for rc, name in calls(h, [0.0, 1.0], counts=None):
            assert rc == nb.NBODY_ERR_INVALID and name in lib.nbody_last_error(h)
        assert lib.nbody_pair_counts(h, None, 1, word.ctypes.data, None) == nb.NBODY_ERR_INVALID and b"nbody_pair_counts" in lib.nbody_last_error(h)
        rc = lib.nbody_pair_counts_at(h, None, 3, np.array([0.0, 1.0]).ctypes.data, 1, word.ctypes.data, out.ctypes.data)
        assert rc == nb.NBODY_ERR_INVALID and b"nbody_pair_counts_at" in lib.nbody_last_error(h), "points == NULL with m > 0"
        assert (word == 99).all() and (out == 99).all(), "a refused call writes nothing"
        assert sim.pair_search_stats() == ZEROS, "a refused call looked at no pair"
        # points == NULL with m == 0, outside == NULL and 1 024 bins are fine; the squares may ascend where the edges do not
        assert lib.nbody_pair_counts_at(h, None, 0, np.array([0.0, 1.0]).ctypes.data, 1, word.ctypes.data, None) == 0 and word[0] == 0
        assert lib.nbody_pair_counts(h, np.array([0.0, 1.0]).ctypes.data, 1, word.ctypes.data, None) == 0
        counts, outside = sim.pair_counts(ref.log_edges(1e-3, 1.0, 1024))
        assert len(counts) == 1024
        ref.check(sim.pair_counts([0.0, -1.0, 2.0]), ref.pair_counts(rec, [0.0, 1.0, 2.0]), "negative edges whose squares ascend")
        ref.check(sim.pair_counts(bin_sets("clumpy255", False)["log33"]), expected("clumpy255", False, "log33"), "the handle still works")
    for rc, _ in calls(None, [0.0, 1.0]):
        assert rc == nb.NBODY_ERR_INVALID
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, WIDTH, **kw) as sim:
            for rc, name in calls(sim._h, [0.0, 1.0]):
                assert rc == nb.NBODY_ERR_INVALID and name in lib.nbody_last_error(sim._h)


# ------------------------------------------------------------------------------------------------ 8. the chain through the layers
def test_cli_prints_the_pair_counts(gpu):
    nb = gpu
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nbody-llm_amd", "nbody_cli")
    num = r"([-+0-9.eE]+)"
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, WIDTH, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        for arg, lo, hi, bins, log_bins in (("0.01:4:12", 0.01, 4.0, 12, True), ("0.01:4:12:log", 0.01, 4.0, 12, True), ("0:3:7:lin", 0.0, 3.0, 7, False)):
            f = np.arange(bins + 1, dtype=np.float64) / np.float64(bins)
            formula = np.float64(lo) * (np.float64(hi) / np.float64(lo)) ** f if log_bins else np.float64(lo) + (np.float64(hi) - np.float64(lo)) * f
            lines = {}
            for mode in ("all", "cells"):
                out = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--pair-counts", arg,
                                      "--pair-search", mode], capture_output=True, text=True, timeout=120)
                assert out.returncode == 0, out.stderr
                rows = re.findall(r"^Pair count: bin (\d+) %s %s (\d+)$" % (num, num), out.stdout, flags=re.M)
                tail = re.findall(r"^Pair counts outside: below (\d+) beyond (\d+)$", out.stdout, flags=re.M)
                assert len(rows) == bins and len(tail) == 1, out.stdout
                assert [int(r[0]) for r in rows] == list(range(bins))
                edges = np.array([float(r[1]) for r in rows] + [float(rows[-1][2])])   # 17 digits name each double
                assert [float(r[2]) for r in rows[:-1]] == [float(r[1]) for r in rows[1:]]
                assert edges[0] == lo and edges[-1] == hi, "the ends are the arguments themselves"
                assert np.allclose(edges[1:-1], formula[1:-1], rtol=4 * np.finfo(np.float64).eps, atol=0.0), "the documented formula, to pow's last bits"
                counts, outside = sim.pair_counts(edges)
                assert [int(r[3]) for r in rows] == [int(c) for c in counts], (arg, mode)
                assert (int(tail[0][0]), int(tail[0][1])) == (int(outside[0]), int(outside[1]))
                lines[mode] = (rows, tail)
                found = re.findall(r"^Pair search: cells (\d+) gridded (\d+) occupied (\d+) candidates (\d+)$", out.stdout, flags=re.M)
                assert len(found) == (1 if mode == "cells" else 0), out.stdout
                if mode == "cells":
                    assert int(found[0][0]) == 1 and int(found[0][1]) == 400
            assert lines["all"] == lines["cells"]
    for bad in ("0:1:4", "0:1:4:log", "1:0.5:4", "0.1:1:0", "0.1:1:1025", "0.1:1", "abc", "0.1:1:4:cubic", "0.1:inf:4"):
        out = subprocess.run([cli, "-n", "16", "--pair-counts", bad], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2, bad


def test_the_mirror_provides_the_calls_and_the_constant(gpu):
    nb = gpu
    assert nb.PAIR_COUNT_MAX_BINS == 1024
    rec, _ = world("clumpy257", False)
    edges = bin_sets("clumpy257", False)["log33"]
    with make(nb, rec) as sim:
        counts, outside = sim.pair_counts(edges)
        assert counts.dtype == np.uint64 and outside.dtype == np.uint64 and counts.shape == (33,) and outside.shape == (2,)
        ref.check((counts, outside), expected("clumpy257", False, "log33"))
        ref.check(sim.pair_counts(list(edges)), expected("clumpy257", False, "log33"), "a list of edges")
        counts, outside = sim.pair_counts_at([[0.0, 0.0, 0.0]], edges)
        assert counts.dtype == np.uint64 and counts.shape == (33,) and total((counts, outside)) == 257
        with sim.clone() as twin:
            assert twin.pair_search == nb.SEARCH_CELLS and as_bytes(twin.pair_counts(edges)) == as_bytes(sim.pair_counts(edges))
