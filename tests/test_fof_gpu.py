"""nbody_fof_labels and nbody_fof_groups on the device (include/nbody_hip.h, "friends-of-friends groups"): the labels integer
for integer and every byte of the catalogue against the numpy restatement (tests/fof_ref.py) across the 256-body tile edge;
adversarial chains, a star and interleaved lattices; independence of the launch shape; after a retain without a count call; no
trace in the state; capacity and NULL forms; refusals; the command line.  tests/test_fof_checker.py checks the worlds used here
on the restatement itself."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fof_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 64.0
SIZES = [0, 1, 2, 255, 256, 257, 1000]
B = ref.CLUMPY_B
CHAIN_B = 0.25


def settings(**kw):
    return dict(dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5), **kw)


def make(nb, rec, method="bf", st=None, width=WIDTH, math_mode=None, hermite=False, block=None, **kw):
    bh = method == "bh"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE,
                        math_mode=nb.FAST if math_mode is None else math_mode, tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO,
                        capacity=max(len(rec), 4), **kw)
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
def _clumpy(n, f64):
    rec = ref.clumpy(_nb(), n, seed=n, f64=f64)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def expected_labels(n, f64):
    """the restatement's labels of _clumpy(n, f64), computed once"""
    lab = ref.labels(_clumpy(n, f64), B)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def expected_groups(n, f64, min_members):
    return ref.groups(_clumpy(n, f64), B, min_members, lab=expected_labels(n, f64))


def counters(s):
    return (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


# ------------------------------------------------------------------------------------------------ 1. labels, integer for integer
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_labels_are_the_restatement(gpu, n, f64):
    nb = gpu
    rec = _clumpy(n, f64)
    want = expected_labels(n, f64)
    with make(nb, rec) as sim:
        lab, n_groups = sim.fof_labels(B)
        ref.check_labels(lab, n_groups, rec, B, want=want)
        same_records(sim.get_points(), rec, "a read-only call")
    if n == 2:
        assert want.tolist() == [0, 0]
    if n == 1000:   # (the world itself: tests/test_fof_checker.py::test_the_worlds_of_the_device_tests)
        roots, counts = np.unique(want, return_counts=True)
        assert (counts >= 2).sum() >= 3 and max(len(set((np.nonzero(want == r)[0] // 256).tolist())) for r in roots) >= 3


# ------------------------------------------------------------------------------------------------ 2. adversarial shapes
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_chains_a_star_and_two_lattices(gpu, f64):
    nb = gpu
    rec, perm = ref.chain(nb, 1025, CHAIN_B, f64)
    with make(nb, rec) as sim:
        lab, n_groups = sim.fof_labels(CHAIN_B)
        assert n_groups == 1 and (lab == 0).all(), "one chain in scrambled order is one group with label 0"
    rec, perm = ref.chain(nb, 1025, CHAIN_B, f64, cut=500)
    with make(nb, rec) as sim:
        lab, n_groups = sim.fof_labels(CHAIN_B)
        ref.check_labels(lab, n_groups, rec, CHAIN_B)
        assert n_groups == 2 and (lab[perm[:501]] == 0).all() and (lab[perm[501:]] == perm[501:].min()).all()
    rec = ref.star(nb, 600, CHAIN_B, f64)
    with make(nb, rec) as sim:
        lab, n_groups = sim.fof_labels(CHAIN_B)
        assert n_groups == 1 and (lab == 0).all()
        grp, mem = sim.fof_groups(CHAIN_B)
        assert len(grp) == 1 and grp["count"][0] == 601 and np.array_equal(mem, np.arange(601))
    rec = ref.two_lattices(nb, 6, CHAIN_B, f64)
    with make(nb, rec) as sim:
        lab, n_groups = sim.fof_labels(CHAIN_B)
        assert n_groups == 2 and (lab[0::2] == 0).all() and (lab[1::2] == 1).all()
        grp, mem = sim.fof_groups(CHAIN_B)
        ref.check_groups(grp, mem, *ref.groups(rec, CHAIN_B, lab=lab))


def test_a_lattice_full_of_ties_and_a_nan_body(gpu):
    nb = gpu
    rec = ref.lattice(nb, 5, True)
    rec["position"][7, 2] = np.nan
    rec["position"][9, 0] = np.inf
    with make(nb, rec) as sim:
        for b in (1.0, 1.001, 1.5):   # (neighbours exactly 1 apart: not linked at b = 1)
            lab, n_groups = sim.fof_labels(b)
            ref.check_labels(lab, n_groups, rec, b)
            assert lab[7] == 7 and lab[9] == 9 and (lab == 7).sum() == 1 and (lab == 9).sum() == 1
        assert sim.fof_labels(1.0)[1] == 125


# ------------------------------------------------------------------------------------------------ 3. the launch shape
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_launch_shape_does_not_show(gpu, f64):
    nb = gpu
    rec = _clumpy(1000, f64)
    got = []
    for waves in (64, 4096):   # 4 and 16 partner slices at 1000 bodies
        with make(nb, rec, tuning={"bf64_waves": waves}) as sim:
            for _ in range(2):
                lab, n_groups = sim.fof_labels(B)
                grp, mem = sim.fof_groups(B, 2)
                got.append((lab.tobytes(), n_groups, grp.tobytes(), mem.tobytes()))
    assert all(g == got[0] for g in got[1:])
    assert np.array_equal(np.frombuffer(got[0][0], np.int32), expected_labels(1000, f64))


# ------------------------------------------------------------------------------------------------ 4. the catalogue
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("min_members", [1, 2, 5])
def test_the_catalogue_is_the_restatement(gpu, min_members, f64):
    nb = gpu
    rec = _clumpy(1000, f64)
    want, want_members = expected_groups(1000, f64, min_members)
    assert (want["count"] > 128).any() and ((want["count"] > 64) & (want["count"] <= 128)).any()
    with make(nb, rec) as sim:
        grp, mem = sim.fof_groups(B, min_members)
    ref.check_groups(grp, mem, want, want_members)   # first, count, offset, the members; mass, mx, mv bit for bit
    assert (np.diff(grp["first"]) > 0).all() and (grp["count"] >= min_members).all()
    for g in grp:
        who = mem[g["offset"]:g["offset"] + g["count"]]
        assert who[0] == g["first"] and (np.diff(who) > 0).all()
    if min_members == 1:
        assert np.array_equal(np.sort(mem), np.arange(1000)), "every body exactly once"


# ------------------------------------------------------------------------------------------------ 5. after a retain
@pytest.mark.parametrize("method,f64", [("bf", False), ("bf", True), ("bh", False)], ids=["bf-f32", "bf-f64", "bh-f32"])
def test_after_a_retain_without_a_count_call(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies, the host's view of the count stays an upper bound"""
    nb = gpu
    n = 700
    rec = nb.plummer(n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        h = sim._h
        n_out, n_groups = C.c_size_t(0), C.c_size_t(0)
        lab = np.full(n, -7, np.int32)
        assert nb.lib.nbody_fof_labels(h, 0.08, lab.ctypes.data, n, C.byref(n_out), C.byref(n_groups)) == 0   # (no count before it)
        grp, mem = sim.fof_groups(0.08, 2)
        pts = twin.get_points()
        assert 0 < len(pts) < n - 10 and n_out.value == len(pts)
        ref.check_labels(lab[: n_out.value], n_groups.value, pts, 0.08)
        assert (lab[n_out.value:] == -7).all()
        want, want_members = ref.groups(pts, 0.08, 2)
        assert len(want) >= 3
        ref.check_groups(grp, mem, want, want_members)


# ------------------------------------------------------------------------------------------------ 6. no trace
@pytest.mark.parametrize("which", ["bf-f32", "bh-f32", "hermite-block"])
def test_the_calls_leave_no_trace(gpu, which):
    nb = gpu
    hermite = which == "hermite-block"
    rec = _clumpy(257, hermite)
    st = settings(dt=1.0 / 64 if hermite else 1.0 / 256)

    def build():
        return make(nb, rec, "bh" if which == "bh-f32" else "bf", st=st, hermite=hermite, block=(0.02, 4))

    def state(sim):
        out = {"records": sim.get_points(), "stats": counters(sim.stats())}
        if hermite:
            out.update(jerk=sim.jerk(), levels=sim.levels(), block_counts=sim.block_step_counts())
        return out

    with build() as a, build() as never:
        a.steps(3)
        never.steps(3)
        lab, n_groups = a.fof_labels(B)
        grp, mem = a.fof_groups(B, 1)
        assert len(lab) == 257 and len(grp) == n_groups and len(mem) == 257
        if hermite:   # the held derivatives and the levels are still valid
            assert len(a.jerk()) == 257 and len(a.levels()) == 257
        with a.clone() as twin:   # a clone gives the same answer as its source
            lab2, n2 = twin.fof_labels(B)
            grp2, mem2 = twin.fof_groups(B, 1)
            assert lab2.tobytes() == lab.tobytes() and n2 == n_groups and grp2.tobytes() == grp.tobytes() and mem2.tobytes() == mem.tobytes()
        ref.check_labels(lab, n_groups, a.get_points(), B)
        a.steps(3)
        never.steps(3)
        sa, sn = state(a), state(never)
        same_records(sa["records"], sn["records"], which)
        assert sa["stats"] == sn["stats"], which
        if hermite:
            assert ref.same_bits(sa["jerk"], sn["jerk"]) and np.array_equal(sa["levels"], sn["levels"]), which
            assert sa["block_counts"] == sn["block_counts"], which


def test_tracers_and_the_external_field_play_no_part(gpu):
    nb = gpu
    rec = _clumpy(257, False)
    import merge_ref
    tracers = merge_ref.cloud(nb, 100, seed=41, f64=False)
    with make(nb, rec) as sim:
        sim.set_tracers(tracers)
        sim.external_field = [nb.external_component(nb.EXT_PLUMMER, (2.0, 1.5), (0.5, 0.0, 0.0))]
        before = sim.get_tracers()
        lab, n_groups = sim.fof_labels(B)
        ref.check_labels(lab, n_groups, rec, B, want=expected_labels(257, False))
        assert len(before) == 100 and sim.get_tracers().tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ 7. capacity, NULL forms, refusals
def test_capacity_and_null_forms(gpu):
    nb = gpu
    lib = nb.lib
    rec = _clumpy(257, True)
    want = expected_labels(257, True)
    want_grp, want_mem = expected_groups(257, True, 2)
    n_all = len(np.unique(want))
    k, m = len(want_grp), len(want_mem)
    assert k >= 2 and m > k
    with make(nb, rec) as sim:
        h = sim._h
        n, ng, nm = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
        assert lib.nbody_fof_labels(h, B, None, 0, C.byref(n), None) == 0 and n.value == 257
        assert lib.nbody_fof_labels(h, B, None, 0, C.byref(n), C.byref(ng)) == 0 and (n.value, ng.value) == (257, n_all)
        assert lib.nbody_fof_labels(h, B, None, 0, None, None) == 0
        lab = np.full(257, -7, np.int32)
        n.value = ng.value = 77
        assert lib.nbody_fof_labels(h, B, lab.ctypes.data, 256, C.byref(n), C.byref(ng)) == nb.NBODY_ERR_CAPACITY
        assert (n.value, ng.value) == (257, n_all) and b"nbody_fof_labels" in lib.nbody_last_error(h) and (lab == -7).all()
        assert lib.nbody_fof_labels(h, B, lab.ctypes.data, 257, None, None) == 0 and np.array_equal(lab, want)
        # groups: counts only, either array alone, and either one too small
        assert lib.nbody_fof_groups(h, B, 2, None, 0, C.byref(ng), None, 0, C.byref(nm)) == 0 and (ng.value, nm.value) == (k, m)
        assert lib.nbody_fof_groups(h, B, 2, None, 0, None, None, 0, None) == 0
        grp = np.zeros(k, nb.GROUP_DTYPE)
        mem = np.full(m, -7, np.int32)
        for gcap, mcap in ((k - 1, m), (k, m - 1)):
            ng.value = nm.value = 77
            assert lib.nbody_fof_groups(h, B, 2, grp.ctypes.data, gcap, C.byref(ng), mem.ctypes.data, mcap, C.byref(nm)) == nb.NBODY_ERR_CAPACITY
            assert (ng.value, nm.value) == (k, m) and b"nbody_fof_groups" in lib.nbody_last_error(h)
            assert not grp["count"].any() and (mem == -7).all(), "nothing written"
        assert lib.nbody_fof_groups(h, B, 2, grp.ctypes.data, k, None, None, 0, None) == 0
        ref.check_groups(grp, want_mem, want_grp, want_mem)
        assert lib.nbody_fof_groups(h, B, 2, None, 0, None, mem.ctypes.data, m, C.byref(nm)) == 0 and np.array_equal(mem, want_mem)
        same_records(sim.get_points(), rec, "after the calls")
        sim.steps(2)
        assert len(sim) == 257


def test_refusals_name_the_call(gpu):
    nb = gpu
    lib = nb.lib
    rec = _clumpy(255, False)
    n = C.c_size_t(0)
    with make(nb, rec) as sim:
        h = sim._h
        for b in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.nbody_fof_labels(h, b, None, 0, C.byref(n), C.byref(n)) == nb.NBODY_ERR_INVALID
            assert b"nbody_fof_labels" in lib.nbody_last_error(h)
            assert lib.nbody_fof_groups(h, b, 2, None, 0, C.byref(n), None, 0, None) == nb.NBODY_ERR_INVALID
            assert b"nbody_fof_groups" in lib.nbody_last_error(h)
            with pytest.raises(nb.NbodyError) as e:
                sim.fof_labels(b)
            assert e.value.code == nb.NBODY_ERR_INVALID
        for min_members in (0, -3):
            assert lib.nbody_fof_groups(h, B, min_members, None, 0, C.byref(n), None, 0, None) == nb.NBODY_ERR_INVALID
            assert b"nbody_fof_groups" in lib.nbody_last_error(h) and b"min_members" in lib.nbody_last_error(h)
        lab, n_groups = sim.fof_labels(B)   # the handle still works
        ref.check_labels(lab, n_groups, rec, B, want=expected_labels(255, False))
        same_records(sim.get_points(), rec, "after the refusals")
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, WIDTH, **kw) as sim:
            assert lib.nbody_fof_labels(sim._h, B, None, 0, None, None) == nb.NBODY_ERR_INVALID
            assert b"nbody_fof_labels" in lib.nbody_last_error(sim._h)
            assert lib.nbody_fof_groups(sim._h, B, 2, None, 0, None, None, 0, None) == nb.NBODY_ERR_INVALID
            assert b"nbody_fof_groups" in lib.nbody_last_error(sim._h)
            with pytest.raises(nb.NbodyError) as e:
                sim.fof_groups(B)
            assert e.value.code == nb.NBODY_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_cli_prints_the_groups(gpu):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nbody-llm_amd", "nbody_cli")
    out = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--fof", "0.1:3"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^FoF groups: (\d+) largest (\d+) mass (\S+) ungrouped (\S+)$", out.stdout, flags=re.M)
    assert len(rows) == 1, out.stdout
    groups, largest, mass, loose = int(rows[0][0]), int(rows[0][1]), float(rows[0][2]), float(rows[0][3])
    assert groups >= 1 and largest >= 3 and abs(mass - largest / 400.0) < 1e-9 and 0.0 <= loose < 1.0
