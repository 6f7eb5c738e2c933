"""nbody_partners and nbody_bound_pairs on the device (include/nbody_hip.h, "binary census"): partner, energy and every field of
every NbodyBoundPair BIT FOR BIT against the numpy restatement (tests/pairs_ref.py) across the 64-lane and 256-body tile
edges; the same bits whatever the number of partner slices; ties and non-finite inputs; after a retain without a count call;
no trace in state or statistics; capacity and NULL forms; refusals; the command line."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pairs_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 64.0
CONFIGS = [("bf", False), ("bf", True), ("bh", False), ("bh", True)]
SIZES = [0, 1, 2, 63, 65, 301, 1500]


def settings(f64, **kw):
    """f64 handles run unsoftened (the planted binaries keep their Kepler elements), f32 handles with g_soft = 0.01"""
    return dict(dict(g=1.0, g_soft=0.0 if f64 else 0.01, dt=1.0 / 256, theta2=0.5), **kw)


def make(nb, rec, method="bf", st=None, width=WIDTH, math_mode=None, hermite=False, block=None, **kw):
    f64 = rec.dtype == nb.PARTICLE_DTYPE64
    bh = method == "bh"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE,
                        math_mode=nb.FAST if math_mode is None else math_mode, tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO,
                        capacity=max(len(rec), 4), **kw)
    sim.settings = nb.Settings(**(st or settings(f64)))
    sim.init()
    if hermite:
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
    return sim


@functools.lru_cache(maxsize=None)
def _bodies(n, f64):
    import __graft_entry__ as graft
    nb = graft.load_package()
    planted = {301: 6, 1500: 20, 3001: 20}.get(n, min(n // 2, 2))
    rec = ref.planted_bodies(nb, n, planted, seed=11 if n == 301 else 12 if n == 1500 else n + 7, f64=True)
    if not f64:
        rec32 = np.zeros(n, nb.PARTICLE_DTYPE)
        for f in ("position", "velocity", "mass"):
            rec32[f] = rec[f]
        rec = rec32
    rec.setflags(write=False)
    return rec


def bodies(n, f64):
    """the planted sets of tests/test_pairs_checker.py at n = 301 and 1500 (shared, read-only)"""
    return _bodies(n, f64)


@functools.lru_cache(maxsize=None)
def expected(n, f64, g, g_soft):
    """the restatement's (partner, energy, pairs, binding_sum) of bodies(n, f64), computed once"""
    rec = bodies(n, f64)
    return ref.partners(rec, g, g_soft) + ref.bound_pairs(rec, g, g_soft)


def check_against(got_partner, got_energy, got_pairs, got_sum, want):
    partner, energy, pairs, total = want
    assert got_partner.dtype == np.int32 and np.array_equal(got_partner, partner), "partner"
    assert ref.same_bits(got_energy, energy), "energy"
    assert len(got_pairs) == len(pairs), f"{len(got_pairs)} pairs, want {len(pairs)}"
    for f in ("i", "j"):
        assert np.array_equal(got_pairs[f], pairs[f]), f
    for f in ref.FIELDS[2:]:
        assert ref.same_bits(got_pairs[f], pairs[f]), f
    assert ref.same_bits(got_sum, total), "binding sum"


def census(sim):
    partner, energy = sim.partners()
    pairs, total = sim.bound_pairs()
    return partner, energy, pairs, total


def same_census(a, b, what):
    assert np.array_equal(a[0], b[0]) and ref.same_bits(a[1], b[1]), what
    assert len(a[2]) == len(b[2]) and a[2].tobytes() == b[2].tobytes(), what
    assert ref.same_bits(a[3], b[3]), what


def counters(s):
    return (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)


def same_records(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} against {len(b)} records"
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f}"


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("method,f64", CONFIGS, ids=[f"{m}-{'f64' if d else 'f32'}" for m, d in CONFIGS])
@pytest.mark.parametrize("n", SIZES)
def test_census_is_the_restatement_bit_for_bit(gpu, n, method, f64):
    nb = gpu
    rec = bodies(n, f64)
    with make(nb, rec, method) as sim:
        g, g_soft = ref.settings_of(sim)
        assert g_soft == (0.0 if f64 else float(np.float32(0.01)))
        got = census(sim)
        check_against(*got, expected(n, f64, g, g_soft))
        same_census(census(sim), got, "the same calls twice")
        if n >= 301 and f64:
            planted = {301: 6, 1500: 20}[n]
            listed = set(zip(got[2]["i"].tolist(), got[2]["j"].tolist()))
            assert all((2 * k, 2 * k + 1) in listed for k in range(planted))
            assert len(got[2]) == {301: 23, 1500: 69}[n]


def test_census_of_a_hermite_handle_is_of_the_held_state(gpu):
    nb = gpu
    rec = bodies(301, True)
    st = settings(True, g_soft=0.05, dt=1.0 / 1024)
    with make(nb, rec, st=st, hermite=True) as sim:
        sim.steps(1)
        got = census(sim)   # (before get_points: the calls must not need the count it refreshes)
        pts = sim.get_points()
        assert len(pts) == 301 and pts["position"].tobytes() != rec["position"].tobytes()
        ref.check_partners(got[0], got[1], pts, 1.0, 0.05)
        assert ref.check_bound_pairs(got[2], got[3], pts, 1.0, 0.05) > 0


# ------------------------------------------------------------------------------------------------ 2. independent of K
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1500, 3001])
def test_the_bits_do_not_depend_on_the_number_of_slices(gpu, n, f64):
    """bf64_waves = 64, the default (2048) and 20000: 2, 24 and 24 slices at n = 1500; 1, 42 and 47 at n = 3001"""
    nb = gpu
    rec = bodies(n, f64)
    got = []
    for knobs in ({"bf64_waves": 64}, None, {"bf64_waves": 20000}):
        with make(nb, rec, tuning=knobs) as sim:
            g, g_soft = ref.settings_of(sim)
            got.append(census(sim))
    same_census(got[0], got[1], "bf64_waves = 64 against the default")
    same_census(got[2], got[1], "bf64_waves = 20000 against the default")
    check_against(*got[0], expected(n, f64, g, g_soft))
    assert len(got[0][2]) > 20


# ------------------------------------------------------------------------------------------------ 3. ties, non-finite inputs
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_ties_give_the_lowest_index(gpu, f64):
    """5^3 equal masses at rest on an integer lattice: the six neighbours at distance 1 tie, many pairs at every distance tie"""
    nb = gpu
    lat = ref.lattice_bodies(nb, 5, f64)
    with make(nb, lat, st=settings(f64, g_soft=0.0)) as sim:
        got = census(sim)
    ref.check_partners(got[0], got[1], lat, 1.0, 0.0)
    ref.check_bound_pairs(got[2], got[3], lat, 1.0, 0.0)
    x = lat["position"].astype(np.float64)
    for i in (0, 1, 62, 124):
        near = [j for j in range(len(lat)) if j != i and np.abs(x[j] - x[i]).sum() == 1.0]
        assert got[0][i] == min(near) and got[1][i] == -0.5


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_non_finite_and_degenerate_inputs(gpu, f64):
    nb = gpu
    holed = bodies(65, f64).copy()
    holed["position"][7, 1] = np.nan
    st = settings(f64, g_soft=0.0)
    with make(nb, holed, st=st) as sim:
        got = census(sim)
    assert got[0][7] == -1 and got[1][7] == np.inf and 7 not in got[0]
    ref.check_partners(got[0], got[1], holed, 1.0, 0.0)
    ref.check_bound_pairs(got[2], got[3], holed, 1.0, 0.0)
    # every coordinate NaN: nobody has a partner
    dead = holed.copy()
    dead["position"][:, 0] = np.nan
    with make(nb, dead, st=st) as sim:
        got = census(sim)
    assert (got[0] == -1).all() and (got[1] == np.inf).all() and len(got[2]) == 0 and got[3] == 0.0
    # two bodies flying apart: partners, no bound pair
    two = bodies(2, f64).copy()
    two["velocity"][1] = two["velocity"][0] + 100.0
    with make(nb, two, st=st) as sim:
        got = census(sim)
    assert list(got[0]) == [1, 0] and got[1][0] == got[1][1] > 0 and len(got[2]) == 0 and got[3] == 0.0 and not np.signbit(got[3])
    ref.check_partners(got[0], got[1], two, 1.0, 0.0)
    # two coincident bodies without softening: -inf wins and is listed
    two["position"][1] = two["position"][0]
    with make(nb, two, st=st) as sim:
        got = census(sim)
    assert list(got[0]) == [1, 0] and (got[1] == -np.inf).all() and len(got[2]) == 1 and got[3] == -np.inf
    ref.check_bound_pairs(got[2], got[3], two, 1.0, 0.0)
    assert got[2]["semi_major"][0] == 0.0 and got[2]["separation"][0] == 0.0


# ------------------------------------------------------------------------------------------------ 4. after a retain
@pytest.mark.parametrize("method,f64", CONFIGS, ids=[f"{m}-{'f64' if d else 'f32'}" for m, d in CONFIGS])
def test_census_after_a_retain_without_a_count_call(gpu, method, f64):
    """a narrow box: the half drift's retain drops bodies, the host's view of the count stays an upper bound"""
    nb = gpu
    n = 1001
    rec = nb.plummer(n, seed=5, f64=f64)
    rec["mass"] = np.random.default_rng(5).uniform(0.5, 1.5, n) / n
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, method, st=st, width=1.5) as sim, make(nb, rec, method, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = census(sim)
        pts = twin.get_points()
        assert 0 < len(pts) < n - 10, len(pts)
        g, g_soft = ref.settings_of(sim)
        ref.check_partners(got[0], got[1], pts, g, g_soft)
        assert ref.check_bound_pairs(got[2], got[3], pts, g, g_soft) > 0
        with make(nb, pts, method, st=st, width=1.5) as fresh:
            same_census(census(fresh), got, "a fresh handle with the survivors")
        same_records(sim.get_points(), pts, "after the calls")


# ------------------------------------------------------------------------------------------------ 5. no trace
@pytest.mark.parametrize("which", ["bf-f32", "bh-f32", "hermite-block"])
def test_the_calls_leave_no_trace(gpu, which):
    nb = gpu
    hermite = which == "hermite-block"
    rec = bodies(301, hermite)
    st = settings(hermite, g_soft=0.05, dt=1.0 / 64 if hermite else 1.0 / 256)

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
        first = census(a)
        same_census(census(a), first, "the same calls twice")
        a.steps(3)
        never.steps(3)
        sa, sn = state(a), state(never)
        same_records(sa["records"], sn["records"], which)
        assert sa["stats"] == sn["stats"], which
        if hermite:
            assert ref.same_bits(sa["jerk"], sn["jerk"]) and np.array_equal(sa["levels"], sn["levels"]), which
            assert sa["block_counts"] == sn["block_counts"], which
        assert len(first[0]) == 301


# ------------------------------------------------------------------------------------------------ 6. capacity and NULL forms
def test_capacity_and_null_forms(gpu):
    nb = gpu
    rec = bodies(301, True)
    lib = nb.lib
    with make(nb, rec) as sim:
        h = sim._h
        g, g_soft = ref.settings_of(sim)
        want_p, want_e, want_pairs, want_sum = expected(301, True, g, g_soft)
        n = C.c_size_t(77)
        assert lib.nbody_partners(h, None, None, 0, C.byref(n)) == 0 and n.value == 301
        assert lib.nbody_partners(h, None, None, 0, None) == 0
        partner = np.full(301, -7, np.int32)
        energy = np.full(301, -7.0)
        n.value = 0
        assert lib.nbody_partners(h, partner.ctypes.data, energy.ctypes.data, 300, C.byref(n)) == nb.NBODY_ERR_CAPACITY
        assert n.value == 301 and b"nbody_partners" in lib.nbody_last_error(h) and (partner == -7).all() and (energy == -7.0).all()
        assert lib.nbody_partners(h, partner.ctypes.data, None, 301, C.byref(n)) == 0 and np.array_equal(partner, want_p)
        assert lib.nbody_partners(h, None, energy.ctypes.data, 301, None) == 0 and ref.same_bits(energy, want_e)
        # pairs
        k = len(want_pairs)
        total = C.c_double(-1.0)
        assert lib.nbody_bound_pairs(h, None, 0, C.byref(n), None) == 0 and n.value == k
        assert lib.nbody_bound_pairs(h, None, 0, C.byref(n), C.byref(total)) == 0 and n.value == k and ref.same_bits(total.value, want_sum)
        assert lib.nbody_bound_pairs(h, None, 0, None, None) == 0
        pairs = np.zeros(k, nb.BOUND_PAIR_DTYPE)
        n.value = 0
        assert lib.nbody_bound_pairs(h, pairs.ctypes.data, k - 1, C.byref(n), C.byref(total)) == nb.NBODY_ERR_CAPACITY
        assert n.value == k and b"nbody_bound_pairs" in lib.nbody_last_error(h) and not pairs["j"].any()
        assert lib.nbody_bound_pairs(h, pairs.ctypes.data, k, C.byref(n), None) == 0 and n.value == k
        assert pairs.tobytes() == want_pairs.tobytes()
        # the handle keeps working
        sim.steps(2)
        assert len(sim.get_points()) == 301


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_call(gpu):
    nb = gpu
    rec = bodies(65, False)
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, WIDTH, **kw) as sim:
            for call, name in ((sim.partners, "nbody_partners"), (sim.bound_pairs, "nbody_partners")):
                with pytest.raises(nb.NbodyError) as e:
                    call()
                assert e.value.code == nb.NBODY_ERR_INVALID and name in str(e.value), str(e.value)
            assert nb.lib.nbody_bound_pairs(sim._h, None, 0, None, None) == nb.NBODY_ERR_INVALID
            assert b"nbody_bound_pairs" in nb.lib.nbody_last_error(sim._h)


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_cli_prints_the_census(gpu):
    nb = gpu
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nbody-llm_amd", "nbody_cli")
    num = r"([-+0-9.eE]+|nan|-?inf)"
    for dtype in ("f32", "f64"):
        out = subprocess.run([cli, "-n", "500", "--ic", "plummer", "--method", "bf", "--steps", "0", "--dtype", dtype, "--pairs"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = re.findall(r"^Bound pairs: (\d+) binding %s hardest a=%s e=%s$" % (num, num, num), out.stdout, flags=re.M)
        assert len(rows) == 1 and "Diagnostics" not in out.stdout, out.stdout
        rec = nb.plummer(500, f64=dtype == "f64")
        with make(nb, rec, st=dict(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)) as sim:
            pairs, total = sim.bound_pairs()
        hard = pairs[np.argmin(pairs["binding"])]
        assert int(rows[0][0]) == len(pairs) > 0
        assert float(rows[0][1]) == pytest.approx(total, rel=1e-8) and float(rows[0][2]) == pytest.approx(hard["semi_major"], rel=1e-8)
        assert float(rows[0][3]) == pytest.approx(hard["eccentricity"], rel=1e-8, abs=1e-12)
