"""nbody_grid_poisson on the device (include/nbody_hip.h, "grid Poisson") against nbody_host_grid_poisson: phi equal byte for
byte on f32 and f64 handles and on a handle holding no body, periodic and isolated, up to the longest line a block can hold; the
plans of the knobs give the same bytes and the stats tell them apart; deposit, solve and sample against the three host calls;
no trace in the state or in later steps, right after a retain included; in place, capacity and refusals.  That the host call
is the numpy restatement and solves Poisson's equation is asserted on the CPU in tests/test_poisson_checker.py."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import poisson_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 64.0
SPACING, G = 0.375, 1.25
PERIODIC = ref.PERIODIC_SHAPES + ((4096, 2, 1), (1, 2, 4096), (32, 32, 32))   # 4096: the longest line a block holds, contiguous and most strided
ISOLATED = ((8, 4, 2), (16, 16, 1), (32, 32, 32), (2048, 1, 2))               # 2048 pads to the axis cap
PERIODIC_CASES = [(s, dict(periodic=True, green=gr, deconvolve=d)) for s in PERIODIC for gr in (ref.SPECTRAL, ref.DIFF2) for d in (0, 2)]
ISOLATED_CASES = [(s, dict(soften=e)) for s in ISOLATED for e in ref.SOFTENS]
TILES = (1, 16, 64)   # poisson_tile: the smallest, the default, the largest
PLANS = list(itertools.product((0, 1), TILES))


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


def make(nb, rec, width=WIDTH, st=None, **kw):
    sim = nb.Simulation(rec, CENTER, width, method=nb.BRUTE_FORCE, math_mode=nb.FAST, capacity=max(len(rec), 4), **kw)
    sim.settings = nb.Settings(**(st or dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5)))
    sim.init()
    return sim


@functools.lru_cache(maxsize=None)
def mass_of(shape):
    return ref.masses(shape, "random", seed=2)


@functools.lru_cache(maxsize=None)
def expected(shape, kw):
    """phi of the host call, computed once and left unchanged"""
    return _nb().host_grid_poisson(mass_of(shape), SPACING, G, **dict(kw))


def check(sim, shape, kw, what):
    got = sim.grid_poisson(mass_of(shape), SPACING, G, **kw)
    ref.same_bits(got, expected(shape, tuple(sorted(kw.items()))), what)
    return got


def same_records(a, b, what):
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


# ------------------------------------------------------------------------------------------------ 1. the host's bytes
@pytest.mark.parametrize("handle", ["f32", "f64", "empty"])
def test_phi_is_the_host_s_byte_for_byte(gpu, handle):
    nb = gpu
    rec = nb.plummer(257, seed=11, f64=handle == "f64")[: 0 if handle == "empty" else 257]
    with make(nb, rec) as sim:
        assert list(sim.grid_poisson_stats()) == [0, 0, 0, 0]
        for shape, kw in PERIODIC_CASES + ISOLATED_CASES:
            got = check(sim, shape, kw, f"{handle} {shape} {kw}")
            assert got.any()
        zero = sim.grid_poisson(np.zeros((16, 8, 4)), SPACING, G, soften=0.05)
        assert not zero.any() and not np.signbit(zero).any()
        zero = sim.grid_poisson(np.zeros((16, 8, 4)), SPACING, G, periodic=True)
        assert not zero.any() and not np.signbit(zero).any()
        same_records(sim.get_points(), rec, "the handle lends its stream and its memory only")
        assert int(sim.grid_poisson_stats()[0]) == 1


# ------------------------------------------------------------------------------------------------ 2. the plan does not show
def test_every_plan_gives_the_same_bytes_and_the_stats_tell_them_apart(gpu):
    nb = gpu
    cases = [((16, 8, 4), dict(periodic=True, green=ref.DIFF2, deconvolve=2)), ((32, 32, 32), dict(periodic=True)), ((32, 32, 32), dict(soften=0.05)),
             ((1, 2, 4096), dict(periodic=True)), ((4096, 2, 1), dict(periodic=True)), ((2048, 1, 2), dict(soften=0.0))]
    with make(nb, nb.plummer(64, seed=3)) as sim:
        assert [sim.get_tuning(k) for k in ("poisson_lds", "poisson_tile")] == [1, 16]
        for shape, kw in cases:
            launches = {}
            for lds, tile in PLANS:
                sim.set_tuning("poisson_lds", lds)
                sim.set_tuning("poisson_tile", tile)
                check(sim, shape, kw, f"plan {(lds, tile)} {shape} {kw}")
                stats = [int(v) for v in sim.grid_poisson_stats()]
                padded = [n if kw.get("periodic") or n == 1 else 2 * n for n in shape]
                assert stats[0] == 1 and stats[1] == (lds | tile << 1), (shape, lds, tile, stats)
                assert stats[3] == int(np.prod(padded)) * (2 if kw.get("periodic") else 3), (shape, stats)
                launches[(lds, tile)] = stats[2]
            transforms = 2 if kw.get("periodic") else 3
            axes = [n for n in padded if n > 1]
            assert all(launches[(1, t)] == transforms * len(axes) for t in TILES), launches                        # one launch per axis
            assert all(launches[(0, t)] == transforms * sum(n.bit_length() - 1 for n in axes) for t in TILES), launches   # one per stage
            assert launches[(1, 16)] < launches[(0, 16)]
        sim.set_tuning("poisson_tile", 48)   # rounded down to a power of two
        check(sim, (32, 32, 32), dict(periodic=True), "tile 48")
        assert int(sim.grid_poisson_stats()[1]) == (1 | 32 << 1)


# ------------------------------------------------------------------------------------------------ 3. a closed loop
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_deposit_solve_sample_is_the_host_s_byte_for_byte(gpu, f64):
    nb = gpu
    rec = nb.plummer(4099, seed=7, f64=f64)
    origin, spacing, dims = (-2.0, -2.0, -2.0), 0.125, (32, 32, 32)
    with make(nb, rec) as sim:
        now = sim.get_points()
        xyz, m = np.ascontiguousarray(now["position"], np.float64), np.ascontiguousarray(now["mass"], np.float64)
        for periodic in (False, True):
            mass, _ = sim.deposit(origin, spacing, dims, scheme=nb.DEPOSIT_CIC, periodic=periodic)
            phi = sim.grid_poisson(mass, spacing, 1.0, periodic=periodic, green=nb.POISSON_DIFF2 if periodic else 0)
            got = sim.grid_sample(phi, origin, spacing, scheme=nb.DEPOSIT_CIC, op=nb.SAMPLE_GRADIENT2, periodic=periodic)
            host_mass, _ = nb.host_deposit(xyz, m, origin, spacing, dims, scheme=nb.DEPOSIT_CIC, periodic=periodic)
            host_phi = nb.host_grid_poisson(host_mass, spacing, 1.0, periodic=periodic, green=nb.POISSON_DIFF2 if periodic else 0)
            want = nb.host_grid_sample(xyz, host_phi, origin, spacing, scheme=nb.DEPOSIT_CIC, op=nb.SAMPLE_GRADIENT2, periodic=periodic)
            ref.same_bits(mass, host_mass, f"deposit, periodic {periodic}")
            ref.same_bits(phi, host_phi, f"solve, periodic {periodic}")
            ref.same_bits(got[0], want[0], f"sample, periodic {periodic}")
            assert got[0].any() and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 4. no trace
def test_no_trace_in_state_stats_or_later_steps(gpu):
    nb = gpu
    rec = nb.plummer(4099, seed=7)

    def state(sim):
        s = sim.stats()
        return sim.get_points(), (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)

    with make(nb, rec) as sim, make(nb, rec) as never:
        sim.steps(2)
        never.steps(2)
        for lds, tile in PLANS:
            sim.set_tuning("poisson_lds", lds)
            sim.set_tuning("poisson_tile", tile)
            check(sim, (16, 8, 4), dict(periodic=True), "between steps")
            check(sim, (8, 4, 2), dict(soften=0.05), "between steps")
        sim.set_tuning("poisson_lds", 1)
        sim.set_tuning("poisson_tile", 16)
        for when in ("right after the calls", "three steps later"):
            a, b = state(sim), state(never)
            same_records(a[0], b[0], when)
            assert a[1] == b[1], when
            sim.steps(3)
            never.steps(3)
            check(sim, (32, 32, 32), dict(periodic=True), "interleaved")


def test_right_after_a_retain_inside_unsynchronised_steps(gpu):
    """a narrow box: the half drift's retain drops bodies inside steps(k) and no nbody_count follows before the solve"""
    nb = gpu
    rec = nb.plummer(700, seed=5)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    with make(nb, rec, width=1.5, st=st) as sim, make(nb, rec, width=1.5, st=st) as twin:
        sim.steps(4)
        twin.steps(4)
        check(sim, (16, 8, 4), dict(periodic=True, green=ref.DIFF2), "after a retain")   # (no count before it)
        check(sim, (16, 16, 1), dict(soften=0.0), "after a retain")
        now = twin.get_points()
        assert 0 < len(now) < 690
        same_records(sim.get_points(), now, "the state after the calls")
        sim.steps(2)
        twin.steps(2)
        same_records(sim.get_points(), twin.get_points(), "two steps later")


# ------------------------------------------------------------------------------------------------ 5. in place and errors
def test_in_place_capacity_and_refusals(gpu):
    nb = gpu
    shape = (16, 8, 4)
    m = mass_of(shape)
    with make(nb, nb.plummer(64, seed=3)) as sim:
        spec = nb.grid_spec((0, 0, 0), SPACING, shape)
        ps = nb.NbodyPoissonSpec(G, 0.05, 0, 0, (C.c_int32 * 2)(0, 0))
        buf = m.copy()
        assert nb.lib.nbody_grid_poisson(sim._h, C.byref(spec), C.byref(ps), buf.ctypes.data, buf.ctypes.data, buf.size) == nb.NBODY_OK
        ref.same_bits(buf, expected(shape, (("soften", 0.05),)), "mass is phi")
        phi = np.full(shape, 7.0)
        assert nb.lib.nbody_grid_poisson(sim._h, C.byref(spec), C.byref(ps), m.ctypes.data, phi.ctypes.data, m.size - 1) == nb.NBODY_ERR_CAPACITY
        assert (phi == 7.0).all() and b"nbody_grid_poisson" in nb.lib.nbody_last_error(sim._h)
        odd = nb.grid_spec((0, 0, 0), SPACING, (16, 8, 3))
        bad_ps = nb.NbodyPoissonSpec(G, 0.05, 1, 0, (C.c_int32 * 2)(0, 0))
        for s, p, mass, out in ((odd, ps, m, phi), (spec, bad_ps, m, phi), (spec, None, m, phi), (None, ps, m, phi), (spec, ps, None, phi), (spec, ps, m, None)):
            rc = nb.lib.nbody_grid_poisson(sim._h, C.byref(s) if s is not None else None, C.byref(p) if p is not None else None,
                                           mass.ctypes.data if mass is not None else None, out.ctypes.data if out is not None else None, m.size)
            assert rc == nb.NBODY_ERR_INVALID and b"nbody_grid_poisson:" in nb.lib.nbody_last_error(sim._h)
        assert (phi == 7.0).all(), "a refused call writes nothing"
        assert nb.lib.nbody_grid_poisson(None, C.byref(spec), C.byref(ps), m.ctypes.data, phi.ctypes.data, m.size) == nb.NBODY_ERR_INVALID
        with pytest.raises(nb.NbodyError):
            sim.grid_poisson(m, SPACING, G, periodic=True, soften=0.05)
        assert nb.lib.nbody_grid_poisson_stats(sim._h, None) == nb.NBODY_ERR_INVALID


def test_the_command_line_option(gpu):
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
        sim.init()
        for _ in range(2):
            sim.step()
        for name, kw in (("isolated", dict()), ("spectral", dict(periodic=True)), ("diff2", dict(periodic=True, green=nb.POISSON_DIFF2))):
            run = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "2", "--dtype", "f64", "--deposit", "cic:8:2",
                                  "--poisson", name], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr
            mass, _ = sim.deposit((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), scheme=nb.DEPOSIT_CIC, periodic=kw.get("periodic", False))
            phi = sim.grid_poisson(mass, 0.5, 1.0, **kw)
            m = re.search(r"^Poisson sum (\S+) min (\S+) at (\d+) (\d+) (\d+)$", run.stdout, flags=re.M)
            assert m and re.search(r"^Poisson: .* dims 8 8 8 ", run.stdout, flags=re.M), run.stdout
            total = 0.0
            for v in phi.reshape(-1):
                total += float(v)
            low = int(np.argmin(phi))
            assert float(m.group(1)) == total and float(m.group(2)) == phi.reshape(-1)[low], (name, run.stdout)
            assert tuple(int(m.group(k)) for k in (3, 4, 5)) == np.unravel_index(low, phi.shape), (name, run.stdout)
    assert subprocess.run([cli, "--deposit", "cic:8:2", "--poisson", "fourth"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([cli, "--poisson", "isolated"], capture_output=True, text=True, timeout=60).returncode == 2


def test_multi_rank_and_spatial_handles_are_refused(gpu):
    nb = gpu
    rec = nb.plummer(257, seed=11)
    m = mass_of((16, 8, 4))
    spec = nb.grid_spec((0, 0, 0), SPACING, m.shape)
    ps = nb.NbodyPoissonSpec(G, 0.0, 0, 0, (C.c_int32 * 2)(0, 0))
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, 64.0, **kw) as sim:
            phi = np.full(m.shape, 7.0)
            stats = (C.c_uint64 * 4)(9, 9, 9, 9)
            assert nb.lib.nbody_grid_poisson(sim._h, C.byref(spec), C.byref(ps), m.ctypes.data, phi.ctypes.data, m.size) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_poisson:" in nb.lib.nbody_last_error(sim._h) and (phi == 7.0).all(), kw
            assert nb.lib.nbody_grid_poisson_stats(sim._h, stats) == nb.NBODY_ERR_INVALID, kw
            assert b"nbody_grid_poisson_stats:" in nb.lib.nbody_last_error(sim._h) and list(stats) == [9, 9, 9, 9], kw
