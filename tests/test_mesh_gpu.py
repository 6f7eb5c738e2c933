"""Mesh gravity on the device (include/nbody_hip.h, "mesh gravity") against tests/mesh_ref.py, byte for byte: nbody_update_forces
and steps under the mesh on both dtypes, with and without bodies leaving; every plan of the knobs gives the same bytes and the
stats tell the plans apart; steps(k) against k step_by calls; the external field; tracers; no trace on handles that never set it;
every refusal; the command line and the mirrors.  That the restatement's loop is the leapfrog is asserted on the CPU in
tests/test_mesh_checker.py."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import external_ref
import mesh_ref
import pm_ref as ref

pytestmark = pytest.mark.gpu

CENTER, WIDE, NARROW = (0.0, 0.0, 0.0), 4.0e3, 4.0   # NARROW: the walls at -2 and 2, so that the retain removes bodies
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
WORLDS = ("n1", "n64", "n65", "w4099")
GRIDS = ("p8x8x8", "p16x8x4", "i8x4x2", "i32x32x32")
#: (world, its grids) of test 1: every world on every grid above, and the grids whose ignored axis is x or y under their own world
WORLD_GRIDS = tuple((w, GRIDS) for w in WORLDS) + ((ref.AXIS_WORLD, ref.AXIS_GRIDS),)
COMBOS = tuple(itertools.product(ref.SCHEMES, ref.GRADIENTS))
KNOBS = ("mesh_kick_fuse", "mesh_keep_kernel", "pm_share_sort", "pm_gather", "deposit_sort", "sample_sort", "poisson_lds")
G = 1.25            # the handle's g: what a pass reads
G_IGNORED = 77.0    # pm->poisson.g as set: what a pass does not read
DTS = (1.0 / 64, 1.0 / 32, 1.0 / 128, 3.0 / 256)


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


@functools.lru_cache(maxsize=None)
def world(name, f64):
    return ref.world(_nb(), name, f64)


def poisson_of(grid, gradient):
    if ref.GRIDS[grid][3]:
        return dict(green=ref.DIFF2, deconvolve=0, soften=0.0) if gradient == ref.GRADIENT2 else dict(green=ref.SPECTRAL, deconvolve=1, soften=0.0)
    return dict(green=0, deconvolve=0, soften=0.0 if gradient == ref.GRADIENT2 else 0.05)


def mesh_of(grid, scheme, gradient):
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid]
    return dict(origin=origin, spacing=spacing, dims=dims, g=G_IGNORED, scheme=scheme, gradient=gradient, periodic=periodic, project_axis=axis,
                **poisson_of(grid, gradient))


def make(nb, rec, width=WIDE, math=None, method=None, capacity=None, **kw):
    sim = nb.Simulation(rec, CENTER, width, method=nb.BRUTE_FORCE if method is None else method, math_mode=nb.FAST if math is None else math,
                        capacity=capacity or max(len(rec), 4), **kw)
    sim.settings = nb.Settings(g=G, g_soft=0.05, dt=DTS[0], theta2=0.5)
    sim.init()
    return sim


def want_step(rec, dts, width, grid, scheme, gradient, **kw):
    return mesh_ref.step(_nb(), rec, dts, -width / 2, width / 2, G, grid, scheme, gradient, **kw, **poisson_of(grid, gradient))


def same_records(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} bodies vs {len(b)}"
    for f in ("position", "velocity", "acceleration", "mass"):
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def set_plan(sim, plan):
    for knob, v in zip(KNOBS, plan):
        sim.set_tuning(knob, v)


def stats(sim):
    return [int(v) for v in sim.mesh_gravity_stats()]


# ------------------------------------------------------------------------------------------------ 1. update_forces
@DTYPES
@pytest.mark.parametrize("name,grids", WORLD_GRIDS, ids=[w for w, _ in WORLD_GRIDS])
def test_update_forces_leaves_the_rounded_host_field_in_the_acc_rows(gpu, name, grids, f64):
    nb = gpu
    rec = world(name, f64)
    with make(nb, rec) as sim:
        for grid, (scheme, gradient) in itertools.product(grids, COMBOS):
            what = f"{name} {grid} scheme {scheme} gradient {gradient}"
            sim.mesh_gravity = mesh_of(grid, scheme, gradient)
            sim.update_forces()
            got = sim.get_points()
            want = mesh_ref.forces(nb, rec, G, grid, scheme, gradient, **poisson_of(grid, gradient))
            assert got["acceleration"].tobytes() == want.tobytes(), f"{what}: against F(host_pm_field)"
            origin, spacing, dims, periodic, axis = ref.GRIDS[grid]
            dev = sim.pm_field(origin, spacing, dims, float(rec["position"].dtype.type(G)), scheme, gradient, periodic, project_axis=axis, phi=False,
                               **poisson_of(grid, gradient))[0]
            assert got["acceleration"].tobytes() == dev.astype(rec["position"].dtype).tobytes(), f"{what}: against F(pm_field) on the handle"
            for f in ("position", "velocity", "mass"):
                assert got[f].tobytes() == rec[f].tobytes(), f"{what}: {f} was touched"
            if grids is ref.AXIS_GRIDS:   # active rows and zero rows (that AXIS_WORLD meets every class: tests/test_pm_checker.py)
                host = nb.host_pm_field(*ref.bodies(rec), origin, spacing, dims, float(rec["position"].dtype.type(G)), scheme, gradient, periodic,
                                        project_axis=axis, **poisson_of(grid, gradient))
                idle = host[2] >= 2   # outside and skipped: +0.0
                assert not got["acceleration"][idle].any() and got["acceleration"][~idle].any(), what
                assert not got["acceleration"][:, axis].any() and not np.signbit(got["acceleration"][:, axis]).any(), what
        assert sim.stats().steps == 0


# ------------------------------------------------------------------------------------------------ 2. steps
@DTYPES
@pytest.mark.parametrize("width", [WIDE, NARROW], ids=["wide", "walls"])
@pytest.mark.parametrize("name", WORLDS)
def test_one_and_four_unequal_steps_are_the_restatement_s_bytes(gpu, name, width, f64):
    nb = gpu
    rec = world(name, f64)
    for k, (scheme, gradient) in enumerate(COMBOS):
        grid = GRIDS[k % len(GRIDS)]
        what = f"{name} width {width} {grid} scheme {scheme} gradient {gradient}"
        with make(nb, rec, width=width) as sim:
            sim.mesh_gravity = mesh_of(grid, scheme, gradient)
            sim.step_by(DTS[0])
            one = sim.get_points()
            same_records(one, want_step(rec, DTS[:1], width, grid, scheme, gradient), f"{what}: one step")
            for dt in DTS[1:]:
                sim.step_by(dt)
            four = sim.get_points()
            want = want_step(rec, DTS, width, grid, scheme, gradient)
            same_records(four, want, f"{what}: four steps")
            assert len(sim) == len(want) and sim.stats().steps == 4, what
            if width == NARROW and len(rec) >= 64:
                assert len(want) < len(rec) - 1, "the walls must remove more than the body that is not finite"


# ------------------------------------------------------------------------------------------------ 3. the plans
def plans():
    return list(itertools.product((1, 0), repeat=len(KNOBS)))


@DTYPES
@pytest.mark.parametrize("name,grid,scheme,gradient", [("n65", "i8x4x2", ref.TSC, ref.GRADIENT2), ("w4099", "i32x32x32", ref.CIC, ref.GRADIENT4),
                                                       ("w4099", "p16x8x4", ref.TSC, ref.GRADIENT4)])
def test_every_plan_gives_the_same_bytes_and_the_stats_tell_them_apart(gpu, name, grid, scheme, gradient, f64):
    nb = gpu
    rec = world(name, f64)
    want = want_step(rec, DTS[:2], NARROW, grid, scheme, gradient)
    isolated = not ref.GRIDS[grid][3]
    for plan in plans():
        fuse, keep, share, gather, dsort, ssort, lds = plan
        with make(nb, rec, width=NARROW) as sim:
            assert [sim.get_tuning(k) for k in KNOBS] == [1] * len(KNOBS)
            set_plan(sim, plan)
            sim.mesh_gravity = mesh_of(grid, scheme, gradient)
            assert stats(sim) == [0, 0, 0, 0]
            seen = []
            for dt in DTS[:2]:
                sim.step_by(dt)
                seen.append(stats(sim))
            same_records(sim.get_points(), want, f"{name} {grid} plan {plan}")
            shared = share and dsort and ssort
            assert seen[1][0] == 2 and seen[1][1] == (fuse | keep << 1 | (gather | (2 if shared else 0)) << 2), (plan, seen)
            first, second = seen[0][2], seen[1][2] - seen[0][2]
            assert (first, second) == ((3, 2 if keep else 3) if isolated else (2, 2)), (plan, seen)
            assert seen[0][3] == 1 and seen[1][3] == 1, (plan, seen)


@DTYPES
def test_the_resident_state_is_made_once_and_regrown_past_the_bound(gpu, f64):
    nb = gpu
    rec = world("w4099", f64)
    with make(nb, rec, capacity=len(rec) + 8) as sim:
        sim.mesh_gravity = mesh_of("i32x32x32", ref.CIC, ref.GRADIENT2)
        sim.steps(16)
        assert stats(sim)[0] == 16 and stats(sim)[2] == 3 + 2 * 15 and stats(sim)[3] == 1, stats(sim)
        now = sim.get_points()
        assert len(now) == len(rec) - 1   # (the body that is not finite left at the first retain)
        extra = now[:2].copy()
        extra["position"] += rec["position"].dtype.type(0.125)
        for k in range(2):     # the second one is past the bound the state was made for
            sim.add_point(extra[k])
        sim.step_by(DTS[1])
        assert stats(sim)[3] == 2 and stats(sim)[2] == 3 + 2 * 15 + 3, stats(sim)
        same_records(sim.get_points(), want_step(np.concatenate([now, extra]), DTS[1:2], WIDE, "i32x32x32", ref.CIC, ref.GRADIENT2), "after add_point")
        sim.mesh_gravity = mesh_of("p8x8x8", ref.CIC, ref.GRADIENT2)   # another spec: another state
        sim.update_forces()
        assert stats(sim)[3] == 3
        sim.mesh_gravity = None
        assert sim.mesh_gravity is None and stats(sim)[3] == 3


# ------------------------------------------------------------------------------------------------ 4. steps(k)
@DTYPES
@pytest.mark.parametrize("grid", ["p16x8x4", "i32x32x32"])
def test_unsynchronised_steps_are_step_by_calls_and_pm_field_follows(gpu, grid, f64):
    nb = gpu
    rec = world("w4099", f64)
    scheme, gradient = ref.TSC, ref.GRADIENT2
    with make(nb, rec, width=NARROW) as a, make(nb, rec, width=NARROW) as b:
        a.mesh_gravity = b.mesh_gravity = mesh_of(grid, scheme, gradient)
        a.steps(8)
        origin, spacing, dims, periodic, axis = ref.GRIDS[grid]
        acc = a.pm_field(origin, spacing, dims, G, scheme, gradient, periodic, project_axis=axis, phi=False, **poisson_of(grid, gradient))[0]   # (no count before it)
        for _ in range(8):
            b.step_by(DTS[0])
            len(b)
        now = b.get_points()
        same_records(a.get_points(), now, "steps(8) against eight step_by calls")
        assert 0 < len(now) < len(rec) - 1
        x, m = ref.bodies(now)
        ref.same_bits(acc, nb.host_pm_field(x, m, origin, spacing, dims, G, scheme, gradient, periodic, project_axis=axis, phi=False,
                                            **poisson_of(grid, gradient))[0], "pm_field right after steps(8)")
        same_records(now, want_step(rec, DTS[:1] * 8, NARROW, grid, scheme, gradient), "eight steps against the restatement")


# ------------------------------------------------------------------------------------------------ 5. the external field
@DTYPES
@pytest.mark.parametrize("fuse", [1, 0])
def test_the_external_field_is_added_to_the_mesh_pass(gpu, fuse, f64):
    nb = gpu
    rec = world("n65", f64)
    comps = external_ref.FIELDS["mix8"]
    for grid, scheme, gradient in (("p8x8x8", ref.CIC, ref.GRADIENT2), ("i8x4x2", ref.TSC, ref.GRADIENT4)):
        with make(nb, rec, width=NARROW) as sim:
            sim.set_tuning("mesh_kick_fuse", fuse)
            sim.external_field = external_ref.to_abi(nb, comps)
            sim.mesh_gravity = mesh_of(grid, scheme, gradient)
            sim.step_by(DTS[1])
            same_records(sim.get_points(), want_step(rec, DTS[1:2], NARROW, grid, scheme, gradient, ext=comps), f"{grid}: one step with mix8")
            sim.update_forces()
            now = sim.get_points()
            a = mesh_ref.forces(nb, now, G, grid, scheme, gradient, **poisson_of(grid, gradient))
            a = a + external_ref.acc(comps, now["position"].dtype.type(G), now["position"], now["position"].dtype)
            assert now["acceleration"].tobytes() == a.tobytes(), f"{grid}: update_forces with mix8"


# ------------------------------------------------------------------------------------------------ 6. tracers
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("with_ext", [False, True], ids=["mesh", "mesh+ext"])
def test_tracers_ride_in_the_mesh_field_at_their_own_positions(gpu, with_ext, fuse):
    nb = gpu
    rec = world("w4099", False)
    comps = external_ref.FIELDS["plummer"] if with_ext else None
    for grid, scheme, gradient in (("p16x8x4", ref.TSC, ref.GRADIENT2), ("i8x4x2", ref.CIC, ref.GRADIENT4), ("i32x32x32", ref.NGP, ref.GRADIENT2)):
        tracers = np.zeros(97, nb.PARTICLE_DTYPE)
        tracers["position"] = ref.caller_points(grid, 97)[:, :].astype(np.float32)   # some off the grid, one far away, one not finite
        tracers["velocity"] = np.random.default_rng(3).uniform(-1, 1, (97, 3)).astype(np.float32)
        with make(nb, rec, width=NARROW) as sim:
            sim.set_tuning("mesh_kick_fuse", fuse)
            sim.set_tracers(tracers)
            if comps:
                sim.external_field = external_ref.to_abi(nb, comps)
            sim.mesh_gravity = mesh_of(grid, scheme, gradient)
            before = sim.tracer_stats()
            for dt in DTS[:2]:
                sim.step_by(dt)
            want, want_tr = want_step(rec, DTS[:2], NARROW, grid, scheme, gradient, ext=comps, tracers=tracers)
            same_records(sim.get_points(), want, f"{grid}: the bodies")
            got_tr = sim.get_tracers()
            assert 0 < len(want_tr) < 97
            same_records(got_tr, want_tr, f"{grid}: the tracers")
            assert sim.tracer_stats() == before, "the tracer passes' pair statistics do not move under the mesh"
            sim.update_forces()
            now, tr = sim.get_points(), sim.get_tracers()
            x, m = ref.bodies(now)
            at = mesh_ref.field(nb, x, m, np.float32(G), grid, scheme, gradient, np.float32, points=tr["position"], **poisson_of(grid, gradient))
            if comps:
                at = at + external_ref.acc(comps, np.float32(G), tr["position"], np.float32)
            assert tr["acceleration"].tobytes() == at.tobytes(), f"{grid}: update_forces at the tracers"


def test_tracers_of_a_handle_without_bodies_get_a_zero_field(gpu):
    nb = gpu
    tracers = nb.plummer(97, seed=6)
    tracers["mass"] = 0.0
    with make(nb, np.zeros(0, nb.PARTICLE_DTYPE), capacity=4) as sim:
        sim.set_tracers(tracers)
        sim.mesh_gravity = mesh_of("i32x32x32", ref.CIC, ref.GRADIENT2)
        sim.step_by(DTS[0])
        got = sim.get_tracers()
        want = external_ref.leapfrog_orbits([], G, tracers, DTS[:1], -WIDE / 2, WIDE / 2)
        same_records(got, want, "no body: free flight")
        assert not np.signbit(got["acceleration"]).any()


# ------------------------------------------------------------------------------------------------ 7. no trace
@pytest.mark.parametrize("f64,math", [(False, "fast"), (False, "strict"), (True, "fast"), (True, "strict")])
def test_no_trace_on_handles_that_never_step_under_the_mesh(gpu, f64, math):
    nb = gpu
    rec = world("w4099", f64)
    mode = nb.FAST if math == "fast" else nb.STRICT
    grid, scheme, gradient = "i32x32x32", ref.TSC, ref.GRADIENT4

    def counters(sim):
        s = sim.stats()
        return s.steps, s.interactions, s.force_kernel_interactions

    with make(nb, rec, math=mode) as never, make(nb, rec, math=mode) as sim:
        sim.mesh_gravity = mesh_of(grid, scheme, gradient)
        got = sim.mesh_gravity
        assert got is not None and got[1].poisson.g == G_IGNORED and list(got[0].dims) == [32, 32, 32] and got[1].gradient == gradient
        sim.mesh_gravity = None   # set and cleared with no pass in between
        assert sim.mesh_gravity is None and stats(sim) == [0, 0, 0, 0]
        never.steps(2)
        sim.steps(2)
        same_records(sim.get_points(), never.get_points(), "set, cleared, two brute-force steps")
        assert counters(sim) == counters(never) and counters(sim)[1] > 0
        # the read-only calls return what they did before, with mesh gravity set
        e0, p0 = never.energy(), never.potentials()[0]
        sim.mesh_gravity = mesh_of(grid, scheme, gradient)
        assert sim.energy() == e0 and sim.potentials()[0].tobytes() == p0.tobytes()
        # under the mesh the interaction counters stand still, steps count as before, and a clone continues with the same bits
        c0 = counters(sim)
        sim.step_by(DTS[0])
        assert counters(sim) == (c0[0] + 1, c0[1], c0[2])
        with sim.clone() as twin:
            assert twin.mesh_gravity is not None and bytes(twin.mesh_gravity[0]) == bytes(sim.mesh_gravity[0]) and bytes(twin.mesh_gravity[1]) == bytes(sim.mesh_gravity[1])
            sim.steps(2)
            twin.steps(2)
            same_records(twin.get_points(), sim.get_points(), "a clone under the mesh")
        want = want_step(never.get_points(), DTS[:1] * 3, WIDE, grid, scheme, gradient)
        same_records(sim.get_points(), want, "three mesh steps after two brute-force ones")
        # ... and cleared again, the handle is a brute-force handle again
        sim.mesh_gravity = None
        sim.update_forces()
        with make(nb, sim.get_points(), math=mode) as fresh:
            fresh.update_forces()
            assert fresh.get_points()["acceleration"].tobytes() == sim.get_points()["acceleration"].tobytes()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_name_the_call_and_leave_the_handle_stepping(gpu):
    nb = gpu
    rec = world("n65", True)
    good = mesh_of("p8x8x8", ref.CIC, ref.GRADIENT2)

    def refused(sim, spec, pm, call=b"nbody_set_mesh_gravity:"):
        rc = nb.lib.nbody_set_mesh_gravity(sim._h, None if spec is None else C.byref(spec), None if pm is None else C.byref(pm))
        assert rc == nb.NBODY_ERR_INVALID and call in nb.lib.nbody_last_error(sim._h), (rc, nb.lib.nbody_last_error(sim._h))

    with make(nb, rec, width=NARROW) as sim:
        spec, pm = nb.mesh_gravity_specs(good)
        refused(sim, spec, None)
        refused(sim, None, pm)
        bad_specs = [dict(origin=(np.nan, 0, 0)), dict(spacing=0.0), dict(dims=(0, 8, 8)), dict(dims=(8, 6, 8)), dict(scheme=3), dict(project_axis=3)]
        for kw in bad_specs:
            refused(sim, nb.mesh_gravity_specs(dict(good, **kw))[0], pm)
        quantity = nb.mesh_gravity_specs(good)[0]
        quantity.quantity = nb.DEPOSIT_NUMBER
        refused(sim, quantity, pm)
        for kw in (dict(g=np.inf), dict(soften=0.1), dict(green=2), dict(deconvolve=3), dict(gradient=nb.SAMPLE_VALUE), dict(gradient=3)):
            refused(sim, spec, nb.mesh_gravity_specs(dict(good, **kw))[1])
        for k in range(3):
            bad = nb.mesh_gravity_specs(good)[1]
            bad.reserved[k] = 1
            refused(sim, spec, bad)
        refused(sim, nb.mesh_gravity_specs(dict(good, periodic=False))[0], nb.mesh_gravity_specs(dict(good, green=1))[1])
        assert sim.mesh_gravity is None and stats(sim) == [0, 0, 0, 0]
        assert nb.lib.nbody_mesh_gravity_stats(sim._h, None) == nb.NBODY_ERR_INVALID
        with pytest.raises(nb.NbodyError):
            sim.mesh_gravity = dict(good, gradient=nb.SAMPLE_VALUE)
        # Hermite, both ways round
        sim.integrator = nb.HERMITE4
        refused(sim, spec, pm)
        sim.integrator = nb.LEAPFROG
        sim.mesh_gravity = good
        with pytest.raises(nb.NbodyError):
            sim.integrator = nb.HERMITE4
        assert b"nbody_set_integrator" in nb.lib.nbody_last_error(sim._h)
        # the handle keeps working, under the setting that stood
        sim.step_by(DTS[0])
        same_records(sim.get_points(), want_step(rec, DTS[:1], NARROW, "p8x8x8", ref.CIC, ref.GRADIENT2), "after the refusals")
    spec, pm = nb.mesh_gravity_specs(good)
    on = C.c_int(5)
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    rec32 = nb.plummer(65)
    for kw in (dict(method=nb.BARNES_HUT, math_mode=nb.FAST), dict(method=nb.BARNES_HUT, math_mode=nb.STRICT),
               dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2), dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec32, CENTER, 64.0, **kw) as sim:
            refused(sim, spec, pm)
            refused(sim, None, None)
            assert nb.lib.nbody_get_mesh_gravity(sim._h, None, None, C.byref(on)) == nb.NBODY_ERR_INVALID and on.value == 5, kw
            assert b"nbody_get_mesh_gravity:" in nb.lib.nbody_last_error(sim._h), kw
            assert nb.lib.nbody_mesh_gravity_stats(sim._h, out) == nb.NBODY_ERR_INVALID and list(out) == [9, 9, 9, 9], kw
            assert b"nbody_mesh_gravity_stats:" in nb.lib.nbody_last_error(sim._h), kw
            if kw.get("world_size", 1) == 1 and "shard_mode" not in kw:
                sim.settings = nb.Settings(g=G, g_soft=0.05, dt=DTS[0], theta2=0.5)
                sim.init()
                sim.steps(1)   # a Barnes-Hut handle steps on as it did
                assert sim.stats().steps == 1
    assert nb.lib.nbody_set_mesh_gravity(None, C.byref(spec), C.byref(pm)) == nb.NBODY_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 9. the command line and the mirrors
def test_the_command_line_option(gpu):
    """nbody_cli --mesh goes through the C++ mirror (host/simulation.hpp): its bodies are the Python mirror's"""
    nb = gpu
    cli = os.path.join(os.path.dirname(nb.LIB_PATH), "nbody_cli")
    rec = nb.plummer(400, f64=True)   # the command line's seed is the mirror's default
    for arg, periodic, green, gradient in (("isolated:grad2", False, 0, nb.SAMPLE_GRADIENT2), ("diff2:grad2", True, nb.POISSON_DIFF2, nb.SAMPLE_GRADIENT2),
                                           ("spectral:grad4", True, nb.POISSON_SPECTRAL, nb.SAMPLE_GRADIENT4)):
        run = subprocess.run([cli, "-n", "400", "--ic", "plummer", "--method", "bf", "--steps", "3", "--dtype", "f64", "--deposit", "cic:8:2",
                              "--mesh", arg], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        m = re.search(r"^MESH: (\S+) gradient (\d) plan (\d+) passes (\d+) transforms (\d+) allocations (\d+)$", run.stdout, flags=re.M)
        assert m, run.stdout
        with nb.Simulation(rec, CENTER, 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
            sim.settings = nb.Settings(g=1.0, g_soft=0.02, dt=3e-2, theta2=1.0)   # the command line's
            sim.init()
            sim.mesh_gravity = dict(origin=(-2.0, -2.0, -2.0), spacing=0.5, dims=(8, 8, 8), scheme=nb.DEPOSIT_CIC, gradient=gradient, periodic=periodic,
                                    green=green)
            sim.steps(3)
            want = stats(sim)
            now = sim.get_points()
        assert m.group(1) == arg.split(":")[0] and int(m.group(2)) == gradient
        assert [int(m.group(k)) for k in (4, 3, 5, 6)] == want, (run.stdout, want)
        rows = re.findall(r"^MESH body (\d+)((?: \S+)+)$", run.stdout, flags=re.M)
        assert len(rows) == 8, run.stdout
        for i, (index, values) in enumerate(rows):
            assert int(index) == i
            assert np.array([float(v) for v in values.split()]).tobytes() == np.concatenate([now["position"][i], now["acceleration"][i]]).tobytes()
    assert subprocess.run([cli, "--deposit", "cic:8:2", "--mesh", "isolated:grad3"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([cli, "--mesh", "isolated:grad2"], capture_output=True, text=True, timeout=60).returncode == 2


def test_the_mirror_s_shapes(gpu):
    nb = gpu
    with make(nb, world("n65", True)) as sim:
        assert sim.mesh_gravity is None
        s = sim.mesh_gravity_stats()
        assert s.shape == (4,) and s.dtype == np.uint64 and not s.any()
        sim.mesh_gravity = dict(origin=(-2, -2, -2), spacing=0.5, dims=(8, 8, 8), periodic=True)
        spec, pm = sim.mesh_gravity
        assert isinstance(spec, nb.GridSpec) and isinstance(pm, nb.NbodyPmSpec) and pm.poisson.g == 1.0 and spec.scheme == nb.DEPOSIT_CIC
        sim.mesh_gravity = (spec, pm)   # the pair it returns is a value it takes
        sim.update_forces()
        assert [int(v) for v in sim.mesh_gravity_stats()] == [1, 1 | 2 | (1 | 2) << 2, 2, 1]
        for k in ("mesh_kick_fuse", "mesh_keep_kernel"):
            assert sim.get_tuning(k) == 1
