"""Tracers on the device: massless particles that feel the bodies and exert nothing (include/nbody_hip.h, "tracers").

Brute-force handles, both math modes: strict results are compared bit for bit with the CPU oracle on the world with the
tracers appended as zero-mass bodies; fast results with the probe technique of tests/bf_probe.py (one term per tracer) and
with the rounding-count bound of tests/tracer_ref.py (full sums).  Barnes-Hut handles: the tracer walk against the f64 sum
of its own node list (tests/bh_list.py), on the tree the body pass built."""
import ctypes as C

import numpy as np
import pytest

import tracer_ref
from bh_list import LIST_RTOL_F32, walk_errors
from bf_probe import PROBE_G, PROBE_MASS, PROBE_RTOL, probe_columns, probe_records, set_probe

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 8.0
FIELDS = ("position", "velocity", "acceleration")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_records(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} against {len(b)} records"
    for f in FIELDS:
        assert np.array_equal(bits(a[f]), bits(b[f])), f"{what}: {f} differs"


def tracer_records(dtype, m, seed, spread=2.0, speed=0.3):
    rng = np.random.default_rng(seed)
    t = np.zeros(m, dtype)
    t["position"] = rng.uniform(-spread, spread, (m, 3))
    t["velocity"] = rng.uniform(-speed, speed, (m, 3))
    t["mass"] = 7.0   # ignored on upload
    return t


def make(nb, bodies, math_mode, st, width=WIDTH, **kw):
    sim = nb.Simulation(bodies, CENTER, width, method=nb.BRUTE_FORCE, math_mode=math_mode, **kw)
    sim.settings = nb.Settings(**st)
    sim.init()
    return sim


# ---------------------------------------------------------------------------------------------- 1. strict, bit for bit
@pytest.mark.parametrize("m", [1, 63, 65, 300])
def test_strict_steps_equal_the_oracle_on_the_appended_world(gpu, orc, m):
    nb = gpu
    n = 64
    st = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    bodies = nb.plummer(n, seed=21).astype(orc.P32)
    bodies["position"] = np.clip(bodies["position"], -3.0, 3.0)   # (nobody else is near the walls)
    tracers = tracer_records(orc.P32, m, seed=m)
    # body 5 and tracer 0 run for the wall: they are outside at the half drift of the fifth step
    bodies["position"][5] = (3.65, 0.0, 0.0)
    bodies["velocity"][5] = (200.0, 0.0, 0.0)
    tracers["position"][0] = (0.0, 3.65, 0.0)
    tracers["velocity"][0] = (0.0, 200.0, 0.0)
    dts = [1e-3, 1e-3, -1e-3, 1e-3, 1e-3, 5e-4]
    world = tracer_ref.with_zero_mass(bodies, tracers)
    with make(nb, bodies, nb.STRICT, st) as sim, make(nb, bodies, nb.STRICT, st) as plain:
        sim.set_tracers(tracers)
        assert sim.n_tracers == m and len(sim) == n
        for k, dt in enumerate(dts):
            sim.step_by(dt)
            plain.step_by(dt)
            world = orc.bf_step_by(world, st, CENTER, WIDTH, dt)
            ref_b, ref_t = tracer_ref.split_back(world)
            got_b, got_t = sim.get_points(), sim.get_tracers()
            same_records(got_b, ref_b, f"step {k}: bodies against the oracle")
            same_records(got_t, ref_t, f"step {k}: tracers against the oracle")
            assert (got_t["mass"] == 0).all()
            same_records(got_b, plain.get_points(), f"step {k}: bodies against a handle without tracers")
            assert sim.n_tracers == len(ref_t) and len(sim) == len(ref_b)
        assert len(ref_b) == n - 1 and len(ref_t) == m - 1, "the scenario lost its escapes"


def test_strict_update_forces_past_one_tile(gpu, orc):
    nb = gpu
    n, m = 1025, 65   # one body more than the strict kernels' LDS tile
    st = dict(g=1.25, g_soft=0.01, dt=1e-3, theta2=0.5)
    bodies = nb.plummer(n, seed=4).astype(orc.P32)
    tracers = tracer_records(orc.P32, m, seed=8)
    world = tracer_ref.with_zero_mass(bodies, tracers)
    orc.bf_update_forces(world, st)
    ref_b, ref_t = tracer_ref.split_back(world)
    with make(nb, bodies, nb.STRICT, st) as sim:
        sim.set_tracers(tracers)
        sim.update_forces()
        same_records(sim.get_tracers(), ref_t, "tracers")
        same_records(sim.get_points(), ref_b, "bodies")
        assert sim.tracer_stats() == (m * n, 0)


# ---------------------------------------------------------------------------------------------- 2. fast: every pair once
# (the last two: two and four tracers per lane, which the plan picks from 2^17 and 2^19 tracers)
FAST_SHAPES = [(3, 5000), (1500, 7), (1025, 257), (3, 1 << 17), (3, 1 << 19)]


# probe only (5e8 pairs): two tracers per lane WITH planes (K = 4), and slices of 1 088 bodies, longer than one LDS tile
PLANES_AND_TILES = (4160, 1 << 17)


def slice_columns(nb, n, m):
    plan = nb.host_tracer_plan(m, n)
    return probe_columns(n, set_sizes=(plan["slice_len"],), n_random=8, every_below=80)


@pytest.mark.parametrize("eps", [0.0, 0.01])
@pytest.mark.parametrize("n,m", FAST_SHAPES + [PLANES_AND_TILES])
def test_fast_probe_every_pair_exactly_once(gpu, orc, n, m, eps):
    nb = gpu
    st = dict(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5)
    pos = nb.plummer(n, seed=n)["position"]
    tracers = tracer_records(orc.P32, m, seed=n + m)
    g64, e64, m64 = (float(np.float32(v)) for v in (PROBE_G, eps, PROBE_MASS))
    worst = 0.0
    with make(nb, set_probe(probe_records(orc.P32, pos), 0), nb.FAST, st) as sim:
        for k in slice_columns(nb, n, m):
            if eps > 0:
                tracers["position"][m // 2] = pos[k]   # a tracer sitting exactly on the only massive body
            sim.upload(set_probe(probe_records(orc.P32, pos), k))
            sim.set_tracers(tracers)
            sim.update_forces()
            got = sim.get_tracers()
            assert len(got) == m
            acc = got["acceleration"].astype(np.float64)
            d = pos[k].astype(np.float64) - tracers["position"].astype(np.float64)
            q = (d * d).sum(1) + e64 * e64
            q_safe = np.where(q > 0, q, 1.0)
            ref = (g64 * m64) * d / (q_safe * np.sqrt(q_safe))[:, None]
            assert np.isfinite(acc).all(), f"column {k}: non-finite tracer accelerations"
            den = np.linalg.norm(ref, axis=1)
            num = np.linalg.norm(acc - ref, axis=1)
            on_body = den == 0
            assert (num[on_body] == 0).all(), f"column {k}: a tracer on the body must get exactly 0"
            if eps > 0:
                assert on_body[m // 2] and (acc[m // 2] == 0).all()
            err = num[~on_body] / den[~on_body]
            assert (err <= PROBE_RTOL).all(), (f"column {k} of n={n}, m={m}: {int((err > PROBE_RTOL).sum())} tracers off, "
                                               f"worst {float(err.max())}")
            worst = max(worst, float(err.max()))
    print(f"tracer probe n={n} m={m} eps={eps}: worst relative error {worst:.3g} (PROBE_RTOL {PROBE_RTOL})")


# ---------------------------------------------------------------------------------------------- 3. fast: full sums
@pytest.mark.parametrize("eps", [0.0, 0.01])
@pytest.mark.parametrize("n,m", FAST_SHAPES)
def test_fast_full_sums(gpu, orc, n, m, eps):
    nb = gpu
    g = 1.25
    st = dict(g=g, g_soft=eps, dt=1e-3, theta2=0.5)
    rng = np.random.default_rng(n * 7 + m)
    bodies = nb.plummer(n, seed=n + 1).astype(orc.P32)
    bodies["mass"] = rng.uniform(0.1, 2.0, n)
    tracers = tracer_records(orc.P32, m, seed=m + 3)
    S, T = tracer_ref.pair_sums(bodies, tracers["position"], g, eps)
    with make(nb, bodies, nb.FAST, st) as sim:
        sim.set_tracers(tracers)
        sim.update_forces()
        first = sim.get_tracers()
        worst = tracer_ref.check_fast(first["acceleration"], S, T, n, g, f"n={n} m={m}")
        print(f"tracer full sums n={n} m={m} eps={eps}: worst ratio to the bound {worst:.3g} "
              f"(recorded WORST_OBSERVED {tracer_ref.WORST_OBSERVED})")
        sim.update_forces()
        same_records(sim.get_tracers(), first, "the same call twice")
        sim.set_tracers(tracers[::-1].copy())
        sim.update_forces()
        assert np.array_equal(bits(sim.get_tracers()["acceleration"]), bits(first["acceleration"][::-1])), "reversed tracers"
        # all masses zero: T == 0, exactly 0 for everybody
        zero = bodies.copy()
        zero["mass"] = 0
        sim.upload(zero)
        sim.update_forces()
        assert (sim.get_tracers()["acceleration"] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. no trace in the bodies
def test_no_trace_in_the_bodies_fast_brute_force(gpu, orc):
    nb = gpu
    st = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.5)
    bodies = nb.plummer(2048, seed=6).astype(orc.P32)
    tracers = tracer_records(orc.P32, 1000, seed=2)
    # (a box no body leaves, so that the interaction count below is 5 M N)
    with make(nb, bodies, nb.FAST, st, width=256.0) as a, make(nb, bodies, nb.FAST, st, width=256.0) as b:
        a.set_tracers(tracers)
        for _ in range(5):
            a.step_by(st["dt"])
            b.step_by(st["dt"])
        same_records(a.get_points(), b.get_points(), "bodies with and without tracers")
        sa, sb = a.stats(), b.stats()
        assert (sa.interactions, sa.node_visits, sa.steps) == (sb.interactions, sb.node_visits, sb.steps)
        assert a.tracer_stats() == (5 * 1000 * 2048, 0)
        assert len(a) == 2048 and a.count_global() == 2048
        a.reset_stats()
        assert a.tracer_stats() == (0, 0)


def bh_sim(nb, bodies, tree, leaf, st, box=((0.0, 0.0, 0.0), 64.0), **tuning):
    sim = nb.Simulation(bodies, *box, method=nb.BARNES_HUT, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if tree == "device" else nb.TREE_HOST,
                        leaf_mode=nb.LEAF_DIRECT if leaf == "direct" else nb.LEAF_REFERENCE, tuning=tuning)
    sim.settings = nb.Settings(**st)
    sim.init()
    return sim


def test_no_trace_in_the_bodies_fast_barnes_hut_device_build(gpu, orc):
    nb = gpu
    st = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
    bodies = nb.plummer(2048, seed=6).astype(orc.P32)
    tracers = tracer_records(orc.P32, 1000, seed=2)
    with bh_sim(nb, bodies, "device", "reference", st) as a, bh_sim(nb, bodies, "device", "reference", st) as b:
        a.set_tracers(tracers)
        for _ in range(5):
            a.step_by(st["dt"])
            b.step_by(st["dt"])
        same_records(a.get_points(), b.get_points(), "bodies with and without tracers")
        sa, sb = a.stats(), b.stats()
        assert (sa.interactions, sa.node_visits, sa.steps) == (sb.interactions, sb.node_visits, sb.steps)
        accepted, visited = a.tracer_stats()
        assert 0 < accepted <= visited
        assert a.n_tracers == 1000 and len(a) == len(b)
        assert not np.array_equal(a.get_tracers()["position"], tracers["position"]), "the tracers moved"


# ---------------------------------------------------------------------------------------------- 5. the Barnes-Hut tracer walk
BH_BOX = ((0.0, 0.0, 0.0), 64.0)


def bh_world(nb, orc, n=4097, m=1000, seed=41):
    """n Plummer bodies well inside BH_BOX; m tracers: half inside the cloud, a tenth far outside the populated part of the
    box, the rest in between, and tracer 7 exactly on body 11."""
    rec = nb.plummer(2 * n + 64, seed=seed).astype(orc.P32)
    rec = np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 20.0][:n])
    assert len(rec) == n
    rng = np.random.default_rng(seed + 1)
    t = np.zeros(m, orc.P32)
    pos = rng.uniform(-6.0, 6.0, (m, 3))
    pos[: m // 2] = rng.normal(0.0, 0.5, (m // 2, 3))
    far = rng.uniform(25.0, 31.0, (m // 10, 3)) * rng.choice([-1.0, 1.0], (m // 10, 3))
    pos[m // 2: m // 2 + m // 10] = far
    t["position"] = pos
    t["position"][7] = rec["position"][11]
    t["velocity"] = rng.uniform(-0.1, 0.1, (m, 3))
    return rec, t


def checked_tracer_walk(nb, orc, sim, leaf, theta2, g_soft, what):
    sim.settings = nb.Settings(1.0, g_soft, 1e-3, theta2)
    sim.reset_stats()
    sim.update_forces()
    got = sim.get_tracers()
    ref = orc.bh_walk_list(sim.tree(), got["position"], theta2, 1.0, g_soft, 1 if leaf == "direct" else 0, 16)
    err = walk_errors(got["acceleration"], ref)
    worst = float(err.max())
    print(f"\n[tracer walk] {what}: worst |a - S| / T {worst:.3e} (LIST_RTOL_F32 {LIST_RTOL_F32:g})")
    assert (err <= LIST_RTOL_F32).all(), f"{what}: {int((~(err <= LIST_RTOL_F32)).sum())} of {len(err)} tracers beyond the bound, worst {worst}"
    assert sim.tracer_stats() == (int(ref["accepted"].sum()), int(ref["visited"].sum())), what
    return got


@pytest.mark.parametrize("leaf", ["reference", "direct"])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_barnes_hut_tracer_walk(gpu, orc, tree, leaf):
    nb = gpu
    bodies, tracers = bh_world(nb, orc)
    st = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.25)
    with bh_sim(nb, bodies, tree, leaf, st) as sim, bh_sim(nb, bodies, tree, leaf, st) as plain:
        sim.set_tracers(tracers)
        for g_soft in (0.0, 0.01):
            got = checked_tracer_walk(nb, orc, sim, leaf, 0.25, g_soft, f"{tree} {leaf} g_soft={g_soft}")
            assert np.array_equal(bits(got["position"]), bits(tracers["position"])) and (got["mass"] == 0).all()
            assert np.isfinite(got["acceleration"]).all()
        # the bodies' pass is the one of a handle without tracers
        plain.settings = sim.settings
        plain.reset_stats()
        plain.update_forces()
        same_records(sim.get_points(), plain.get_points(), "bodies")
        sa, sb = sim.stats(), plain.stats()
        assert (sa.interactions, sa.node_visits) == (sb.interactions, sb.node_visits)


@pytest.mark.parametrize("split,m", [(1, 1000), (16, 100_000)])
def test_barnes_hut_tracer_walk_runs_of_segments(gpu, orc, split, m):
    """One segment (the walk stores its own sums) and 16 segments taken in 11 runs by 100 000 tracers (1 < runs < segments)."""
    nb = gpu
    bodies, tracers = bh_world(nb, orc, m=m, seed=43)
    st = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
    with bh_sim(nb, bodies, "device", "direct", st, bh_walk_split=split) as sim:
        sim.set_tracers(tracers)
        checked_tracer_walk(nb, orc, sim, "direct", 0.25, 0.01, f"bh_walk_split={split} m={m}")


# ---------------------------------------------------------------------------------------------- 6. stepping contracts
def runaways(tracers, k=5):
    """The first k tracers leave a box of width 8 within three steps of 2e-3."""
    tracers["position"][:k] = (3.9, 0.0, 0.0)
    tracers["position"][:k, 1] = np.linspace(-1.0, 1.0, k)
    tracers["velocity"][:k] = (40.0, 0.0, 0.0)
    return tracers


def test_tracers_are_read_after_a_replayed_run(gpu, orc):
    """Two bodies 2e-7 apart, the device build's second keys switched off: the build of every enqueued step raises its flag on
    the device and all later kernels, the tracers' included, do nothing until the host replays the steps on its own tree.  A
    tracer read that comes BEFORE any body read must wait for that: tracers, counters and bodies equal the host-build handle's."""
    nb = gpu
    st = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
    bodies = nb.plummer(500, seed=3).astype(orc.P32)
    bodies["position"][7] = bodies["position"][3] + np.float32(2e-7)
    bodies["velocity"][7] = bodies["velocity"][3]
    tracers = tracer_records(orc.P32, 300, seed=9)
    knobs = dict(tree_max_tie=1, bh_walk_split=4)   # (no second keys: any collision of the first keys is "too deep"; one split count for both)
    with bh_sim(nb, bodies, "device", "reference", st, **knobs) as a, bh_sim(nb, bodies, "host", "reference", st, **knobs) as b:
        a.set_tracers(tracers)
        b.set_tracers(tracers)
        a.steps(6)
        b.steps(6)
        assert a.n_tracers == b.n_tracers == 300
        ta = a.get_tracers()       # before any body-side read of a
        sa = a.tracer_stats()
        same_records(ta, b.get_tracers(), "tracers after a replayed run")
        assert sa == b.tracer_stats() and sa[0] > 0
        assert not np.array_equal(ta["position"], tracers["position"])
        same_records(a.get_points(), b.get_points(), "bodies after a replayed run")
        # a new set uploaded onto pending steps must not be moved by them
        a.steps(2)
        b.steps(2)
        a.set_tracers(tracers)
        b.set_tracers(tracers)
        same_records(a.get_tracers(), b.get_tracers(), "a set uploaded after enqueued steps")
        assert np.array_equal(bits(a.get_tracers()["position"]), bits(tracers["position"]))


@pytest.mark.parametrize("tree", ["host", "device"])
def test_stepping_contracts_fast_barnes_hut(gpu, orc, tree):
    nb = gpu
    n, m = 1500, 700
    st = dict(g=1.0, g_soft=0.01, dt=2e-3, theta2=0.25)
    bodies = nb.plummer(n, seed=n).astype(orc.P32)
    bodies = np.ascontiguousarray(bodies[np.abs(bodies["position"]).max(1) < 3.5])
    tracers = runaways(tracer_records(orc.P32, m, seed=m))
    box = (CENTER, WIDTH)
    with bh_sim(nb, bodies, tree, "reference", st, box=box) as a, bh_sim(nb, bodies, tree, "reference", st, box=box) as b:
        a.set_tracers(tracers)
        b.set_tracers(tracers, capacity=2 * m)
        a.steps(5)
        b.step_by(st["dt"])
        b.step_by(st["dt"])
        twin = b.clone()
        for s in (b, twin):
            for _ in range(3):
                s.step_by(st["dt"])
        assert a.n_tracers == m - 5, "the scenario lost its escapes"
        same_records(a.get_tracers(), b.get_tracers(), "steps(5) against five step_by: tracers")
        same_records(a.get_points(), b.get_points(), "steps(5) against five step_by: bodies")
        same_records(twin.get_tracers(), b.get_tracers(), "clone after two steps: tracers")
        same_records(twin.get_points(), b.get_points(), "clone after two steps: bodies")
        twin.close()
        assert np.isfinite(a.get_tracers()["acceleration"]).all() and a.get_tracers()["acceleration"].any()

@pytest.mark.parametrize("n,m", [(1500, 700), (300, 5000)])
def test_stepping_contracts_fast_brute_force(gpu, orc, n, m):
    nb = gpu
    st = dict(g=1.0, g_soft=0.01, dt=2e-3, theta2=0.5)
    bodies = nb.plummer(n, seed=n).astype(orc.P32)
    bodies = np.ascontiguousarray(bodies[np.abs(bodies["position"]).max(1) < 3.5])
    tracers = runaways(tracer_records(orc.P32, m, seed=m))
    # (tracers leave the box, and b's clone refreshes its host view of the count where a's never is: the plans do not depend on it)
    w = WIDTH
    with make(nb, bodies, nb.FAST, st, width=w) as a, make(nb, bodies, nb.FAST, st, width=w) as b, make(nb, bodies, nb.FAST, st, width=w) as never:
        a.set_tracers(tracers)
        b.set_tracers(tracers, capacity=2 * m)
        a.steps(5)
        b.step_by(st["dt"])
        b.step_by(st["dt"])
        twin = b.clone()
        for s in (b, twin):
            for _ in range(3):
                s.step_by(st["dt"])
        same_records(a.get_tracers(), b.get_tracers(), "steps(5) against five step_by: tracers")
        same_records(a.get_points(), b.get_points(), "steps(5) against five step_by: bodies")
        same_records(twin.get_tracers(), b.get_tracers(), "clone after two steps: tracers")
        same_records(twin.get_points(), b.get_points(), "clone after two steps: bodies")
        assert twin.n_tracers == m - 5 and a.n_tracers == m - 5, "the scenario lost its escapes"
        twin.close()
        # the tracers moved
        assert not np.array_equal(a.get_tracers()["position"], tracers["position"])
        # an empty set, then steps: a handle that never had tracers
        a.upload(bodies)
        assert a.n_tracers == m - 5, "uploading bodies anew keeps the tracers"
        same_records(a.get_tracers(), b.get_tracers(), "tracers after a body upload")
        # no tracers but room kept for some: nothing to step, and the room is there
        a.set_tracers(tracers[:0], capacity=m)
        assert a.n_tracers == 0 and len(a.get_tracers()) == 0
        a.step_by(st["dt"])
        never.step_by(st["dt"])
        a.set_tracers(tracers[:3], capacity=m)
        assert a.n_tracers == 3
        a.set_tracers(tracers[:0])
        assert a.n_tracers == 0 and len(a.get_tracers()) == 0
        a.steps(3)
        never.steps(3)
        same_records(a.get_points(), never.get_points(), "after removing the tracers")
        with pytest.raises(nb.NbodyError) as e:
            a.set_tracers(tracers, capacity=m - 1)
        assert e.value.code == -3 and "nbody_tracers_upload" in str(e.value)


# ---------------------------------------------------------------------------------------------- 7. refusals
def tracer_calls(nb, sim, rec):
    n = C.c_size_t(0)
    out = (C.c_uint64 * 2)()
    return {
        "nbody_tracers_upload": lambda: nb.lib.nbody_tracers_upload(sim._h, rec.ctypes.data, len(rec), rec.dtype.itemsize, 0),
        "nbody_tracers_download": lambda: nb.lib.nbody_tracers_download(sim._h, rec.ctypes.data, len(rec), rec.dtype.itemsize, C.byref(n)),
        "nbody_tracers_count": lambda: nb.lib.nbody_tracers_count(sim._h, C.byref(n)),
        "nbody_tracer_stats": lambda: nb.lib.nbody_tracer_stats(sim._h, out),
    }


@pytest.mark.parametrize("which", ["f64", "world of two"])
def test_refusals(gpu, orc, which):
    nb = gpu
    rec = tracer_records(nb.PARTICLE_DTYPE, 16, seed=1)
    if which == "f64":
        sim = nb.Simulation(nb.plummer(64, f64=True), CENTER, WIDTH, method=nb.BRUTE_FORCE, math_mode=nb.STRICT)
    else:
        sim = nb.Simulation(nb.plummer(64), CENTER, WIDTH, method=nb.BRUTE_FORCE, math_mode=nb.STRICT, rank=0, world_size=2)
    with sim:
        for name, call in tracer_calls(nb, sim, rec).items():
            assert call() == -1, f"{name} on a handle of {which}"
            assert name in (nb.lib.nbody_last_error(sim._h) or b"").decode()
