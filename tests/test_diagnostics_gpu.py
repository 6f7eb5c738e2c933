"""nbody_moments and nbody_lagrangian_radii on the device (include/nbody_hip.h, "diagnostics of the state as a whole"): the
moments BIT FOR BIT against the numpy restatement (tests/diag_ref.py), the radii bit for bit where the prefixes are exact and
within the admissible sets of the stated prefix bound otherwise; after a retain without a count call; edge inputs; no trace in
state or statistics; refusals; conservation of P and L over a Hermite run; the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import diag_ref as ref
import test_diag_checker as checker

pytestmark = pytest.mark.gpu

CENTER, WIDTH = (0.0, 0.0, 0.0), 64.0
ST = dict(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5)
CONFIGS = ["bf-strict", "bf-fast", "bh-device", "hermite"]


def make(nb, rec, config, st=ST, width=WIDTH, capacity=None, block=None):
    bh = config == "bh-device"
    sim = nb.Simulation(rec, CENTER, width, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE,
                        math_mode=nb.STRICT if config == "bf-strict" else nb.FAST, tree_build=nb.TREE_DEVICE if bh else nb.TREE_AUTO,
                        capacity=capacity)
    sim.settings = nb.Settings(**st)
    sim.init()
    if config == "hermite":
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
    return sim


def handles():
    """(config, f64) the diagnostics are checked on: every config on both dtypes, the Hermite integrator where it exists (f64)"""
    return [(c, f64) for c in CONFIGS for f64 in (False, True) if f64 or c != "hermite"]


def ids(p):
    return [f"{c}-{'f64' if f64 else 'f32'}" for c, f64 in p]


def counters(s):
    return (s.steps, s.interactions, s.node_visits, s.tree_nodes, s.force_kernel_interactions)


def same_records(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} against {len(b)} records"
    for f in ("position", "velocity", "acceleration", "mass"):
        assert ref.same_bits(a[f], b[f]) if a[f].dtype == np.float64 else np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f}"


# ---------------------------------------------------------------------------------------------- 1. moments, bit for bit
@pytest.mark.parametrize("config,f64", handles(), ids=ids(handles()))
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1001])
def test_moments_are_the_restatement_bit_for_bit(gpu, n, config, f64):
    nb = gpu
    rec = checker.bodies(nb, n, seed=n + 3, f64=f64)
    with make(nb, rec, config, capacity=max(n, 4)) as sim:
        mom = sim.moments()
        ref.check_moments(ref.raw(mom), rec)
        if n:
            assert mom.mass > 0 and ref.same_bits(mom.com, mom.mass_dipole / mom.mass) and mom.angular_momentum.any()
        else:
            assert not ref.raw(mom).any() and not np.signbit(ref.raw(mom)).any()
        sim.steps(3)
        got = ref.raw(sim.moments())   # (before get_points: the call must not need the count it refreshes)
        pts = sim.get_points()
        assert len(pts) == n
        ref.check_moments(got, pts)
        assert ref.same_bits(ref.raw(sim.moments()), got), "the same call twice"
        if n > 2:
            assert not ref.same_bits(got, ref.moments(rec)), "the steps moved nothing"


@pytest.mark.parametrize("config,f64", [("bf-fast", False), ("bf-fast", True), ("bh-device", False), ("bh-device", True)],
                         ids=["bf-fast-f32", "bf-fast-f64", "bh-device-f32", "bh-device-f64"])
def test_moments_and_radii_after_a_retain_without_a_count_call(gpu, config, f64):
    """a narrow box: the half drift's retain drops bodies, the host's view of the count stays an upper bound"""
    nb = gpu
    n = 1001
    rec = checker.bodies(nb, n, seed=5, f64=f64)
    st = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    fr = [0.0, 0.1, 0.5, 0.9, 1.0]
    with make(nb, rec, config, st=st, width=1.5) as sim, make(nb, rec, config, st=st, width=1.5) as twin:
        sim.steps(4)
        twin.steps(4)
        got = ref.raw(sim.moments())
        radii, mass = sim.lagrangian_radii(fr)
        radii_at, mass_at = sim.lagrangian_radii(fr, center=(0.1, 0.0, 0.0))
        pts = twin.get_points()
        assert 0 < len(pts) < n - 10, len(pts)
        ref.check_moments(got, pts)
        ref.check_radii_admissible(radii, mass, pts, ref.center_of_mass(pts), fr)
        ref.check_radii_admissible(radii_at, mass_at, pts, (0.1, 0.0, 0.0), fr)
        same_records(sim.get_points(), pts, "after the calls")


# ---------------------------------------------------------------------------------------------- 2. radii
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 257, 1001])
def test_radii_with_exact_prefixes_bit_for_bit(gpu, n, f64):
    """masses that are integer multiples of 2^-20 and sum to a power of two: every prefix and every target is exact, the answer
    unique; fractions 0, 1, 0.5, on a prefix and one ulp either side of it"""
    nb = gpu
    rec = ref.exact_mass_bodies(nb, n, seed=n, f64=f64)
    with make(nb, rec, "bf-strict") as sim:
        for center in ((0.05, -0.1, 0.02), None):
            at = ref.center_of_mass(rec) if center is None else center
            fr = ref.exact_fractions(rec, at)
            radii, mass = sim.lagrangian_radii(fr, center=center)
            ref.check_radii_exact(radii, mass, rec, at, fr)
            again, mass2 = sim.lagrangian_radii(fr, center=center)
            assert ref.same_bits(again, radii) and mass2 == mass
        none, mass = sim.lagrangian_radii([])
        assert none.shape == (0,) and mass == rec["mass"].astype(np.float64).sum()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_radii_of_a_mirrored_set_keep_ascending_index_in_ties(gpu, f64):
    """bodies mirrored through the centre share r2 bit for bit; the order is (r2, index), as the restatement's stable sort has
    it (the radius itself cannot tell the two bodies of a pair apart: what is checked is that ties disturb nothing)"""
    nb = gpu
    rec = ref.exact_mass_bodies(nb, 514, seed=77, f64=f64)
    rec["position"][257:] = -rec["position"][:257]
    r2 = ref.r2_of(rec, CENTER)
    assert np.array_equal(r2[:257], r2[257:])
    fr = ref.exact_fractions(rec, CENTER)
    with make(nb, rec, "bf-strict") as sim:
        radii, mass = sim.lagrangian_radii(fr, center=CENTER)
    ref.check_radii_exact(radii, mass, rec, CENTER, fr)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_radii_with_general_masses_are_admissible(gpu, f64):
    nb = gpu
    rec = checker.general_bodies(nb, f64)
    fr = checker.GENERAL_FRACTIONS
    with make(nb, rec, "bf-fast") as sim:
        for center in (None, (0.1, 0.0, -0.2)):
            at = ref.center_of_mass(rec) if center is None else center
            radii, mass = sim.lagrangian_radii(fr, center=center)
            loose = ref.check_radii_admissible(radii, mass, rec, at, fr)
            assert loose <= len(fr) // 100
            assert (np.diff(radii[:201]) >= 0).all() and radii[200] == np.sqrt(ref.r2_of(rec, at)).max()
            again, mass2 = sim.lagrangian_radii(fr, center=center)
            assert ref.same_bits(again, radii) and ref.same_bits(mass2, mass), "the same call twice"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_radii_edge_inputs(gpu, f64):
    nb = gpu
    rec = ref.exact_mass_bodies(nb, 257, seed=4, f64=f64)
    with make(nb, rec, "bf-strict") as sim:
        # center=None against the explicit X / M
        com = ref.center_of_mass(rec)
        fr = ref.exact_fractions(rec, com)
        a, ma = sim.lagrangian_radii(fr)
        b, mb = sim.lagrangian_radii(fr, center=com)
        assert ref.same_bits(a, b) and ma == mb
        assert ref.same_bits(sim.moments().com, com)
    holed = rec.copy()
    holed["position"][7, 1] = np.nan
    holed["position"][11, 0] = np.inf
    with make(nb, holed, "bf-strict") as sim:
        fr = [0.0, 0.5, 1.0]
        radii, mass = sim.lagrangian_radii(fr, center=CENTER)
        ref.check_radii_exact(radii, mass, holed, CENTER, fr)
        assert mass == rec["mass"].astype(np.float64).sum() - float(holed["mass"][7]) and radii[2] == np.inf and np.isfinite(radii[:2]).all()
        # the centre of mass of this set is NaN: no body is left in the order
        radii, mass = sim.lagrangian_radii(fr)
        assert np.isnan(radii).all() and mass == 0.0
    with make(nb, rec[:0], "bf-strict", capacity=4) as sim:
        for center in (None, CENTER):
            radii, mass = sim.lagrangian_radii([0.0, 0.5, 1.0], center=center)
            assert np.isnan(radii).all() and mass == 0.0


# ---------------------------------------------------------------------------------------------- 3. no trace
def tracer_records(nb, m, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(m, nb.PARTICLE_DTYPE)
    t["position"] = rng.uniform(-1.3, 1.3, (m, 3))
    t["velocity"] = rng.uniform(-0.3, 0.3, (m, 3))
    return t


@pytest.mark.parametrize("which", ["bf-fast", "bh-device-tracers-field", "hermite-block"])
def test_the_calls_leave_no_trace_and_a_clone_continues(gpu, which):
    nb = gpu
    hermite = which == "hermite-block"
    n = 256 if hermite else 1500
    rec = checker.bodies(nb, n, seed=14, f64=hermite)
    st = dict(ST, dt=1.0 / 64) if hermite else ST
    config = {"bf-fast": "bf-fast", "bh-device-tracers-field": "bh-device", "hermite-block": "hermite"}[which]

    def build():
        sim = make(nb, rec, config, st=st, block=(0.02, 4))
        if which == "bh-device-tracers-field":
            sim.set_tracers(tracer_records(nb, 300, seed=2))
            sim.external_field = [nb.external_component(nb.EXT_HERNQUIST, (5.0, 1.5), (0.2, 0.0, 0.0))]
        return sim

    def state(sim):
        out = {"records": sim.get_points(), "stats": counters(sim.stats())}
        if which == "bh-device-tracers-field":
            out["tracers"] = sim.get_tracers()
            out["tracer_stats"] = sim.tracer_stats()
        if hermite:
            out["jerk"] = sim.jerk()
            out["levels"] = sim.levels()
            out["block_counts"] = sim.block_step_counts()
        return out

    def same_state(a, b, what):
        same_records(a["records"], b["records"], what)
        assert a["stats"] == b["stats"], what
        if "tracers" in a:
            same_records(a["tracers"], b["tracers"], what + ": tracers")
            assert a["tracer_stats"] == b["tracer_stats"], what
        if "jerk" in a:
            assert ref.same_bits(a["jerk"], b["jerk"]) and np.array_equal(a["levels"], b["levels"]), what
            assert a["block_counts"] == b["block_counts"], what

    fr = [0.1, 0.5, 0.9]
    with build() as a, build() as never:
        a.steps(3)
        never.steps(3)
        mom = ref.raw(a.moments())
        radii, mass = a.lagrangian_radii(fr)
        a.lagrangian_radii(fr, center=(0.0, 0.1, 0.0))
        a.steps(3)
        never.steps(3)
        sa, sn = state(a), state(never)
        same_state(sa, sn, which)
        assert np.isfinite(mom).all() and np.isfinite(radii).all() and mass > 0
        # the calls on the state as it is now, then a clone: it continues like its source and like the twin
        ref.check_moments(ref.raw(a.moments()), sa["records"])
        a.lagrangian_radii(fr)
        with a.clone() as b:
            for sim in (a, b, never):
                sim.steps(2)
            sb = state(b)
            sb["stats"] = state(a)["stats"]   # (a clone starts with fresh statistics)
            if "tracer_stats" in sb:
                sb["tracer_stats"] = state(a)["tracer_stats"]
            if "block_counts" in sb:
                sb["block_counts"] = state(a)["block_counts"]
            same_state(state(a), sb, which + ": clone")
            same_state(state(a), state(never), which + ": after the clone")


# ---------------------------------------------------------------------------------------------- 4. refusals
def refused(nb, call, needle):
    with pytest.raises(nb.NbodyError) as e:
        call()
    assert e.value.code == nb.NBODY_ERR_INVALID, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_refusals_name_the_call_and_leave_the_handle_working(gpu):
    import ctypes as C
    nb = gpu
    rec = checker.bodies(nb, 65, seed=1, f64=False)
    for kw in (dict(method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=0, world_size=2),
               dict(method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL)):
        with nb.Simulation(rec, CENTER, WIDTH, **kw) as sim:
            refused(nb, sim.moments, "nbody_moments")
            refused(nb, lambda: sim.lagrangian_radii([0.5]), "nbody_lagrangian_radii")
    with make(nb, rec, "bf-fast") as sim, make(nb, rec, "bf-fast") as twin:
        for bad in ([-0.1], [1.0 + 2.0 ** -52], [np.nan], [0.5, np.inf], [0.5, -np.inf, 0.2]):
            refused(nb, lambda: sim.lagrangian_radii(bad), "nbody_lagrangian_radii")
        lib, h = nb.lib, sim._h
        fr = np.array([0.5, 1.0])
        out = np.zeros(2)
        mass = C.c_double(-1.0)
        assert lib.nbody_lagrangian_radii(h, None, None, 2, out.ctypes.data, C.byref(mass)) == nb.NBODY_ERR_INVALID
        assert b"nbody_lagrangian_radii" in lib.nbody_last_error(h)
        assert lib.nbody_lagrangian_radii(h, None, fr.ctypes.data, 2, None, C.byref(mass)) == nb.NBODY_ERR_INVALID
        assert lib.nbody_lagrangian_radii(h, None, fr.ctypes.data, (1 << 20) + 1, out.ctypes.data, None) == nb.NBODY_ERR_INVALID
        assert b"2^20" in lib.nbody_last_error(h)
        assert lib.nbody_moments(h, None) == nb.NBODY_ERR_INVALID and b"nbody_moments" in lib.nbody_last_error(h)
        assert mass.value == -1.0
        # n_frac == 0 is valid, with or without buffers; mass_out may be NULL
        assert lib.nbody_lagrangian_radii(h, None, None, 0, None, C.byref(mass)) == 0 and mass.value > 0
        assert lib.nbody_lagrangian_radii(h, None, fr.ctypes.data, 2, out.ctypes.data, None) == 0 and out[1] >= out[0] > 0
        # the handle keeps working
        sim.steps(2)
        twin.steps(2)
        same_records(sim.get_points(), twin.get_points(), "after the refusals")
        ref.check_moments(ref.raw(sim.moments()), twin.get_points())


# ---------------------------------------------------------------------------------------------- 5. physics
def test_a_hermite_run_conserves_momentum_and_angular_momentum(gpu):
    """256 bodies, f64, Hermite, 100 steps: pair forces are antisymmetric, so P and L move by rounding only -- less than
    1e-10 of sum m |v| and of sum m |x| |v|"""
    nb = gpu
    rec = checker.bodies(nb, 256, seed=21, f64=True)
    x, v, m = (rec[k].astype(np.float64) for k in ("position", "velocity", "mass"))
    p_scale = (m * np.linalg.norm(v, axis=1)).sum()
    l_scale = (m * np.linalg.norm(x, axis=1) * np.linalg.norm(v, axis=1)).sum()
    with make(nb, rec, "hermite") as sim:
        before = sim.moments()
        sim.steps(100)
        after = sim.moments()
    dp = np.abs(after.momentum - before.momentum).max() / p_scale
    dl = np.abs(after.angular_momentum - before.angular_momentum).max() / l_scale
    print(f"relative drift over 100 Hermite steps: P {dp:.3g}, L {dl:.3g}; M {before.mass!r} -> {after.mass!r}")
    assert after.mass == before.mass
    assert np.abs(after.com - before.com).max() > 1e-6, "the cluster did not move"
    assert dp < 1e-10 and dl < 1e-10


# ---------------------------------------------------------------------------------------------- 6. the command line
def test_cli_prints_the_diagnostics(gpu):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nbody-llm_amd", "nbody_cli")
    num = r"([-+0-9.eE]+|nan|inf)"
    for dtype in ("f32", "f64"):
        out = subprocess.run([cli, "-n", "500", "--steps", "5", "--dtype", dtype, "--diagnostics"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = re.findall(r"Diagnostics (before|after): M %s  \|P\| %s  \|L\| %s  r10 %s  r50 %s  r90 %s  mass in radii %s" % ((num,) * 7), out.stdout)
        assert [r[0] for r in rows] == ["before", "after"], out.stdout
        for r in rows:
            mass, p, l, r10, r50, r90, inside = (float(v) for v in r[1:])
            assert mass == pytest.approx(1.2, rel=1e-5) and inside == pytest.approx(mass, rel=1e-12) and l > 0 and 0 <= r10 <= r50 <= r90 and r90 > 0
        assert rows[0] != rows[1]
