"""ABI behaviour around the hot path: strides, re-upload, capacity, error reporting, statistics."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)


def test_strided_upload_and_download(gpu):
    """Callers may embed PointParticle in a larger record: stride >= 40, multiple of 4."""
    nb = gpu
    n = 300
    ics = nb.plummer(n, seed=1)
    wide = np.zeros(n, dtype=np.dtype([("p", nb.PARTICLE_DTYPE), ("tag", "<i4", 2)]))
    wide["p"] = ics
    wide["tag"] = 7
    with nb.Simulation(ics[:1], *BOX, capacity=n) as sim:
        sim._check(nb.lib.nbody_upload(sim._h, wide.ctypes.data, n, wide.dtype.itemsize))
        out = np.zeros(n, dtype=wide.dtype)
        out["tag"] = 9
        got_n = C.c_size_t(0)
        sim._check(nb.lib.nbody_download(sim._h, out.ctypes.data, n, out.dtype.itemsize, C.byref(got_n)))
        assert got_n.value == n
        assert np.array_equal(out["p"], ics) and np.all(out["tag"] == 9)
        assert nb.lib.nbody_upload(sim._h, wide.ctypes.data, n, 38) == nb.NBODY_ERR_INVALID
        assert nb.lib.nbody_upload(sim._h, wide.ctypes.data, n + 1, 48) == nb.NBODY_ERR_CAPACITY
        small = np.zeros(10, dtype=nb.PARTICLE_DTYPE)
        assert nb.lib.nbody_download(sim._h, small.ctypes.data, 10, 40, C.byref(got_n)) == nb.NBODY_ERR_CAPACITY
        assert got_n.value == n and b"too small" in nb.lib.nbody_last_error(sim._h)


def test_reupload_replaces_the_body_vector(gpu, orc):
    nb = gpu
    a, b = nb.plummer(500, seed=1), nb.plummer(200, seed=2)
    sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    with nb.Simulation(a, *BOX, math_mode=nb.STRICT) as sim:
        sim.steps(2)
        sim._check(nb.lib.nbody_upload(sim._h, b.ctypes.data, len(b), 40))
        assert len(sim) == 200
        sim.steps(2)
        got = sim.get_points()
    ref = b.astype(orc.P32)
    for _ in range(2):
        ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], sd["dt"])
    assert np.array_equal(got["position"], ref["position"])


def test_step_without_bounds_is_an_error(gpu):
    nb = gpu
    h = C.c_void_p()
    cfg = nb.NbodyConfig(C.sizeof(nb.NbodyConfig), nb.BRUTE_FORCE, nb.STRICT, 0, -1, 0, 1, 0, 16, 0, 0)
    assert nb.lib.nbody_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert nb.lib.nbody_step_by(h, 1e-3) == nb.NBODY_ERR_INVALID
        assert b"nbody_set_bounds" in nb.lib.nbody_last_error(h)
        g, e, dt, t2 = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        assert nb.lib.nbody_get_settings(h, C.byref(g), C.byref(e), C.byref(dt), C.byref(t2)) == 0
        assert (g.value, e.value, dt.value, t2.value) == (1.0, 0.0, np.float32(1e-3), 0.5)   # shared.rs:69-78
    finally:
        nb.lib.nbody_destroy(h)


def test_device_ordinal_out_of_range(gpu):
    nb = gpu
    h = C.c_void_p()
    cfg = nb.NbodyConfig(C.sizeof(nb.NbodyConfig), 0, 0, 0, 99, 0, 1, 0, 16, 0, 0)
    assert nb.lib.nbody_create(C.byref(cfg), C.byref(h)) == nb.NBODY_ERR_INVALID
    assert b"out of range" in nb.lib.nbody_last_error(None)


def test_statistics_and_profiling(gpu):
    nb = gpu
    n = 4096
    with nb.Simulation(nb.plummer(n), *BOX, math_mode=nb.FAST) as sim:
        sim.steps(3)
        s = sim.stats()
        assert (s.steps, s.interactions, s.force_launches) == (3, 3 * n * (n - 1), 0)
        sim.set_profiling(True)
        sim.reset_stats()
        sim.steps(4)
        s = sim.stats()
        assert (s.steps, s.force_launches) == (4, 4) and s.force_kernel_ms > 0
        # the timed launch is the symmetric kernel's rotation: every pair of two DIFFERENT resident sets met symmetrically (6 of
        # the 8 sets' 8 partners at this size; the own-set and opposite-set pairs are the companion blocks' share)
        assert 0.7 * 4 * n * (n - 1) <= s.force_kernel_interactions <= 4 * n * (n - 1)
    with nb.Simulation(nb.plummer(n), *BOX, math_mode=nb.FAST, tuning=dict(sym_min_bodies=1 << 30)) as sim:   # the LDS-tiled kernel: one launch, all pairs
        sim.set_profiling(True)
        sim.steps(2)
        assert sim.stats().force_kernel_interactions == 2 * n * (n - 1)
        sim.reset_stats()
        assert sim.stats().steps == 0
    # f64 handles keep the same contract: set_profiling(k > 1) brackets every k-th force launch only
    with nb.Simulation(nb.plummer(n, f64=True), *BOX, method=nb.BARNES_HUT, math_mode=nb.FAST) as sim:
        sim.set_profiling(2)
        sim.steps(4)
        s = sim.stats()
        assert (s.steps, s.force_launches) == (4, 2) and s.force_kernel_ms > 0


def test_many_handles_share_a_device(gpu, orc):
    """The visualiser keeps a pristine clone beside the running simulation (vis.rs:43,217-220)."""
    nb = gpu
    sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    sims = [nb.Simulation(nb.plummer(128, seed=s), *BOX, math_mode=nb.STRICT) for s in range(6)]
    for k, s in enumerate(sims):
        s.steps(k + 1)
    for k, s in enumerate(sims):
        ref = nb.plummer(128, seed=k).astype(orc.P32)
        for _ in range(k + 1):
            ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], sd["dt"])
        assert np.array_equal(s.get_points()["position"], ref["position"])
        s.close()


@pytest.mark.parametrize("method", ["bf", "bh"])
def test_clone_of_a_handle_with_a_live_communicator(gpu, method):
    """`Clone` (shared.rs:80): the twin of a handle whose RCCL communicator is up (a world of one here) has the state
    but not the communicator, steps on its own, and leaves the original and its communicator usable."""
    nb = gpu
    ics = nb.plummer(3000, seed=81)
    m = nb.BRUTE_FORCE if method == "bf" else nb.BARNES_HUT
    with nb.Simulation(ics, (0, 0, 0), 64.0, method=m, math_mode=nb.FAST) as sim:
        sim.settings = nb.Settings(1.0, 0.01, 1e-3, 0.25)
        sim.comm_init(nb.comm_unique_id())
        sim.steps(3)
        twin = sim.clone()
        try:
            sim.steps(2)
            twin.steps(2)
            a, b = sim.get_points(), twin.get_points()
            assert sim.elapsed() == twin.elapsed()
            for f in ("position", "velocity", "acceleration", "mass"):
                assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f
            sim.steps(1)                      # the original's communicator survived the clone
            assert len(sim) == len(twin) == 3000
        finally:
            twin.close()


def test_strided_upload_and_download_f64(gpu):
    """The same on an f64 handle: an 80-byte PointParticle<f64,3> inside a 96-byte record; stride >= 80, multiple of 8."""
    nb = gpu
    n = 300
    ics = nb.plummer(n, seed=1, f64=True)
    wide = np.zeros(n, dtype=np.dtype([("p", nb.PARTICLE_DTYPE64), ("tag", "<i8", 2)]))
    assert wide.dtype.itemsize == 96
    wide["p"] = ics
    wide["tag"] = 7
    with nb.Simulation(ics[:1], *BOX, capacity=n) as sim:
        sim._check(nb.lib.nbody_upload(sim._h, wide.ctypes.data, n, wide.dtype.itemsize))
        out = np.zeros(n, dtype=wide.dtype)
        out["tag"] = 9
        got_n = C.c_size_t(0)
        sim._check(nb.lib.nbody_download(sim._h, out.ctypes.data, n, out.dtype.itemsize, C.byref(got_n)))
        assert got_n.value == n
        assert out["p"].tobytes() == ics.tobytes() and np.all(out["tag"] == 9)
        assert nb.lib.nbody_upload(sim._h, wide.ctypes.data, n, 72) == nb.NBODY_ERR_INVALID
        assert nb.lib.nbody_upload(sim._h, wide.ctypes.data, n, 84) == nb.NBODY_ERR_INVALID     # not a multiple of 8
        assert nb.lib.nbody_upload(sim._h, wide.ctypes.data, n + 1, 96) == nb.NBODY_ERR_CAPACITY
        small = np.zeros(10, dtype=nb.PARTICLE_DTYPE64)
        assert nb.lib.nbody_download(sim._h, small.ctypes.data, 10, 80, C.byref(got_n)) == nb.NBODY_ERR_CAPACITY
        assert got_n.value == n and b"too small" in nb.lib.nbody_last_error(sim._h)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_vec_surface_push_swap_remove_retain(gpu, orc, f64):
    """Vec::push / Vec::swap_remove / Vec::retain on one shard against a Python list, bit for bit in all ten fields.  Capacity
    1 025: the retain's tile_state has its second tile and the spare word, and the second push lands in that tile."""
    nb = gpu
    cap = 1025
    pool = nb.plummer(cap + 1, seed=5, f64=f64)
    pool["acceleration"] = pool["velocity"][::-1] * 0.25     # (all ten fields carry something to lose)
    model = list(range(cap - 2))     # the Vec, as indices into the pool

    def check(sim):
        got = sim.get_points()
        assert len(sim) == len(got) == len(model)
        assert _same_bits(got, pool[model])

    def swap_remove(k):
        model[k] = model[-1]
        model.pop()

    with nb.Simulation(pool[: cap - 2], *BOX, capacity=cap, method=nb.BRUTE_FORCE, math_mode=nb.STRICT) as sim:
        check(sim)
        for k in (cap - 2, cap - 1):
            sim.add_point(pool[k])
            model.append(k)
            check(sim)
        assert len(model) == cap
        assert nb.lib.nbody_add_point(sim._h, pool[cap:].ctypes.data) == nb.NBODY_ERR_CAPACITY
        check(sim)
        sim.remove_point(0)
        swap_remove(0)
        check(sim)
        sim.remove_point(len(model) - 1)
        swap_remove(len(model) - 1)
        check(sim)
        assert nb.lib.nbody_remove_point(sim._h, len(model)) == nb.NBODY_ERR_INVALID
        check(sim)

        # one step in a box that some bodies leave, chosen from the oracle: half of them lie outside this cube
        sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
        start = pool[model]
        width = float(np.float32(2.0 * np.median(np.abs(start["position"]).max(axis=1))))
        center = (0.0, 0.0, 0.0)
        ref = orc.bf_step_by(start.astype(orc.P64 if f64 else orc.P32), sd, center, width, sd["dt"])
        assert 0 < len(ref) < len(start)
        sim.set_bounds(center, width)
        sim.step()
        got = sim.get_points()
        assert len(sim) == len(got) == len(ref)
        for f in ("position", "velocity", "acceleration", "mass"):     # (the retain keeps the survivors' order)
            assert got[f].tobytes() == ref[f].tobytes(), f


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_clone_carries_the_host_view(gpu, f64):
    """`Clone` (shared.rs:80) takes the settings, the bounds, elapsed, the count and every body field along, and the twin then
    steps bit for bit like its source (Barnes-Hut, strict: the root cell of the next tree is the bounds the twin was given)."""
    nb = gpu
    ics = nb.plummer(301, seed=11, f64=f64)
    center, width = (0.5, -0.25, 0.125), 48.0
    with nb.Simulation(ics[:300], center, width, capacity=400, method=nb.BARNES_HUT, math_mode=nb.STRICT) as sim:
        sim.settings = nb.Settings(0.75, 0.015625, 0.001953125, 0.375)
        sim.steps(2)
        sim.add_point(ics[300])
        twin = sim.clone()
        try:
            assert twin.settings == sim.settings == nb.Settings(0.75, 0.015625, 0.001953125, 0.375)
            assert twin.elapsed() == sim.elapsed() == 2 * 0.001953125
            assert len(twin) == len(sim) == 301
            assert _same_bits(twin.get_points(), sim.get_points())
            sim.steps(2)
            twin.steps(2)
            assert twin.elapsed() == sim.elapsed()
            assert _same_bits(twin.get_points(), sim.get_points())
            (mm_a, depth_a), (mm_b, depth_b) = sim.tree_cells(), twin.tree_cells()
            assert _same_bits(mm_a, mm_b) and _same_bits(depth_a, depth_b)
            c = np.asarray(center, np.float32)
            assert np.array_equal(mm_b[0], np.concatenate([c - np.float32(24.0), c + np.float32(24.0)]))
        finally:
            twin.close()


REGROW_CONFIGS = ["bf-fast-f32", "bh-device-tracers-f32", "bf-hermite-block-f64", "bh-f64"]


def _regrow_handle(nb, config, bodies):
    f64 = config.endswith("f64")
    bh = config.startswith("bh")
    sim = nb.Simulation(bodies, *BOX, capacity=4096, f64=f64, method=nb.BARNES_HUT if bh else nb.BRUTE_FORCE, math_mode=nb.FAST,
                        tree_build=nb.TREE_DEVICE if config == "bh-device-tracers-f32" else nb.TREE_AUTO)
    sim.settings = nb.Settings(g=1.0, g_soft=0.05, dt=1.0 / 256, theta2=0.5)
    if config == "bf-hermite-block-f64":
        sim.integrator = nb.HERMITE4
        sim.block_steps = (0.02, 3)
    return sim


def _regrow_half(nb, sim, config, bodies, tracers, probes):
    """upload, three steps, every lazily allocating reader once: everything the caller can see afterwards, as bytes"""
    f64 = config.endswith("f64")
    bh = config.startswith("bh")
    sim.upload(bodies)
    if not f64:
        sim.set_tracers(tracers)
    sim.steps(3)
    seen = {"points": sim.get_points()}
    if not f64:
        seen["tracers"] = sim.get_tracers()
    for name, mode in [("pairs", nb.POTENTIAL_PAIRS)] + ([("tree", nb.POTENTIAL_TREE)] if bh else []):
        phi, counts = sim.potentials(mode)
        acc, fphi, fcounts = sim.field_at(probes, mode)
        tidal, tcounts = sim.tidal_at(probes, mode, counts=True)
        seen.update({f"phi-{name}": phi, f"field-acc-{name}": acc, f"field-phi-{name}": fphi, f"tidal-{name}": tidal,
                     f"counts-{name}": np.array([counts, fcounts, tcounts], np.uint64)})
    m = sim.moments()
    seen["moments"] = np.concatenate([[m.mass], m.com, m.momentum, m.angular_momentum, m.mass_dipole])
    radii, mass = sim.lagrangian_radii([0.1, 0.5, 0.9])
    seen["radii"] = np.append(radii, mass)
    seen["partner"], seen["partner-energy"] = sim.partners()
    seen["energy"] = np.array(sim.energy(), np.float64)
    return {k: (v.dtype.str, v.shape, np.ascontiguousarray(v).tobytes()) for k, v in seen.items()}


@pytest.mark.parametrize("config", REGROW_CONFIGS)
def test_every_regrow_path_gives_the_bits_of_a_fresh_handle(gpu, config):
    """A handle whose buffers were first sized for 200 bodies and 64 tracers and then regrown for 4 000 and 2 000 -- the body
    staging, the symmetric / plane / walk / tree buffers, the tracer arrays, planes and sort buffers, and the scratch of every
    reader -- reports, byte for byte, what a fresh handle reports that only ever saw the larger set: every downloaded array and
    every reader's output.  Then both are destroyed with every buffer live, created again, and the same holds once more."""
    nb = gpu
    f64 = config.endswith("f64")
    small, large = nb.plummer(200, seed=3, f64=f64), nb.plummer(4000, seed=4, f64=f64)
    rng = np.random.default_rng(17)
    tracers = np.zeros(2000, nb.PARTICLE_DTYPE)
    tracers["position"] = rng.uniform(-1.3, 1.3, (2000, 3))
    tracers["velocity"] = rng.uniform(-0.3, 0.3, (2000, 3))
    probes = rng.uniform(-1.5, 1.5, (100, 3))
    for _ in range(2):
        with _regrow_handle(nb, config, small) as a, _regrow_handle(nb, config, large) as b:
            _regrow_half(nb, a, config, small, tracers[:64], probes)
            got_a = _regrow_half(nb, a, config, large, tracers, probes)
            got_b = _regrow_half(nb, b, config, large, tracers, probes)
            assert got_a.keys() == got_b.keys()
            for key in got_a:
                assert got_a[key] == got_b[key], key
