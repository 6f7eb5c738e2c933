"""NBODY_MATH_FAST on f64 brute-force handles (kernels_bf64.hip): k_bf64_sym evaluates every unordered pair once, the
one-sided k_bf64_os takes the pairs it leaves over (or every pair below Tuning::bf64_min_bodies, and the other blocks'
bodies on index-block ranks), k_bf64_reduce adds the planes in a fixed order.

Checked: the configuration a handle reports (nbody_get_config), exact pair coverage with probe worlds (tests/bf_probe.py
at PROBE64) over every size class and knob, full sums against the per-body bound of tests/bf64_bound.py and the f64
oracle, the fused kick, trajectories beside a strict handle, determinism, re-planning, the interaction counts, G = 2 and
3 real rank processes and the CLI.  Every test prints the worst error it saw (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bf64_bound import PROBE64, R, check_bound
from bf_probe import PROBE_G, check_probe, probe_columns, probe_records, set_probe

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
FIELDS = ("position", "velocity", "acceleration", "mass")
EPS = 2.0 ** -7             # a softening length f32 can hold exactly (bf_probe rounds eps to f32)
MIN_BODIES = 10240           # Tuning::bf64_min_bodies (kernels.h)
SMALL_IPT_BELOW = 16384      # kBf64SmallIptBelow (kernels_f64.h): 4 bodies per lane up to here, 8 beyond
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def report(what, worst):
    print(f"\n[bf64 fast] {what}: worst {worst:.3e}")


def positions(nb, n, seed):
    """n f32-representable Plummer positions (as f64), all well inside BOX."""
    pos = nb.plummer(2 * n + 64, seed=seed)["position"]
    pos = pos[np.abs(pos).max(1) < 30.0][:n]
    assert len(pos) == n
    return np.ascontiguousarray(pos, dtype=np.float64)


def world(nb, n, seed, jitter=True):
    ics = nb.plummer(n, seed=seed, f64=True)
    if jitter:
        ics["mass"] *= np.random.default_rng(seed).uniform(0.5, 1.5, n)
    return ics


def fast64(nb, points, eps, g=PROBE_G, capacity=None, math=None, **tuning):
    sim = nb.Simulation(points, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST if math is None else math, capacity=capacity,
                        f64=True, tuning=tuning)
    sim.settings = nb.Settings(g=g, g_soft=eps, dt=1e-3, theta2=0.5)
    return sim


def probe_update_forces(nb, sim, pos, cols, eps, what):
    rec = probe_records(nb.PARTICLE_DTYPE64, pos)
    worst = 0.0
    for k in cols:
        sim.upload(set_probe(rec, k))
        sim.update_forces()
        worst = max(worst, check_probe(sim.get_points()["acceleration"], pos, k, PROBE_G, eps, rtol=PROBE64, what=what))
    return worst


# ---------------------------------------------------------------------------------------------- the configuration
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("method", ["bf", "bh"])
def test_config_reports_the_effective_math_and_tree_build(gpu, f64, method):
    nb = gpu
    m = nb.BRUTE_FORCE if method == "bf" else nb.BARNES_HUT
    for math in (nb.STRICT, nb.FAST):
        with nb.Simulation(nb.plummer(100, f64=f64), *BOX, method=m, math_mode=math) as sim:
            c = sim.config
            assert c["math_mode"] == math
            assert c["tree_build"] == (nb.TREE_DEVICE if math == nb.FAST else nb.TREE_HOST)   # what AUTO resolved to
            assert c["dtype"] == (nb.F64 if f64 else nb.F32) and c["method"] == m
            assert c["struct_size"] == ctypes.sizeof(nb.NbodyConfig) and c["capacity"] == 100 and c["world_size"] == 1
        with nb.Simulation(nb.plummer(100, f64=f64), *BOX, method=m, math_mode=math, tree_build=nb.TREE_HOST) as sim:
            assert sim.config["tree_build"] == nb.TREE_HOST


# ---------------------------------------------------------------------------------------------- exact pair coverage
PROBE_SIZES = [  # (n, eps): the one-sided kernel alone below MIN_BODIES, k_bf64_sym with 4 bodies per lane (sets of 256) up
    # to SMALL_IPT_BELOW, with 8 (sets of 512) beyond
    (1, 0.0), (2, 0.0), (63, 0.0), (64, EPS), (65, 0.0),
    (MIN_BODIES - 1, 0.0), (MIN_BODIES, 0.0), (MIN_BODIES + 1, EPS),
    (12031, 0.0), (12033, EPS), (SMALL_IPT_BELOW, 0.0), (SMALL_IPT_BELOW + 1, 0.0), (20000, EPS), (65536, 0.0),
]


@pytest.mark.parametrize("n,eps", PROBE_SIZES)
def test_probe_every_pair_direction(gpu, n, eps):
    nb = gpu
    pos = positions(nb, n, seed=n)
    set_size = 256 if n <= SMALL_IPT_BELOW else 512
    cols = probe_columns(n, set_sizes=(set_size,) if n >= MIN_BODIES else (64,), n_random=16, every_below=70)
    with fast64(nb, probe_records(nb.PARTICLE_DTYPE64, pos), eps) as sim:
        worst = probe_update_forces(nb, sim, pos, cols, eps, f"n={n}")
    report(f"probe n={n} eps={eps} ({len(cols)} columns)", worst)


KNOBS = [  # (n, knobs): every value of the f64 knobs, and small worlds pushed onto k_bf64_sym (A = 1, 2, 3, 4 sets)
    (5000, dict(bf64_min_bodies=2, bf64_ipt=8)), (5000, dict(bf64_min_bodies=2, bf64_ipt=8, bf64_rot=1)), (20000, dict(bf64_ipt=4)),
    (20000, dict(bf64_rot=1)), (3001, dict(bf64_min_bodies=2, bf64_rot=1)), (3001, dict(bf64_min_bodies=2, bf64_waves=64)),
    (3001, dict(bf64_waves=64)), (3001, dict(bf64_waves=20000)), (20000, dict(bf64_min_bodies=100000)),
    (200, dict(bf64_min_bodies=2)), (300, dict(bf64_min_bodies=2)), (700, dict(bf64_min_bodies=2)),
    (1000, dict(bf64_min_bodies=2, bf64_rot=1)), (1500, dict(bf64_min_bodies=2, bf64_ipt=8)),
]


@pytest.mark.parametrize("n,knobs", KNOBS)
def test_probe_knobs(gpu, n, knobs):
    nb = gpu
    pos = positions(nb, n, seed=n + 1)
    cols = probe_columns(n, set_sizes=(256, 512), n_random=12, every_below=0)
    with fast64(nb, probe_records(nb.PARTICLE_DTYPE64, pos), 0.0, **knobs) as sim:
        worst = probe_update_forces(nb, sim, pos, cols, 0.0, f"n={n} {knobs}")
    report(f"probe n={n} {knobs}", worst)


# ---------------------------------------------------------------------------------------------- full sums
@pytest.mark.parametrize("n,eps", [(2, 0.0), (1000, 0.0), (2047, 1e-2), (4096, 1e-2), (8192, 0.0)])
def test_full_sums_every_row(gpu, orc, n, eps):
    nb = gpu
    ics = world(nb, n, seed=n + 5)
    with fast64(nb, ics, eps, g=1.25) as sim:
        sim.update_forces()
        got = sim.get_points()
    worst = check_bound(got["acceleration"], ics["position"], ics["mass"], 1.25, eps, what=f"n={n}")
    ref = ics.copy().astype(orc.P64)
    orc.bf_update_forces_rows(ref, dict(g=1.25, g_soft=eps, dt=1e-3, theta2=0.5), threads=8)
    l2 = np.linalg.norm(got["acceleration"] - ref["acceleration"]) / np.linalg.norm(ref["acceleration"])
    assert l2 <= 1e-13, l2
    report(f"full sums n={n}: |a - S| / T, L2 {l2:.2e}", worst)


@pytest.mark.parametrize("n", [65536, 262144])
def test_full_sums_sampled_rows(gpu, orc, n):
    nb = gpu
    eps = 1e-2
    ics = world(nb, n, seed=n)
    with fast64(nb, ics, eps, g=1.25) as sim:
        sim.update_forces()
        got = sim.get_points()
    rows = np.unique(np.concatenate([np.random.default_rng(n).choice(n, 96, replace=False), [0, 511, 512, n - 1]]))
    worst = check_bound(got["acceleration"], ics["position"], ics["mass"], 1.25, eps, rows=rows, what=f"n={n}")
    # relative L2 against the f64 oracle over the sampled rows (the oracle computes rows [0, m) of a reordered copy)
    order = np.concatenate([rows, np.setdiff1d(np.arange(n), rows)])
    ref = ics[order].copy().astype(orc.P64)
    orc.bf_update_forces_range(ref, dict(g=1.25, g_soft=eps, dt=1e-3, theta2=0.5), 0, len(rows), threads=8)
    a, b = got["acceleration"][rows], ref["acceleration"][: len(rows)]
    l2 = np.linalg.norm(a - b) / np.linalg.norm(b)
    assert l2 <= 1e-13, l2
    report(f"sampled rows n={n}: |a - S| / T, L2 {l2:.2e}", worst)


# ---------------------------------------------------------------------------------------------- stepping
def test_one_step_from_rest_through_the_fused_kick(gpu):
    """From rest, step_by(dt) = drift by 0, forces, then k_bf64_reduce<true>'s kick: v = 0 + a dt, x = x0 + (v 0.5) dt,
    bit for bit on the returned accelerations; the accelerations within the bound."""
    nb = gpu
    n, dt, eps = 6000, 1e-3, 1e-2
    pos = positions(nb, n, seed=11)
    ics = probe_records(nb.PARTICLE_DTYPE64, pos)
    ics["mass"] = np.random.default_rng(11).uniform(0.5, 1.5, n)
    with fast64(nb, ics, eps) as sim:
        sim.step_by(dt)
        got = sim.get_points()
    a = got["acceleration"]
    v = 0.0 + a * dt
    assert eq(got["velocity"], v)
    assert eq(got["position"], pos + (v * 0.5) * dt)
    report("fused kick", check_bound(a, pos, ics["mass"], PROBE_G, eps, rows=np.arange(0, n, 7), what="kick"))


def test_trajectory_beside_a_strict_handle(gpu):
    """Bodies leave a tight box, settings change between steps, dt goes negative, add_point / remove_point / clone: the
    fast handle keeps the strict handle's bodies, positions to 1e-12, and its final forces within the bound."""
    nb = gpu
    box = ((0.1, -0.05, 0.0), 1.7)
    ics = nb.plummer(3000, seed=52, f64=True)
    extra = np.zeros(1, nb.PARTICLE_DTYPE64)
    extra["position"], extra["velocity"], extra["mass"] = (0.2, 0.1, -0.3), (0.01, 0.0, 0.02), 0.5
    sims = [nb.Simulation(ics, *box, method=nb.BRUTE_FORCE, math_mode=m, capacity=3100) for m in (nb.FAST, nb.STRICT)]
    try:
        for s in sims:
            s.init()
        for k in range(9):
            sd = dict(g=1.0 + 0.1 * k, g_soft=0.05, dt=2e-2, theta2=0.5)
            for i, s in enumerate(sims):
                if k == 2:
                    s.add_point(extra)
                if k == 3:
                    s.remove_point(5)
                if k == 4:
                    twin = s.clone()
                    s.close()
                    sims[i] = s = twin
                s.settings = nb.Settings(**sd)
                s.step_by(-1e-2 if k == 5 else sd["dt"])
            f, st = (s.get_points() for s in sims)
            assert len(f) == len(st)
            assert np.abs(f["position"] - st["position"]).max() < 1e-12
        assert len(f) < 2900
        for s in sims:
            s.update_forces()
        f = sims[0].get_points()
        worst = check_bound(f["acceleration"], f["position"], f["mass"], sd["g"], sd["g_soft"], what="trajectory")
        assert sims[1].config["math_mode"] == nb.STRICT and sims[0].config["math_mode"] == nb.FAST
    finally:
        for s in sims:
            s.close()
    report("trajectory beside strict", worst)


def test_steps_equal_step_by_and_runs_repeat_bit_for_bit(gpu):
    nb = gpu
    ics = world(nb, 20000, seed=3)
    runs = []
    for how in ("steps", "step_by", "steps"):
        with fast64(nb, ics, 1e-2, g=1.0) as sim:
            sim.settings = nb.Settings(g=1.0, g_soft=1e-2, dt=1e-3, theta2=0.5)
            if how == "steps":
                sim.steps(4)
            else:
                for _ in range(4):
                    sim.step_by(1e-3)
            runs.append(sim.get_points())
    for f in FIELDS:
        assert eq(runs[0][f], runs[1][f]), f
        assert eq(runs[0][f], runs[2][f]), f


def test_replanning_one_handle_equals_a_fresh_handle(gpu):
    """One handle across body counts that change the plan (one-sided only, 4 and 8 bodies per lane) is bit-equal to a
    fresh handle of each count."""
    nb = gpu
    big = world(nb, 20000, seed=9)
    with fast64(nb, big, 1e-2, capacity=20000) as sim:
        for n in (20000, 5000, 1000, 17000, 3001):
            sim.upload(big[:n])
            sim.steps(2)
            got = sim.get_points()
            with fast64(nb, big[:n], 1e-2) as fresh:
                fresh.steps(2)
                ref = fresh.get_points()
            for f in FIELDS:
                assert eq(got[f], ref[f]), (n, f)


@pytest.mark.parametrize("n", [1000, 5000])
def test_interactions_count_directed_pairs(gpu, n):
    nb = gpu
    with fast64(nb, world(nb, n, seed=n), 1e-2) as sim:
        sim.set_profiling(1)
        sim.steps(3)
        sim.update_forces()
        s = sim.stats()
    assert s.interactions == 4 * n * (n - 1)
    assert s.force_launches == 4 and 0 < s.force_kernel_interactions <= 4 * n * (n - 1)


# ---------------------------------------------------------------------------------------------- index-block ranks
def _world_cfg(tmp_path, G, ics, settings, schedule, box, tuning=None):
    return {"world": G, "out": str(tmp_path / "world"), "transport": "ipc", "device": 0,
            "sim": dict(method="bf", math="fast", tuning=tuning or {}),
            "ics": ics, "box": box, "settings": settings, "schedule": schedule, "env": {}}


SYM = dict(bf64_min_bodies=2)   # every rank's own block through k_bf64_sym + the left-over pairs, whatever its size


@pytest.mark.parametrize("G,n,tuning", [(2, 6000, None), (3, 10000, None), (2, 6000, SYM), (3, 10000, SYM),
                                        (2, 24000, None)])   # (the last: 12 000 bodies per rank, symmetric by default)
def test_ranks_with_escapes_match_one_handle(gpu, tmp_path, G, n, tuning):
    nb = gpu
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], 3.0]
    sd = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    cfg = _world_cfg(tmp_path, G, dict(n=n, seed=12, mass_jitter=n, f64=True), sd, [["steps", 2], ["step_by", 2e-2], ["steps", 1], ["update_forces"]], box,
                     tuning)
    res = ranks.run_world(cfg, ranks_per_process=1, timeout=240)
    got = ranks.gather_world(res)
    pts = ranks.make_ics(nb, cfg["ics"])
    with ranks.make_sim(nb, dict(cfg, sim=dict(cfg["sim"], shard="index")), pts, 0, 1, 0) as sim:
        sim.settings = nb.Settings(**sd)
        sim.init()
        sim = ranks.run_schedule(nb, sim, cfg["schedule"])
        ref, s1 = sim.get_points(), sim.stats()
    assert got.dtype == nb.PARTICLE_DTYPE64 and len(got) == len(ref) < n
    assert np.abs(got["position"] - ref["position"]).max() < 1e-12
    assert sum(r["interactions"] for r in res) == s1.interactions
    worst = check_bound(got["acceleration"], got["position"], got["mass"], sd["g"], sd["g_soft"],
                        rows=np.arange(0, len(got), 3 if n <= 10000 else 11), what=f"G={G}")
    report(f"ranks G={G} n={n} {tuning or {}}", worst)


@pytest.mark.parametrize("G,n,tuning", [(2, 4097, None), (3, 3001, None), (2, 4097, SYM), (3, 3001, SYM)])
def test_ranks_probe_shard_boundaries(gpu, tmp_path, G, n, tuning):
    """Probe worlds through real ranks: the own block one-sided (below bf64_min_bodies) or symmetric (SYM: k_bf64_sym +
    the left-over pairs on every rank, my_seg > 0 included), the other blocks one-sided; every pair across a block
    boundary exactly once, in both directions.  SYM also probes each block's first resident-set boundary (sets of 256
    bodies counted from the block's start) and the first body of its last set."""
    nb = gpu
    from nbody_llm_amd import ranks
    blocks = [nb.shard_range(n, r, G) for r in range(G)]
    cols = {c for lo, hi in blocks for c in (lo, lo + 1, hi - 2, hi - 1)}
    if tuning:
        cols |= {c for lo, hi in blocks for c in (lo + 255, lo + 256, lo + (hi - lo - 1) // 256 * 256) if lo <= c < hi}
    cols = sorted(cols)
    worst = 0.0
    for k in cols:
        cfg = _world_cfg(tmp_path / f"k{k}", G, dict(n=n, seed=4, probe=k, f64=True), dict(g=PROBE_G, g_soft=0.0, dt=1e-3, theta2=0.5),
                         [["update_forces"]], [[0.0, 0.0, 0.0], 64.0], tuning)
        got = ranks.gather_world(ranks.run_world(cfg, ranks_per_process=1, timeout=120))
        pos = got["position"]
        assert len(got) == n and got["mass"][k] == 0.75
        worst = max(worst, check_probe(got["acceleration"], pos, k, PROBE_G, 0.0, rtol=PROBE64, what=f"G={G} k={k}"))
    report(f"ranks probe G={G} n={n} {tuning or {}} ({len(cols)} columns)", worst)


# ---------------------------------------------------------------------------------------------- CLI
def test_cli_f64_brute_force_fast_and_strict(gpu, tmp_path):
    nb = gpu
    cli = os.path.join(ROOT, "nbody-llm_amd", "nbody_cli")
    dumps = {}
    for math in ("fast", "strict"):
        f = str(tmp_path / f"{math}.bin")
        r = subprocess.run([cli, "-n", "3000", "--steps", "4", "--dtype", "f64", "--method", "bf", "--ic", "plummer", "--math", math, "--dump", f],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        dumps[math] = np.fromfile(f, nb.PARTICLE_DTYPE64)
    f, s = dumps["fast"], dumps["strict"]
    assert 2500 <= len(f) == len(s)
    assert np.abs(f["position"] - s["position"]).max() < 1e-12
    # the dumps' accelerations are those of the last force pass; the strict run's are the reference's sums, to f64 rounding
    from bf64_bound import direct_rows
    rows = np.arange(0, len(f), 5)
    S, T = direct_rows(s["position"], s["mass"], 1.0, 0.02, rows)
    err = np.linalg.norm(f["acceleration"][rows] - s["acceleration"][rows], axis=1) / np.asarray(T, np.float64)
    assert err.max() <= 2 * R, err.max()
    report("cli fast vs strict", float(err.max()))
