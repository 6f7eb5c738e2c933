"""Exact pair coverage of the fast brute-force kernels: probe worlds (tests/bf_probe.py) in which only body k has mass.

Every body then receives exactly one term, so a pair that a kernel drops, counts twice, applies with the wrong sign
or the wrong mass, or takes from a stale partial-sum plane is an O(1) error against a per-body bound of PROBE_RTOL
(a few f32 roundings and one v_rsq_f32).  The full-sum tests cannot see such an error above ~10 000 bodies, where
one pair is below their per-body tolerance.  Covered: the one-sided kernel k_bf_fast (default and the 1/2/4 bodies-
per-lane variants), the symmetric k_bf_sym with 4 and 8 bodies per lane and its launch and reduction knobs, the kick
fused into the plane reduction, sharded worlds (k_bf_fast over segments, k_bf_cross + k_bf_cross_reduce, k_bf_os),
shards left with 0, 1, 65 or a few hundred live bodies, and re-planning on one handle.  Every test prints the worst
per-body relative error it saw (pytest -s)."""
import numpy as np
import pytest

from bf_probe import PROBE_G, PROBE_RTOL, check_probe, probe_columns, probe_records, set_probe

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)


def positions(nb, n, seed):
    """n Plummer positions, all well inside BOX (a step's retain must keep them)."""
    pos = nb.plummer(2 * n + 64, seed=seed)["position"]
    pos = pos[np.abs(pos).max(1) < 30.0][:n]
    assert len(pos) == n
    return np.ascontiguousarray(pos)


def fast_sim(nb, pos, eps, capacity=None, **tuning):
    sim = nb.Simulation(probe_records(nb.PARTICLE_DTYPE, pos), *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST,
                        capacity=capacity, tuning=tuning)
    sim.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5)
    return sim


def report(what, worst, n_probes):
    print(f"\n[pair coverage] {what}: {n_probes} probes, worst per-body error {worst:.3e}")


def probe_update_forces(sim, pos, cols, eps, what):
    rec = probe_records(sim.dtype, pos)
    worst = 0.0
    for k in cols:
        sim.upload(set_probe(rec, k))
        sim.update_forces()
        worst = max(worst, check_probe(sim.get_points()["acceleration"], pos, k, PROBE_G, eps, what=what))
    return worst


# ---------------------------------------------------------------------------------------------- one shard
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 1023])
def test_one_sided_default_kernel_every_column(gpu, n):
    """Below sym_min_bodies (1024) update_forces runs k_bf_fast<1, 8, 2048>: every column at eps = 0, the rule's
    columns at eps = 1e-2."""
    nb = gpu
    pos = positions(nb, n, seed=n)
    worst = 0.0
    for eps, every in ((0.0, 1100), (1e-2, 0)):
        with fast_sim(nb, pos, eps) as sim:
            worst = max(worst, probe_update_forces(sim, pos, probe_columns(n, set_sizes=(64,), every_below=every), eps,
                                                   f"k_bf_fast n={n}"))
    report(f"k_bf_fast n={n}", worst, n)


@pytest.mark.parametrize("variant", [1, 2, 4])
def test_one_sided_variants(gpu, variant):
    """bf_fast_variant 1, 2, 4: the LDS-tiled kernel with 1, 2, 4 bodies per lane at a ragged size (partial
    64*IPT-body blocks and a partial 2048-body partner tile)."""
    nb = gpu
    n = 3001
    pos = positions(nb, n, seed=3)
    cols = probe_columns(n, set_sizes=(64 * variant, 2048), n_random=16, every_below=0)
    with fast_sim(nb, pos, 0.0, bf_fast_variant=variant) as sim:
        worst = probe_update_forces(sim, pos, cols, 0.0, f"bf_fast_variant={variant}")
    report(f"bf_fast_variant={variant} n={n}", worst, len(cols))


SYM_SIZES = [  # (n, sym_ipt knob, eps): resident sets of 64 * IPT bodies, A = ceil(n / set)
    (1024, 0, 0.0), (1025, 0, 1e-2), (1281, 0, 0.0), (4097, 0, 1e-2), (4097, 0, 0.0), (10240, 0, 0.0),   # IPT 4
    (10241, 0, 1e-2), (12345, 0, 0.0), (33000, 0, 1e-2),                                             # IPT 8
    (1024, 8, 0.0), (1025, 8, 1e-2), (1537, 8, 0.0),                                                  # A = 2, 3, 4
]


@pytest.mark.parametrize("n,ipt,eps", SYM_SIZES)
def test_symmetric_kernel_sizes(gpu, n, ipt, eps):
    nb = gpu
    pos = positions(nb, n, seed=n + ipt)
    set_size = 64 * (ipt or nb.launch_plan(n)["sym_bodies_per_lane"])
    assert set_size == (256 if ipt == 0 and n <= 10240 else 512)
    cols = probe_columns(n, set_sizes=(set_size,), n_random=24)
    kw = dict(sym_ipt=ipt) if ipt else {}
    with fast_sim(nb, pos, eps, **kw) as sim:
        worst = probe_update_forces(sim, pos, cols, eps, f"k_bf_sym n={n} set={set_size}")
    report(f"k_bf_sym n={n} set={set_size} eps={eps}", worst, len(cols))


SYM_KNOBS = [  # (n, knobs, eps); the plan's K is clamped to [1, min(126, L)], L = IPT * (ceil(A/2) - 1)
    (4097, dict(sym_packed=0), 0.0),                     # scalar pairs (and 8 bodies per lane)
    (12345, dict(sym_packed=0), 1e-2),
    (12345, dict(sym_wpb=8), 0.0), (12345, dict(sym_wpb=12), 1e-2), (12345, dict(sym_wpb=16), 0.0),
    (4097, dict(sym_reduce_split=0), 1e-2), (12345, dict(sym_reduce_split=0), 0.0),
    (12345, dict(sym_k=8), 1e-2),                        # K % wpb == 0: resident sums combined in LDS (res_combine 1)
    (12345, dict(sym_k=5), 0.0),                         # res_combine 0
    (12345, dict(sym_k=1), 1e-2),                        # one wave per set
    (12345, dict(sym_wpb=12, sym_k=24), 0.0),            # combined, 12-wave workgroups
    (12345, dict(sym_wpb=8, sym_k=7), 1e-2),             # not combined, 8-wave workgroups
    (33000, dict(sym_k=126), 0.0),                       # the most slices the bounds array holds
    (4097, dict(sym_k=1000), 1e-2),                      # clamped to L
]


@pytest.mark.parametrize("n,knobs,eps", SYM_KNOBS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kn.items())}" for n, kn, _ in SYM_KNOBS])
def test_symmetric_kernel_knobs(gpu, n, knobs, eps):
    nb = gpu
    pos = positions(nb, n, seed=n + 7)
    cols = probe_columns(n, set_sizes=(256, 512) if n <= 10240 else (512,), n_random=12)
    with fast_sim(nb, pos, eps, **knobs) as sim:
        worst = probe_update_forces(sim, pos, cols, eps, f"k_bf_sym n={n} {knobs}")
    report(f"k_bf_sym n={n} {knobs} eps={eps}", worst, len(cols))


@pytest.mark.parametrize("n,knobs", [(700, {}), (1025, {}), (4097, {}), (12345, {}), (12345, dict(sym_reduce_split=0)),
                                     (1024, dict(sym_ipt=8))])
def test_one_step_from_rest(gpu, n, knobs):
    """One step from rest: the drift moves nothing, the forces are the probe's, and the kick (its own kernel below
    1024 bodies, fused into k_bf_sym_reduce*<KICK> above; A = 2 leaves the rotation kernel out) gives v = a dt."""
    nb = gpu
    eps, dt = 1e-2, 1e-3
    pos = positions(nb, n, seed=n + 11)
    cols = probe_columns(n, set_sizes=(256, 512), n_random=8, every_below=64)
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    worst = 0.0
    with fast_sim(nb, pos, eps, **knobs) as sim:
        sim.init()
        for k in cols:
            sim.upload(set_probe(rec, k))
            sim.step()
            got = sim.get_points()
            worst = max(worst, check_probe(got["acceleration"], pos, k, PROBE_G, eps, what=f"step n={n} {knobs}"))
            # v = fl(a dt): one rounding more than the acceleration
            check_probe(got["velocity"].astype(np.float64) / np.float32(dt), pos, k, PROBE_G, eps,
                        rtol=PROBE_RTOL + 2.0 ** -23, what=f"step velocity n={n} {knobs}")
    report(f"one step n={n} {knobs}", worst, len(cols))


def test_replanning_on_one_handle(gpu):
    """One handle of capacity 33 000 takes worlds of 33 000, 9 000, 10 241, 1 025, 300 and 12 345 bodies in turn:
    its symmetric plan, pair count, cut points and planes change under it (and at 300 bodies the one-sided kernel
    runs).  Every probe must pass and equal, bit for bit, the same upload on a handle made for that size."""
    nb = gpu
    eps = 1e-2
    worst, total = 0.0, 0
    with fast_sim(nb, positions(nb, 1, seed=1), eps, capacity=33000) as sim:
        for n in (33000, 9000, 10241, 1025, 300, 12345):
            pos = positions(nb, n, seed=n + 5)
            rec = probe_records(nb.PARTICLE_DTYPE, pos)
            cols = probe_columns(n, set_sizes=(256, 512), n_random=6, every_below=0)
            with fast_sim(nb, pos, eps) as fresh:
                for k in cols:
                    set_probe(rec, k)
                    sim.upload(rec)
                    sim.update_forces()
                    got = sim.get_points()
                    worst = max(worst, check_probe(got["acceleration"], pos, k, PROBE_G, eps, what=f"re-planned n={n}"))
                    fresh.upload(rec)
                    fresh.update_forces()
                    assert np.array_equal(got["acceleration"].view(np.uint32),
                                          fresh.get_points()["acceleration"].view(np.uint32)), (n, k)
            total += len(cols)
    report("re-planning", worst, total)


# ---------------------------------------------------------------------------------------------- sharded worlds
def make_world(nb, pos, G, eps, capacity=None, **tuning):
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    sims = [nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=r, world_size=G,
                          capacity=capacity or len(pos), tuning=tuning) for r in range(G)]
    for s in sims:
        s.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5)
        s.init()
    return sims


def gather(sims):
    return np.concatenate([s.get_points() for s in sims])


def cross_split(seg_cap):
    """First body (relative to a shard) that the higher of two opposite ranks keeps resident (make_cross_plan)."""
    chunks_cap = (seg_cap + 63) // 64
    return ((chunks_cap + 7) // 8 + 1) // 2 * 8 * 64


def sharded_columns(nb, n, G, n_random=24, set_sizes=(256, 512)):
    seg_cap = (n + G - 1) // G
    blocks = [nb.shard_range(n, r, G) for r in range(G)]
    return probe_columns(n, blocks=blocks, set_sizes=set_sizes, offsets=(cross_split(seg_cap),), n_random=n_random,
                         every_below=0)


def probe_world(nb, sims, pos, cols, eps, what):
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    worst = 0.0
    for k in cols:
        set_probe(rec, k)
        for s in sims:
            s.upload(rec)
        nb.sharded_step(sims)
        worst = max(worst, check_probe(gather(sims)["acceleration"], pos, k, PROBE_G, eps, what=what))
    return worst


SHARDED = [  # (G, n, cross_sym, eps): seg_cap = ceil(n / G); below 2048 k_bf_fast runs over the segments
    (2, 3001, 1, 0.0), (3, 5000, 1, 1e-2), (5, 9001, 1, 0.0), (8, 15205, 1, 1e-2),
    (2, 6001, 1, 0.0), (2, 6001, 0, 1e-2), (3, 10000, 1, 1e-2), (3, 10000, 0, 0.0),
    (5, 12001, 1, 0.0), (5, 12001, 0, 1e-2), (8, 20000, 1, 1e-2), (8, 20000, 0, 0.0),
    (2, 4095, 1, 0.0), (8, 16385, 1, 1e-2),       # ragged last block on the other side of 2048
]


@pytest.mark.parametrize("G,n,cross,eps", SHARDED)
def test_sharded_world(gpu, G, n, cross, eps):
    nb = gpu
    pos = positions(nb, n, seed=G * 1000 + n)
    cols = sharded_columns(nb, n, G)
    sims = make_world(nb, pos, G, eps, cross_sym=cross)
    try:
        worst = probe_world(nb, sims, pos, cols, eps, f"G={G} n={n} cross_sym={cross}")
    finally:
        for s in sims:
            s.close()
    report(f"sharded G={G} n={n} seg_cap={(n + G - 1) // G} cross_sym={cross} eps={eps}", worst, len(cols))


CROSS_KNOBS = [  # k_bf_cross launch knobs the planner accepts as written (kernels.h Tuning)
    (8, 20000, dict(cross_ipt=4)), (8, 20000, dict(cross_ipt=8)), (5, 12001, dict(cross_ipt=8)),
    (8, 20000, dict(cross_wpb=8)), (8, 20000, dict(cross_wpb=12)), (3, 10000, dict(cross_wpb=12, cross_ipt=4)),
    (8, 20000, dict(cross_slots=256)), (5, 12001, dict(cross_slots=256, sym_packed=0)),
]


@pytest.mark.parametrize("G,n,knobs", CROSS_KNOBS, ids=[f"G{G}-{n}-{'-'.join(f'{k}{v}' for k, v in kn.items())}" for G, n, kn in CROSS_KNOBS])
def test_sharded_cross_knobs(gpu, G, n, knobs):
    nb = gpu
    eps = 1e-2
    pos = positions(nb, n, seed=G * 1000 + n + 1)
    ipt = knobs.get("cross_ipt")
    cols = sharded_columns(nb, n, G, n_random=8, set_sizes=(64 * ipt,) if ipt else (256, 512))
    sims = make_world(nb, pos, G, eps, **knobs)
    try:
        worst = probe_world(nb, sims, pos, cols, eps, f"G={G} n={n} {knobs}")
    finally:
        for s in sims:
            s.close()
    report(f"sharded G={G} n={n} {knobs}", worst, len(cols))


@pytest.mark.parametrize("live,cross", [((2100, 0, 65, 300), 1), ((2100, 0, 65, 300), 0), ((1, 2100, 0, 513), 1)])
def test_sharded_shards_left_almost_empty(gpu, live, cross):
    """Shards of capacity 2100 (>= 2048: the symmetric schemes) where the bodies uploaded outside the box leave some
    shards with 0, 1, 65, 300 or 513 live bodies.  A first step with dt = 0 drops them (retain) and moves nothing;
    get_points() then brings every rank's host count down to its live count, so the second step's own-shard plans
    have A = 1, 2 or 3 resident sets of 256 bodies (no rotation pass below A = 3).  Both steps are probed."""
    nb = gpu
    eps, G, cap = 1e-2, 4, 2100
    n = G * cap
    inside = positions(nb, n, seed=sum(live))
    pos = inside.copy()
    for r, m in enumerate(live):   # outside the box: beyond x = 32, massless anyway
        pos[r * cap + m:(r + 1) * cap, 0] = 40.0 + np.abs(inside[r * cap + m:(r + 1) * cap, 0])
    alive = np.concatenate([np.arange(r * cap, r * cap + m) for r, m in enumerate(live)])
    live_pos = pos[alive]
    blocks, at = [], 0
    for m in live:
        blocks.append((at, at + m))
        at += m
    cols = probe_columns(len(alive), blocks=blocks, set_sizes=(256,), n_random=12, every_below=0)
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    sims = make_world(nb, pos, G, eps, cross_sym=cross)
    worst = 0.0
    try:
        for k in cols:
            set_probe(rec, int(alive[k]))
            for s in sims:
                s.upload(rec)
            nb.sharded_step(sims, dt=0.0)
            got = gather(sims)
            assert [len(s) for s in sims] == list(live)
            worst = max(worst, check_probe(got["acceleration"], live_pos, k, PROBE_G, eps, what=f"{live} first step"))
            assert not got["velocity"].any()
            nb.sharded_step(sims)
            worst = max(worst, check_probe(gather(sims)["acceleration"], live_pos, k, PROBE_G, eps, what=f"{live} second step"))
    finally:
        for s in sims:
            s.close()
    report(f"sharded live={live} cross_sym={cross}", worst, 2 * len(cols))
