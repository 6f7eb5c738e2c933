"""k_bf_sym with the opposite-set pairs in the rotation (Tuning::sym_opp_rot, the default): for an even number A >= 4 of
resident sets, set a < A/2 meets the chunks of set a + A/2 symmetrically as the last visits of its chunk sequence, the
travelling-side sums of those visits go to one more plane of which only the rows of sets >= A/2 exist, the lower half's
sets are cut by a second table, and the left-over blocks evaluate the own set alone.  With A odd, A = 2 or below the
symmetric kernel's size nothing changes.

Probe worlds (tests/bf_probe.py: one massive body, per-body bound PROBE_RTOL) at sizes that put A on both sides of the
rule for both resident-set sizes, with the columns at both ends of every set boundary, of the opposite set's boundaries
and of the half-way set; the launch and reduction knobs with different cut tables for the two halves; sym_opp_rot 0
against 1; one step from rest; re-planning on one handle; a sharded world whose own-shard launch has even A; and the
pair count the statistics report.  Every test prints the worst per-body relative error it saw (pytest -s)."""
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


def fast_sim(nb, rec, eps, capacity=None, **tuning):
    sim = nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, capacity=capacity, tuning=tuning)
    sim.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5)
    return sim


def plan(nb, n, ipt=0):
    """(set size, A) of an n-body world: make_sym_plan's rule, the bodies per lane from the library."""
    set_size = 64 * (ipt or nb.launch_plan(n)["sym_bodies_per_lane"])
    return set_size, (n + set_size - 1) // set_size


def takes_opposite(A):
    return A % 2 == 0 and A >= 4


def columns(n, set_size, A, n_random=12):
    """Both ends of every set boundary and of the opposite set's boundaries, the first and last body of the first set at
    or past A/2, the last live body (of a ragged set: n - 1), and n_random random ones."""
    half = (A // 2) * set_size
    cols = set(probe_columns(n, set_sizes=(set_size,), offsets=(half,), n_random=n_random, every_below=0))
    cols.update(c for c in (half, min(n, half + set_size) - 1, n - 1) if 0 <= c < n)
    return sorted(cols)


def probe_update_forces(sim, pos, cols, eps, what):
    rec = probe_records(sim.dtype, pos)
    worst = 0.0
    for k in cols:
        sim.upload(set_probe(rec, k))
        sim.update_forces()
        worst = max(worst, check_probe(sim.get_points()["acceleration"], pos, k, PROBE_G, eps, what=what))
    return worst


def report(what, worst, n_probes):
    print(f"\n[opposite rotation] {what}: {n_probes} probes, worst per-body error {worst:.3e}")


SIZES = [  # (n, sym_ipt knob, expected A)
    (1024, 0, 4), (1281, 0, 6), (1537, 0, 7), (2048, 0, 8),          # sets of 256: even, even and ragged, odd, even
    (2048, 8, 4), (2049, 8, 5), (3073, 8, 7), (3585, 8, 8),          # sets of 512 by the knob
    (12345, 0, 25), (13312, 0, 26),                                  # sets of 512 by the rule
    (1024, 8, 2), (1025, 8, 3),                                      # no rotation pass (A = 2), no opposite set (A = 3)
]


@pytest.mark.parametrize("n,ipt,A", SIZES)
def test_sizes_on_both_sides_of_the_rule(gpu, n, ipt, A):
    nb = gpu
    set_size, got_A = plan(nb, n, ipt)
    assert got_A == A and set_size == (64 * ipt if ipt else 256 if n <= 10240 else 512)
    pos = positions(nb, n, seed=n + ipt + 3)
    cols = columns(n, set_size, A)
    kw = dict(sym_ipt=ipt) if ipt else {}
    worst = 0.0
    for eps in (0.0, 1e-2):
        with fast_sim(nb, probe_records(nb.PARTICLE_DTYPE, pos), eps, **kw) as sim:
            worst = max(worst, probe_update_forces(sim, pos, cols, eps, f"n={n} set={set_size} A={A} eps={eps}"))
    report(f"n={n} set={set_size} A={A} (opposite set in the rotation: {takes_opposite(A)})", worst, 2 * len(cols))


@pytest.mark.parametrize("n", [600, 700])
def test_below_the_symmetric_kernel(gpu, n):
    """Below sym_min_bodies the one-sided kernel runs whatever the symmetric kernel's knobs say."""
    nb = gpu
    pos = positions(nb, n, seed=n)
    cols = columns(n, 256, (n + 255) // 256, n_random=6)
    with fast_sim(nb, probe_records(nb.PARTICLE_DTYPE, pos), 0.0, sym_ipt=4) as sim:
        worst = probe_update_forces(sim, pos, cols, 0.0, f"n={n} sym_ipt=4")
    report(f"n={n} sym_ipt=4", worst, len(cols))


KNOBS = [  # (n, knobs, eps).  n = 13 312: A = 26, 96 chunk visits for the upper half's sets, 104 for the lower half's;
           # n = 17 000: A = 34 (ragged), 128 and 136 visits, so that sym_k = 126 is not clamped; n = 2 048: sets of 256, A = 8
    (13312, dict(sym_k=1), 0.0), (13312, dict(sym_k=5), 1e-2), (13312, dict(sym_k=8), 0.0), (17000, dict(sym_k=126), 1e-2),
    (13312, dict(sym_wpb=8), 1e-2), (13312, dict(sym_wpb=12), 0.0), (13312, dict(sym_wpb=16), 1e-2),
    (13312, dict(sym_wpb=12, sym_k=24), 0.0),
    (13312, dict(sym_packed=0), 0.0), (2048, dict(sym_packed=0), 1e-2),
    (13312, dict(sym_reduce_split=0), 1e-2), (2048, dict(sym_reduce_split=0), 0.0), (2048, dict(sym_k=3), 0.0),
]


@pytest.mark.parametrize("n,knobs,eps", KNOBS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kn.items())}" for n, kn, _ in KNOBS])
def test_knobs(gpu, n, knobs, eps):
    nb = gpu
    set_size, A = plan(nb, n, 8 if knobs.get("sym_packed") == 0 or knobs.get("sym_wpb", 4) != 4 else 0)  # (sym_bodies_per_lane: those force 8)
    assert takes_opposite(A)
    pos = positions(nb, n, seed=n + 7)
    cols = columns(n, set_size, A, n_random=8)
    with fast_sim(nb, probe_records(nb.PARTICLE_DTYPE, pos), eps, **knobs) as sim:
        worst = probe_update_forces(sim, pos, cols, eps, f"n={n} {knobs}")
    report(f"n={n} A={A} {knobs} eps={eps}", worst, len(cols))


@pytest.mark.parametrize("n,ipt", [(1281, 0), (3585, 8), (13312, 0)])
def test_against_the_one_sided_opposite_set(gpu, n, ipt):
    """The same upload with sym_opp_rot 0 and 1: the sums are grouped differently, so the results agree to 1e-6 of max|a|,
    not to the bit; each form is bit-reproducible on two fresh handles."""
    nb = gpu
    assert takes_opposite(plan(nb, n, ipt)[1])
    ics = nb.plummer(n, seed=n)
    kw = dict(sym_ipt=ipt) if ipt else {}
    acc = {}
    for opp in (0, 1):
        runs = []
        for _ in range(2):
            with fast_sim(nb, ics, 1e-2, sym_opp_rot=opp, **kw) as sim:
                sim.update_forces()
                runs.append(sim.get_points()["acceleration"].copy())
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), f"sym_opp_rot={opp} is not reproducible"
        acc[opp] = runs[0].astype(np.float64)
    diff = np.abs(acc[1] - acc[0]).max() / np.abs(acc[0]).max()
    print(f"\n[opposite rotation] n={n}: sym_opp_rot 1 against 0: {diff:.3e} of max|a|")
    assert diff <= 1e-6


@pytest.mark.parametrize("n,knobs", [(1281, {}), (13312, {}), (2048, dict(sym_ipt=8))])
def test_one_step_from_rest(gpu, n, knobs):
    """One step from rest: the drift moves nothing, the forces are the probe's, the kick fused into the plane reduction
    gives v = a dt."""
    nb = gpu
    eps, dt = 1e-2, 1e-3
    set_size, A = plan(nb, n, knobs.get("sym_ipt", 0))
    assert takes_opposite(A)
    pos = positions(nb, n, seed=n + 11)
    cols = columns(n, set_size, A, n_random=6)
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    worst = 0.0
    with fast_sim(nb, rec, eps, **knobs) as sim:
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


def test_replanning_across_even_and_odd(gpu):
    """One handle takes worlds with A = 26, 25, 8, 7 and 26 sets in turn: the plan, both cut tables, the extra plane and
    the pair count change under it.  Every probe passes and equals, bit for bit, a handle made for that size."""
    nb = gpu
    eps = 1e-2
    worst, total = 0.0, 0
    with fast_sim(nb, probe_records(nb.PARTICLE_DTYPE, positions(nb, 1, seed=1)), eps, capacity=13312) as sim:
        for n in (13312, 12345, 2048, 1537, 13312):
            set_size, A = plan(nb, n)
            pos = positions(nb, n, seed=n + 5)
            rec = probe_records(nb.PARTICLE_DTYPE, pos)
            cols = columns(n, set_size, A, n_random=4)[::3]
            with fast_sim(nb, rec, eps) as fresh:
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


@pytest.mark.parametrize("cross", [1, 0])
def test_sharded_world_with_even_own_shard(gpu, cross):
    """G = 2, n = 6001: shards of 3001 and 3000 bodies, 12 sets of 256 each: the own-shard k_bf_sym launch takes the
    opposite set in the rotation, its planes sit in front of the cross-shard ones."""
    nb = gpu
    G, n, eps = 2, 6001, 0.0
    blocks = [nb.shard_range(n, r, G) for r in range(G)]
    for lo, hi in blocks:
        assert plan(nb, hi - lo) == (256, 12)
    pos = positions(nb, n, seed=G * 1000 + n + cross)
    cols = probe_columns(n, blocks=blocks, set_sizes=(256,), offsets=(6 * 256,), n_random=12, every_below=0)
    rec = probe_records(nb.PARTICLE_DTYPE, pos)
    sims = [nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, rank=r, world_size=G, capacity=n,
                          tuning=dict(cross_sym=cross)) for r in range(G)]
    worst = 0.0
    try:
        for s in sims:
            s.settings = nb.Settings(g=PROBE_G, g_soft=eps, dt=1e-3, theta2=0.5)
            s.init()
        for k in cols:
            set_probe(rec, k)
            for s in sims:
                s.upload(rec)
            nb.sharded_step(sims)
            got = np.concatenate([s.get_points() for s in sims])
            worst = max(worst, check_probe(got["acceleration"], pos, k, PROBE_G, eps, what=f"G={G} n={n} cross_sym={cross}"))
    finally:
        for s in sims:
            s.close()
    report(f"sharded G={G} n={n} cross_sym={cross}", worst, len(cols))


def rotation_pairs(n, set_size, A, opp_rot=1):
    """Unordered pairs of live bodies the rotation evaluates: every set with the next ceil(A/2) - 1 sets, and each set
    of the lower half with its opposite set when A is even and there is a rotation pass."""
    size = [max(0, min(set_size, n - a * set_size)) for a in range(A)]
    sym_sets = (A + 1) // 2 - 1
    pairs = sum(size[a] * size[(a + d) % A] for a in range(A) for d in range(1, sym_sets + 1))
    if opp_rot and A % 2 == 0 and sym_sets >= 1:
        pairs += sum(size[a] * size[a + A // 2] for a in range(A // 2))
    return pairs


@pytest.mark.parametrize("n,ipt,opp_rot", [(1281, 0, 1), (1281, 0, 0), (1537, 0, 1), (3585, 8, 1), (12345, 0, 1), (13312, 0, 1)])
def test_statistics_count_the_new_pairs(gpu, n, ipt, opp_rot):
    nb = gpu
    set_size, A = plan(nb, n, ipt)
    kw = dict(sym_ipt=ipt) if ipt else {}
    with fast_sim(nb, nb.plummer(n, seed=n), 1e-2, sym_opp_rot=opp_rot, **kw) as sim:
        sim.set_profiling(True)
        sim.reset_stats()
        sim.update_forces()
        s = sim.stats()
    assert s.force_launches == 1
    assert s.force_kernel_interactions == 2 * rotation_pairs(n, set_size, A, opp_rot)
    if opp_rot and takes_opposite(A):   # what is left to the one-sided blocks is the own sets alone
        own = sum(m * (m - 1) for m in (max(0, min(set_size, n - a * set_size)) for a in range(A)))
        assert s.force_kernel_interactions + own == n * (n - 1)
