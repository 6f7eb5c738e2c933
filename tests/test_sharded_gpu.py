"""The multi-GPU path on ONE GPU: G handles of this process play ranks 0..G-1 of a world of G
(same device); the per-step exchange that nbody_step_by does with an RCCL all-gather is done here
with device-to-device copies (nbody_debug_* hooks).  Everything else is the production code:
index-block shards, per-segment counts, the force kernels over segments, per-shard retain.
Oracle of the sharded run = the 1-shard run (and the CPU oracle): strict math bit-exact."""
import numpy as np
import pytest

from bf_probe import PROBE_G, check_probe, probe_columns, probe_records, set_probe
from conftest import Knob, rel_err

pytestmark = pytest.mark.gpu
BOX = ((0.0, 0.0, 0.0), 64.0)
FIELDS = ("position", "velocity", "acceleration", "mass")


def make_world(nb, ics, G, box, st, method, math_mode, **kw):
    sims = [nb.Simulation(ics, *box, method=method, math_mode=math_mode, rank=r, world_size=G, capacity=len(ics), **kw)
            for r in range(G)]
    for s in sims:
        s.settings = st
        s.init()
    return sims


def gather(sims):
    return np.concatenate([s.get_points() for s in sims])


@pytest.mark.parametrize("G", [2, 3, 8])
def test_brute_force_strict_shards_match_single_and_oracle(gpu, orc, G):
    nb = gpu
    sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    st = nb.Settings(**sd)
    ics = nb.plummer(1000, seed=G)         # 1000 is not a multiple of 3 or 8: ragged last block
    sims = make_world(nb, ics, G, BOX, st, nb.BRUTE_FORCE, nb.STRICT)
    assert [s.local_range() for s in sims] == [(lo, hi - lo) for lo, hi in (nb.shard_range(1000, r, G) for r in range(G))]
    for _ in range(5):
        nb.sharded_step(sims)
    got = gather(sims)
    ref = ics.copy().astype(orc.P32)
    for _ in range(5):
        ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], sd["dt"])
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    for s in sims:
        s.close()


def test_brute_force_shards_with_escapes(gpu, orc):
    """Bodies leave a tight box on different shards at different steps: every shard compacts its
    own block, the counts travel with the exchange, global order is preserved."""
    nb = gpu
    box = ((0.0, 0.0, 0.0), 1.5)
    sd = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    ics = nb.plummer(1500, seed=11)
    sims = make_world(nb, ics, 4, box, nb.Settings(**sd), nb.BRUTE_FORCE, nb.STRICT)
    ref = ics.copy().astype(orc.P32)
    for _ in range(10):
        nb.sharded_step(sims)
        ref = orc.bf_step_by(ref, sd, box[0], box[1], sd["dt"])
    got = gather(sims)
    assert len(ref) < 1400 and len(got) == len(ref)
    assert sum(len(s) for s in sims) == sims[0].count_global() == len(ref)
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    for s in sims:
        s.close()


@pytest.mark.parametrize("cross", [1, 0])
@pytest.mark.parametrize("G,n", [(2, 6000), (2, 20000), (3, 10000), (4, 9001), (5, 12000), (8, 20000), (8, 65536),
                                 (2, 4095), (8, 16385)])  # ragged last block on the other side of 2048 bodies
def test_brute_force_fast_shards(gpu, orc, G, n, cross):
    """fast math, sharded (n/G >= 2048; below that the LDS-tiled kernel): the own shard by the
    symmetric kernel; the other shards either symmetric too (cross = 1, the default: every pair
    between shards evaluated once, by one of the two GPUs, partial sums returned to the owner) or
    one-sided (cross = 0, k_bf_os).  1e-5 against the f32 oracle either way."""
    nb = gpu
    Knob(nb, "cross_sym", 1).value = cross
    sd = dict(g=1.0, g_soft=1e-2, dt=1e-3, theta2=0.5)
    ics = nb.plummer(n, seed=5)
    ics["mass"] *= np.random.default_rng(n).uniform(0.5, 1.5, n).astype(np.float32)
    sims = make_world(nb, ics, G, BOX, nb.Settings(**sd), nb.BRUTE_FORCE, nb.FAST)
    steps = 2 if n <= 20000 else 1
    for _ in range(steps):
        nb.sharded_step(sims)
    got = gather(sims)
    ref = ics.copy().astype(orc.P32)
    for k in range(steps):
        if n <= 20000:
            ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], sd["dt"])
        else:  # the serial reference loop is too slow here: same step with the threaded row-wise form
            orc.pre_force(ref, sd["dt"])
            orc.bf_update_forces_rows(ref, sd, threads=16)
            orc.after_force(ref, sd["dt"])
    assert np.isfinite(got["acceleration"]).all()
    assert rel_err(got["acceleration"], ref["acceleration"]) < (1e-5 if n <= 20000 else 3e-5)
    assert rel_err(got["position"], ref["position"]) < 1e-6
    if n // G >= 2048:   # the intended path ran: the timed launch covers the pairs with other shards
        st = [s_.stats() for s_ in sims]
        assert all(s_.steps == steps for s_ in st)
    for s in sims:
        s.close()
    Knob(nb, "cross_sym", 1).value = 1


def test_cross_shard_pairs_are_dealt_exactly_once(gpu):
    """Host-side plan of the symmetric scheme across shards: over all ranks, every (own set, partner
    chunk) block between two different shards is claimed by exactly one of the two GPUs."""
    nb = gpu
    for G in (2, 3, 4, 5, 8):
        n = 4096 * G + 777
        ics = nb.plummer(n, seed=G)
        sims = make_world(nb, ics, G, BOX, nb.Settings(), nb.BRUTE_FORCE, nb.FAST)
        nb.sharded_step(sims)      # builds the plans; momentum conservation checks the pairing as a whole
        got = gather(sims)
        m = got["mass"].astype(np.float64)[:, None]
        p = (got["acceleration"].astype(np.float64) * m).sum(0)
        assert np.abs(p).max() < 2e-6 * np.abs(got["acceleration"].astype(np.float64) * m).sum(), G
        for s in sims:
            s.close()


def test_cross_shard_pairs_are_dealt_exactly_once_probed(gpu):
    """Worlds of the same sizes as above, pair by pair: momentum conservation cannot see a block of pairs dropped or dealt to
    both GPUs (each is applied to both bodies).  In a probe world only body k has mass, so every body receives exactly
    the one term of its pair with k (tests/bf_probe.py); k runs over the ends of every shard block, the first body the
    higher of two opposite ranks keeps resident, the resident-set boundaries of 512 bodies and a few seeded bodies."""
    nb = gpu
    eps = 1e-2
    for G in (2, 3, 4, 5, 8):
        n = 4096 * G + 777
        pos = nb.plummer(n + 256, seed=G)["position"]
        pos = np.ascontiguousarray(pos[np.abs(pos).max(1) < 30.0][:n])   # (all inside the box: none leaves)
        assert len(pos) == n
        rec = probe_records(nb.PARTICLE_DTYPE, pos)
        sims = make_world(nb, rec, G, BOX, nb.Settings(g=PROBE_G, g_soft=eps), nb.BRUTE_FORCE, nb.FAST)
        chunks_cap = ((n + G - 1) // G + 63) // 64
        split = ((chunks_cap + 7) // 8 + 1) // 2 * 8 * 64    # make_cross_plan's opposite-rank cut, in bodies
        cols = probe_columns(n, blocks=[nb.shard_range(n, r, G) for r in range(G)], set_sizes=(512,), offsets=(split,),
                             n_random=4, every_below=0)
        for k in cols:
            for s in sims:
                s.upload(set_probe(rec, k))
            nb.sharded_step(sims)
            check_probe(gather(sims)["acceleration"], pos, k, PROBE_G, eps, what=f"G={G}")
        for s in sims:
            s.close()


def test_brute_force_fast_shards_with_escapes(gpu, orc):
    nb = gpu
    box = ((0.0, 0.0, 0.0), 3.0)
    sd = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    ics = nb.plummer(12000, seed=12)
    sims = make_world(nb, ics, 3, box, nb.Settings(**sd), nb.BRUTE_FORCE, nb.FAST)
    ref = ics.copy().astype(orc.P32)
    for _ in range(8):
        nb.sharded_step(sims)
        ref = orc.bf_step_by(ref, sd, box[0], box[1], sd["dt"])
    got = gather(sims)
    assert len(ref) < 11500 and len(got) == len(ref)
    assert np.array_equal(got["mass"], ref["mass"])
    assert rel_err(got["position"], ref["position"]) < 1e-5
    for s in sims:
        s.close()


def test_fast_shards_straddling_the_symmetric_threshold_after_escapes(gpu, orc):
    """Shards of 2150 bodies in a tight box: bodies leave, one shard's live count falls below the 2048
    bodies at which the symmetric scheme starts while its peer is still above, and get_points() between
    steps refreshes every rank's host view of its own count independently.  The scheme is chosen from the
    shard capacity (shared by all ranks), so the partial-sum exchange keeps matching."""
    nb = gpu
    box = ((0.0, 0.0, 0.0), 2.2)
    sd = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    ics = nb.plummer(4300, seed=14)
    sims = make_world(nb, ics, 2, box, nb.Settings(**sd), nb.BRUTE_FORCE, nb.FAST)
    ref = ics.copy().astype(orc.P32)
    lens = []
    for k in range(10):
        nb.sharded_step(sims)
        ref = orc.bf_step_by(ref, sd, box[0], box[1], sd["dt"])
        if k % 3 == 0:
            lens.append([len(s.get_points()) for s in sims])   # one rank at a time, as a visualiser would
    got = gather(sims)
    assert min(min(l) for l in lens) < 2048, lens
    assert len(got) == len(ref)
    assert np.array_equal(got["mass"], ref["mass"])
    assert rel_err(got["position"], ref["position"]) < 1e-5
    for s in sims:
        s.close()


@pytest.mark.parametrize("G", [2, 4])
def test_barnes_hut_shards_match_single(gpu, orc, G):
    """E2 option A: every shard builds the same global tree from the gathered positions and walks
    it for its own bodies; counts add up to the 1-shard counts, state equals the oracle's."""
    nb = gpu
    sd = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
    ics = nb.plummer(3000, seed=21)
    sims = make_world(nb, ics, G, BOX, nb.Settings(**sd), nb.BARNES_HUT, nb.STRICT)
    ref = ics.copy().astype(orc.P32)
    tot_a = tot_v = 0
    for _ in range(4):
        nb.sharded_step(sims)
        ref, a, v = orc.bh_step_by(ref, sd, BOX[0], BOX[1], sd["dt"], threads=4)
        tot_a += a
        tot_v += v
    got = gather(sims)
    stats = [s.stats() for s in sims]
    assert sum(s.interactions for s in stats) == tot_a and sum(s.node_visits for s in stats) == tot_v
    assert np.abs(got["position"].astype(np.float64) - ref["position"]).max() < 1e-6
    assert rel_err(got["acceleration"], ref["acceleration"]) < 1e-5
    for s in sims:
        s.close()


@pytest.mark.parametrize("G,n,box_w", [(2, 3000, 64.0), (4, 20000, 64.0), (3, 9000, 2.5)])
def test_barnes_hut_shards_with_device_tree_equal_single_shard(gpu, G, n, box_w):
    """Device-side build in a sharded world: every GPU concatenates the gathered segments, builds the
    same tree and walks it for its own bodies.  Same tree + same per-body walk => the state equals the
    1-shard device-tree run bit for bit and the node counts add up exactly (bodies leave the 2.5-wide
    box on the way: per-segment counts, concatenation offsets and own-order lists all move).  The walk's
    node-range split is pinned to 8 segments: its default follows the number of own bodies, and the
    order in which the segments' partial sums are added would differ between the two runs."""
    nb = gpu
    split = Knob(nb, "bh_walk_split", 0)
    split.value = 8
    box = ((0.0, 0.0, 0.0), box_w)
    st = nb.Settings(1.0, 0.01, 5e-3, 0.25)
    ics = nb.plummer(n, seed=31)
    sims = make_world(nb, ics, G, box, st, nb.BARNES_HUT, nb.FAST, tree_build=nb.TREE_DEVICE)
    with nb.Simulation(ics, *box, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as one:
        one.settings = st
        one.init()
        for _ in range(5):
            nb.sharded_step(sims)
            one.step()
        ref = one.get_points()
        s1 = one.stats()
    split.value = 0
    got = gather(sims)
    stats = [s.stats() for s in sims]
    if box_w < 10:
        assert len(ref) < n
    assert len(got) == len(ref)
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), f
    assert sum(s.interactions for s in stats) == s1.interactions and sum(s.node_visits for s in stats) == s1.node_visits
    assert all(s.tree_nodes == s1.tree_nodes for s in stats)
    for s in sims:
        s.close()


@pytest.mark.parametrize("G,n,box_w", [(2, 300, 64.0), (3, 300, 64.0), (2, 3000, 64.0), (3, 3000, 2.5)])
def test_barnes_hut_f64_shards_with_device_tree_equal_single_shard(gpu, tmp_path, G, n, box_w):
    """The f64 twin of the test above: every rank concatenates the gathered f64 blocks (k_tree_cat64), builds the same
    tree on the device and walks it for its own bodies in the order the own-order filter leaves.  An f64 handle exchanges
    inside its step (it has no nbody_debug_* hooks), so the ranks are processes over the one-device transport.  Same tree
    + same per-body walk => the world equals the 1-shard device-tree run bit for bit and the node counts add up exactly;
    bodies leave the 2.5-wide box on the way.  The node-range split is pinned to 8 segments as above."""
    nb = gpu
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], box_w]
    sd = dict(g=1.0, g_soft=0.01, dt=5e-3, theta2=0.25)
    cfg = {"world": G, "out": str(tmp_path / "world"), "transport": "ipc", "device": 0, "box": box, "settings": sd, "env": {},
           "sim": dict(method="bh", math="fast", tree="device", tuning=dict(bh_walk_split=8)), "ics": dict(n=n, seed=31, f64=True),
           "schedule": [["steps", 5]]}
    res = ranks.run_world(cfg, ranks_per_process=1, timeout=120)
    got = ranks.gather_world(res)
    ics = ranks.make_ics(nb, cfg["ics"])
    with ranks.make_sim(nb, cfg, ics, 0, 1, 0) as one:
        one.settings = nb.Settings(**sd)
        one.init()
        one.steps(5)
        ref = one.get_points()
        s1 = one.stats()
    assert got.dtype == nb.PARTICLE_DTYPE64 and all(r["f64"] for r in res)
    if box_w < 10:
        assert len(ref) < n
    assert len(got) == len(ref)
    for f in FIELDS:
        print(f"G={G} n={n} {f}: max |world - one| = {np.abs(got[f] - ref[f]).max():.3e}")
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), f
    assert sum(r["interactions"] for r in res) == s1.interactions and sum(r["node_visits"] for r in res) == s1.node_visits
    assert all(r["tree_nodes"] == s1.tree_nodes for r in res)


def test_rccl_single_rank_communicator(gpu, orc):
    """The RCCL code path itself (ncclGetUniqueId, ncclCommInitRank, grouped in-place all-gathers on
    the handle's stream) with a world of one: results must not change."""
    nb = gpu
    sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    ics = nb.plummer(777, seed=3)
    with nb.Simulation(ics, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.STRICT) as sim:
        sim.settings = nb.Settings(**sd)
        sim.comm_init(nb.comm_unique_id())
        sim.steps(4)
        got = sim.get_points()
    ref = ics.copy().astype(orc.P32)
    for _ in range(4):
        ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], sd["dt"])
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f


@pytest.mark.parametrize("method,math", [("BRUTE_FORCE", "FAST"), ("BARNES_HUT", "STRICT")])
def test_rccl_single_rank_communicator_other_paths(gpu, orc, method, math):
    """Same with the fast symmetric path (n >= 8192: the exchange runs on its own stream beside the
    force kernel) and with Barnes-Hut."""
    nb = gpu
    sd = dict(g=1.0, g_soft=0.01, dt=1e-3, theta2=0.25)
    ics = nb.plummer(9000, seed=4)
    outs = []
    for with_comm in (False, True):
        with nb.Simulation(ics, *BOX, method=getattr(nb, method), math_mode=getattr(nb, math)) as sim:
            sim.settings = nb.Settings(**sd)
            if with_comm:
                sim.comm_init(nb.comm_unique_id())
            sim.steps(3)
            sim.update_forces()
            outs.append(sim.get_points())
    assert np.array_equal(outs[0], outs[1])


def test_sharded_handle_without_communicator_fails_loudly(gpu):
    nb = gpu
    ics = nb.plummer(64)
    with nb.Simulation(ics, *BOX, rank=0, world_size=2, capacity=64) as sim:
        with pytest.raises(nb.NbodyError) as e:
            sim.step()
        assert e.value.code == nb.NBODY_ERR_COMM
        with pytest.raises(nb.NbodyError):
            sim.add_point(ics[0])
