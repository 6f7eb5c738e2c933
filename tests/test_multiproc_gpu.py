"""The PRODUCTION multi-rank step with G real ranks on ONE GPU: every rank a fresh process (G = 8: four processes of
two rank threads -- a GPU box admits six GPU processes), each calling nbody_step_by / nbody_steps on its own handle;
the library's own exchange code (exchange_begin / partials_begin in nbody_f32.cpp, let::pass in nbody_let.cpp: count
matrices, variable-size rounds, the communication stream and its events, the host synchronisations) runs over the
one-device transport of csrc/transport_ipc.hip instead of RCCL, which refuses two ranks on one device.  No
nbody_debug_* hook is involved; the control plane is nbody-llm_amd/rendezvous.py (stdlib sockets, no torch).
Oracle = the single-handle run of the same schedule (and through it the CPU oracle, tests/test_sharded_gpu.py,
tests/test_spatial_gpu.py), with the tolerances those tests use."""
import json
import os

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
BOX = [[0.0, 0.0, 0.0], 64.0]
FIELDS = ("position", "velocity", "acceleration", "mass")


def world_cfg(tmp_path, G, sim, ics, settings, schedule, box=BOX, env=None, **extra):
    cfg = {"world": G, "out": str(tmp_path / "world"), "transport": "ipc", "device": 0, "sim": sim, "ics": ics, "box": box,
           "settings": settings, "schedule": schedule, "env": env or {}}
    cfg.update(extra)
    return cfg


def single(nb, cfg, **kw):
    """the same schedule on one handle"""
    from nbody_llm_amd import ranks
    pts = ranks.make_ics(nb, cfg["ics"])
    one = dict(cfg, sim=dict(cfg["sim"], shard="index", **kw))
    with ranks.make_sim(nb, one, pts, 0, 1, 0) as sim:
        sim.settings = nb.Settings(**cfg["settings"])
        sim.init()
        sim = ranks.run_schedule(nb, sim, cfg["schedule"])
        return sim.get_points(), sim.stats()


def launch(cfg, G):
    from nbody_llm_amd import ranks
    per = 1 if G <= 5 else 2    # (the parent holds the GPU too: at most five more processes)
    return ranks.run_world(cfg, ranks_per_process=per, timeout=240)


@pytest.mark.parametrize("G", [2, 3])
def test_brute_force_strict_ranks_are_bit_equal_to_one_handle_and_the_oracle(gpu, orc, tmp_path, G):
    nb = gpu
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.0, dt=1e-3, theta2=0.5)
    cfg = world_cfg(tmp_path, G, dict(method="bf", math="strict"), dict(n=1000, seed=G), sd, [["steps", 3], ["step_by", 2e-3], ["step_by", -1e-3]])
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    assert all(r["transport"] == "ipc" and r["steps"] == 5 for r in res)
    assert [tuple(r["local_range"]) for r in res] == [(lo, hi - lo) for lo, hi in (nb.shard_range(1000, r, G) for r in range(G))]
    ref = ranks.make_ics(nb, cfg["ics"]).astype(orc.P32)
    for dt in (1e-3, 1e-3, 1e-3, 2e-3, -1e-3):
        ref = orc.bf_step_by(ref, sd, BOX[0], BOX[1], dt)
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f


@pytest.mark.parametrize("cross", ["1", "0"])
@pytest.mark.parametrize("G,n", [(2, 6000), (3, 10000), (4, 9001), (2, 4095), (8, 16385), (8, 20000)])
def test_brute_force_fast_ranks_with_escapes(gpu, orc, tmp_path, G, n, cross):
    """fast math over index-block shards, shard capacities on both sides of the 2 048-body threshold, bodies leaving a
    tight box on different ranks: the all-gather of positions and counts, the symmetric scheme across shards with its
    send/recv round of partial sums (cross = 1) or the one-sided form (cross = 0)."""
    nb = gpu
    from nbody_llm_amd import ranks
    if cross == "0" and G == 8 and n == 20000:
        pytest.skip("one-sided form: covered at the smaller sizes")
    box = [[0.0, 0.0, 0.0], 3.0]
    sd = dict(g=1.0, g_soft=0.05, dt=2e-2, theta2=0.5)
    cfg = world_cfg(tmp_path, G, dict(method="bf", math="fast"), dict(n=n, seed=12, mass_jitter=n), sd, [["steps", 2], ["step_by", 2e-2], ["steps", 1]],
                    box=box, env={"NBODY_CROSS_SYM": cross})
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    ref = ranks.make_ics(nb, cfg["ics"]).astype(orc.P32)
    for _ in range(4):
        if n <= 12000:
            ref = orc.bf_step_by(ref, sd, box[0], box[1], sd["dt"])
        else:
            orc.pre_force(ref, sd["dt"])
            ref = orc.retain(ref, box[0], box[1])
            orc.bf_update_forces_rows(ref, sd, threads=16)
            orc.after_force(ref, sd["dt"])
    assert len(got) == len(ref) < n
    assert sum(r["count"] for r in res) == res[0]["count_global"] == len(ref)
    assert np.array_equal(got["mass"], ref["mass"])
    assert rel_err(got["position"], ref["position"]) < 1e-5
    assert rel_err(got["acceleration"], ref["acceleration"]) < 3e-5


@pytest.mark.parametrize("G,tree,math", [(2, "host", "strict"), (4, "device", "strict"), (3, "device", "fast"), (4, "host", "fast")])
def test_barnes_hut_replicated_tree_ranks(gpu, tmp_path, G, tree, math):
    """Barnes-Hut over index blocks (every rank builds the world's tree from the gathered positions and walks its own
    bodies): strict math is bit-equal to the one-handle run, fast math agrees to rounding."""
    nb = gpu
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], 4.0]
    sd = dict(g=1.0, g_soft=0.01, dt=1e-2, theta2=0.25)
    cfg = world_cfg(tmp_path, G, dict(method="bh", math=math, tree=tree), dict(n=5000, seed=31), sd, [["steps", 4], ["update_forces"]], box=box)
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    ref, s1 = single(nb, cfg)
    assert len(got) == len(ref) < 5000
    if math == "strict":
        for f in FIELDS:
            assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
        assert sum(r["interactions"] for r in res) == s1.interactions and sum(r["node_visits"] for r in res) == s1.node_visits
    else:
        assert rel_err(got["position"], ref["position"]) < 1e-6
        assert rel_err(got["acceleration"], ref["acceleration"]) < 1e-5
    assert all(r["tree_nodes"] == s1.tree_nodes for r in res)


def assert_same_up_to_flips(got, ref, tol):
    n = len(ref)
    err = np.abs(np.asarray(got, np.float64) - ref).max(axis=1) / np.abs(ref).max()
    far = np.count_nonzero(err > tol)
    assert far <= max(1, n // 5000) and err.max() < 1e-4, (err.max(), far)


@pytest.mark.parametrize("G,n,box_w,leaf", [(2, 3000, 64.0, "reference"), (4, 20000, 3.0, "reference"), (3, 9000, 2.5, "direct"), (8, 20000, 3.0, "reference")])
def test_barnes_hut_spatial_ranks_with_migration(gpu, tmp_path, G, n, box_w, leaf):
    """Barnes-Hut over spatial shards: the four exchanges of a step (migrants and tree nodes in variable-size rounds,
    their count matrices, the end-info and spanning-cell tables) between real ranks, with bodies leaving a tight box and
    migrating as the bounds are redrawn; the world stays with the one-handle device-tree run."""
    nb = gpu
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], box_w]
    sd = dict(g=1.0, g_soft=0.01, dt=5e-3, theta2=0.25)
    cfg = world_cfg(tmp_path, G, dict(method="bh", math="fast", shard="spatial", leaf=leaf), dict(n=n, seed=64), sd, [["steps", 4], ["step_by", 5e-3], ["steps", 1]], box=box)
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    ref, s1 = single(nb, cfg, tree="device")
    assert sum(r["count"] for r in res) == res[0]["count_global"] == len(ref) == len(got)
    if box_w < 10:
        assert len(ref) < n
    assert np.array_equal(got["mass"], ref["mass"])
    assert np.abs(got["position"].astype(np.float64) - ref["position"]).max() < 2e-6
    assert_same_up_to_flips(got["acceleration"], ref["acceleration"], 1e-5)
    acc = sum(r["interactions"] for r in res)
    assert abs(acc - s1.interactions) <= 1e-5 * s1.interactions
    if G > 1:
        assert sum(r["let"]["nodes_sent"] for r in res) == sum(r["let"]["nodes_received"] for r in res) > 0
        if box_w < 10:
            assert sum(r["let"]["bodies_migrated"] for r in res) > 0
        for r in res:   # one host synchronisation per step (+ one more in the first, which learns the migrant counts the slow way, and per repeated migrant round)
            assert r["let"]["steps"] == 6 and r["let"]["host_syncs"] == 6 + 1 + r["let"]["migrant_respills"], r["let"]
            assert 0 < r["let"]["node_array_peak_bytes"] <= r["let"]["node_array_bytes"]


def test_spatial_ranks_grow_their_node_list_buffers_inside_a_step(gpu, tmp_path):
    """The export lists lie one after the other in a buffer sized for a quarter of the slice's node capacity, the imports
    are staged in one of the same size; a step that needs more grows them where the host has just read the counts (the
    export lists are then written again).  With buffers of ~1 000 records every step of this world does: same bodies, to
    the bit, as with the default sizes."""
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], 3.0]
    sd = dict(g=1.0, g_soft=0.01, dt=5e-3, theta2=0.25)
    runs = []
    for k, tuning in enumerate((None, {"let_list_div": 1 << 20})):
        sim = dict(method="bh", math="fast", shard="spatial")
        if tuning:
            sim["tuning"] = tuning
        cfg = world_cfg(tmp_path / f"run{k}", 4, sim, dict(n=20000, seed=64), sd, [["steps", 4]], box=box)
        runs.append(launch(cfg, 4))
    a, b = (ranks.gather_world(r) for r in runs)
    assert len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for ra, rb in zip(*runs):
        assert ra["let"]["nodes_received"] == rb["let"]["nodes_received"] > 4 * 2048   # (more than the small buffers held at first)
        assert rb["let"]["node_array_bytes"] < ra["let"]["node_array_bytes"]


def test_spatial_step_repeats_its_migrant_round_when_the_posted_sizes_do_not_hold(gpu, tmp_path):
    """The migrant messages of a step are posted with sizes drawn from the previous step's counts.  Two quiet steps, then
    one that moves every body a long way: far more bodies change ranks than predicted, every rank sees it in the
    all-gathered count matrix, nothing is committed, and the round is made again with the exact sizes -- the world still
    equals the one-handle run."""
    nb = gpu
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.01, dt=1e-4, theta2=0.25)
    cfg = world_cfg(tmp_path, 3, dict(method="bh", math="fast", shard="spatial"), dict(n=6000, seed=66), sd,
                    [["step_by", 1e-4], ["step_by", 1e-4], ["step_by", 0.4], ["step_by", 1e-4], ["step_by", 1e-4]])
    res = launch(cfg, 3)
    got = ranks.gather_world(res)
    ref, s1 = single(nb, cfg, tree="device")
    assert len(got) == len(ref) == 6000
    assert np.abs(got["position"].astype(np.float64) - ref["position"]).max() < 5e-6
    assert_same_up_to_flips(got["acceleration"], ref["acceleration"], 1e-5)
    assert all(r["let"]["migrant_respills"] >= 1 for r in res), [r["let"] for r in res]
    assert len({r["let"]["migrant_respills"] for r in res}) == 1          # every rank repeated the same rounds
    assert sum(r["let"]["bodies_migrated"] for r in res) > 500
    for r in res:
        assert r["let"]["host_syncs"] == 5 + 1 + r["let"]["migrant_respills"]


EDITS = [["steps", 2], ["add_point", [0.3, -0.2, 0.1, 0.0, 0.4, 0.0, 2e-3]], ["steps", 1], ["remove_point", 5], ["steps", 1], ["clone"],
         ["remove_point", 1499], ["add_point", [-0.5, 0.5, 0.25, 0.1, 0.0, -0.1, 1e-3]], ["add_point", [0.05, 0.0, -0.3, 0.0, 0.0, 0.2, 1e-3]],
         ["remove_point", 700], ["steps", 2]]


@pytest.mark.parametrize("G,method,math", [(3, "bf", "strict"), (2, "bh", "strict"), (4, "bf", "fast")])
def test_trait_surface_on_index_block_ranks_push_swap_remove_clone(gpu, tmp_path, G, method, math):
    """Simulation::add_point = Vec::push, remove_point = Vec::swap_remove, Clone (src/shared.rs:80,91-92; the visualiser uses all
    three, src/vis.rs:217-251) on a world of index-block ranks: collective calls, the vector being the concatenation of the
    ranks' blocks (a push lands in the last rank's block, swap_remove moves the world's last body across ranks).  The world
    equals the one-handle run of the same schedule -- strict math: bit for bit."""
    nb = gpu
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.02, dt=2e-3, theta2=0.25)
    cfg = world_cfg(tmp_path, G, dict(method=method, math=math, capacity=1600), dict(n=1500, seed=71), sd, EDITS)
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    ref, _ = single(nb, cfg)
    assert len(got) == len(ref) == 1500
    assert sum(r["count"] for r in res) == res[0]["count_global"] == 1500
    if math == "strict":
        for f in FIELDS:
            assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    else:
        assert np.array_equal(got["mass"], ref["mass"])
        assert rel_err(got["position"], ref["position"]) < 1e-6 and rel_err(got["acceleration"], ref["acceleration"]) < 1e-5


def test_trait_surface_on_spatial_ranks_push_swap_remove_clone(gpu, tmp_path):
    """The same on spatial shards: a pushed body goes to the rank that owns its key range and takes the next free index of the
    vector; swap_remove(i) removes the body with the i-th index and hands its index to the world's last one; a clone carries
    the bodies, their indices and the ownership bounds."""
    nb = gpu
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.02, dt=2e-3, theta2=0.25)
    cfg = world_cfg(tmp_path, 3, dict(method="bh", math="fast", shard="spatial", capacity=1600), dict(n=1500, seed=71), sd, EDITS)
    res = launch(cfg, 3)
    got = ranks.gather_world(res)
    ref, _ = single(nb, cfg, tree="device")
    assert len(got) == len(ref) == 1500 and sum(r["count"] for r in res) == res[0]["count_global"] == 1500
    assert sorted(np.concatenate([r["ids"] for r in res]).tolist()) == list(range(1500))     # the indices stay those of a Vec of 1500
    assert np.array_equal(got["mass"], ref["mass"])
    assert np.abs(got["position"].astype(np.float64) - ref["position"]).max() < 2e-6
    assert_same_up_to_flips(got["acceleration"], ref["acceleration"], 1e-5)


@pytest.mark.parametrize("G,method,leaf", [(2, "bf", "reference"), (4, "bf", "reference"), (2, "bh", "reference"), (4, "bh", "direct")])
def test_f64_ranks_are_bit_equal_to_one_handle_and_the_oracle(gpu, orc, tmp_path, G, method, leaf):
    """F = f64 (the precision the reference's own driver runs, src/main.rs:52-105) over index-block shards: strict arithmetic,
    the replicated tree built on the host; with bodies leaving a tight box the world equals the one-handle run and the
    oracle's f64 instantiation bit for bit."""
    nb = gpu
    from nbody_llm_amd import ranks
    box = [[0.0, 0.0, 0.0], 3.0]
    sd = dict(g=1.0, g_soft=0.05, dt=1e-2, theta2=0.25)
    cfg = world_cfg(tmp_path, G, dict(method=method, math="strict", leaf=leaf), dict(n=1500, seed=81, f64=True), sd, [["steps", 4], ["step_by", -5e-3], ["update_forces"]], box=box)
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    assert got.dtype == nb.PARTICLE_DTYPE64 and all(r["f64"] for r in res)
    ref = ranks.make_ics(nb, cfg["ics"]).astype(orc.P64)
    lm = 1 if leaf == "direct" else 0
    for dt in (1e-2, 1e-2, 1e-2, 1e-2, -5e-3):
        ref = orc.bf_step_by(ref, sd, box[0], box[1], dt) if method == "bf" else orc.bh_step_by(ref, sd, box[0], box[1], dt, threads=4, leaf_mode=lm)[0]
    if method == "bf":
        orc.bf_update_forces(ref, sd)
    else:
        orc.bh_update_forces(ref, sd, box[0], box[1], threads=4, leaf_mode=lm)
    assert len(got) == len(ref) < 1500 and sum(r["count"] for r in res) == res[0]["count_global"] == len(ref)
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint64), ref[f].view(np.uint64)), f


@pytest.mark.parametrize("tree,G,n", [("host", 3, 6000), ("device", 3, 6000), ("device", 2, 40000)])
def test_f64_fast_walk_ranks(gpu, tmp_path, tree, G, n):
    """NBODY_MATH_FAST on f64 ranks: the fast walk over the replicated tree -- built on the host, or (round 3) by every rank
    on the device from the gathered positions (k_tree_cat64 + the f64 device build + the own-order filter) -- to f64
    rounding of the one-handle run with the same build, bodies leaving the box on the way."""
    nb = gpu
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.01, dt=5e-3, theta2=0.25)
    cfg = world_cfg(tmp_path, G, dict(method="bh", math="fast", tree=tree), dict(n=n, seed=82, f64=True), sd, [["steps", 5]], box=[[0.0, 0.0, 0.0], 4.0])
    res = launch(cfg, G)
    got = ranks.gather_world(res)
    ref, s1 = single(nb, cfg)
    assert len(got) == len(ref) < n
    assert np.abs(got["position"] - ref["position"]).max() < 1e-12
    assert sum(r["interactions"] for r in res) == s1.interactions


def test_ranks_created_unlike_fail_at_comm_init_instead_of_hanging(gpu, tmp_path):
    """Two ranks that disagree on the exchange scheme (NBODY_CROSS_SYM) would deadlock in the send/recv round of partial
    sums; nbody_comm_init compares what every rank was created with and refuses."""
    from nbody_llm_amd import ranks
    sd = dict(g=1.0, g_soft=0.05, dt=1e-3, theta2=0.5)
    cfg = world_cfg(tmp_path, 2, dict(method="bf", math="fast"), dict(n=6000, seed=1), sd, [["steps", 1]], env_by_rank={"1": {"NBODY_CROSS_SYM": "0"}})
    with pytest.raises(RuntimeError) as e:
        ranks.run_world(cfg, timeout=120)
    assert "disagree on NBODY_CROSS_SYM" in str(e.value)


def test_one_rank_world_with_a_communicator_runs_every_collective(gpu):
    """A world of one WITH a communicator goes through every exchange of the spatial step (the all-gathers in place, the
    count matrices, empty send/recv rounds) on either transport; results = the plain device-tree run."""
    nb = gpu
    st = nb.Settings(1.0, 0.01, 1e-3, 0.25)
    ics = nb.plummer(3000, seed=65)
    with nb.Simulation(ics, *((0.0, 0.0, 0.0), 64.0), method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as one:
        one.settings = st
        one.steps(3)
        ref = one.get_points()
    for ident, name in ((nb.comm_local_id(), "ipc"), (nb.comm_unique_id(), "rccl")):
        with nb.Simulation(ics, *((0.0, 0.0, 0.0), 64.0), method=nb.BARNES_HUT, math_mode=nb.FAST, shard_mode=nb.SHARD_SPATIAL) as sim:
            sim.settings = st
            sim.comm_init(ident)
            assert sim.comm_transport() == name
            sim.steps(3)
            got = sim.get_points()
            ids = sim.download_ids()
        assert np.array_equal(ids, np.arange(3000))
        assert np.abs(got["position"].astype(np.float64) - ref["position"]).max() < 1e-6
