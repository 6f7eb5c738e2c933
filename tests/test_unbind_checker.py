"""The numpy restatement of nbody_fof_bound_groups (tests/unbind_ref.py) and the worlds of the device tests, checked on the host
alone: every property the device tests (tests/test_unbind_gpu.py) rely on is asserted here on the restatement, so that they
cannot pass vacuously; the restatement's energies are compared with an independently written f64 reference."""
import functools

import numpy as np

import fof_ref
import unbind_ref as ref

B, G, G_SOFT = ref.WORLD_B, ref.WORLD_G, ref.WORLD_G_SOFT


def _nb():
    import __graft_entry__ as graft
    return graft.load_package()


@functools.lru_cache(maxsize=None)
def solved(n, f64, max_iterations=32):
    rec = ref.world(_nb(), n, f64)
    fof = fof_ref.groups(rec, B, 2)
    history = {}
    grp, mem, e = ref.bound_groups(rec, B, G, np.float64(G_SOFT) if f64 else np.float32(G_SOFT), 2, max_iterations, fof=fof, history=history)
    return rec, fof, grp, mem, e, history


def test_the_world_holds_every_case():
    rec, (fof, fof_mem), grp, mem, e, history = solved(3000, True)
    big = grp[np.argmax(grp["fof_count"])]
    who = fof_mem[[g["offset"] for g in fof if g["first"] == big["first"]][0]:][: big["fof_count"]]
    # a group of more than 512 members spread over at least three 256-body tiles of the body index
    assert big["fof_count"] > 512 and len(set((who // 256).tolist())) >= 3
    # ... that converges after at least 3 passes and loses members in at least two different passes
    removed = history[int(big["first"])]
    assert big["converged"] == 1 and big["iterations"] >= 3 and sum(len(r) > 0 for r in removed) >= 2
    assert big["iterations"] == len(removed) + 1 and big["count"] == big["fof_count"] - sum(len(r) for r in removed)
    # ... a removed member with alive members on both sides, in a tile other than tile 0
    gone = np.concatenate(removed)
    alive = np.ones(big["fof_count"], bool)
    alive[gone] = False
    assert any(k >= 256 and alive[k // 256 * 256:k].any() and alive[k + 1:(k // 256 + 1) * 256].any() for k in gone)
    # ... and whose first is itself removed: `first` stays the FoF label
    bound = mem[big["offset"]:big["offset"] + big["count"]]
    assert who[0] == big["first"] and 0 in gone and big["first"] not in bound
    # a hot group that dissolves, and it is a large one
    sizes = {int(g["first"]): int(g["count"]) for g in fof}
    assert history["dissolved"] and max(sizes[f] for f in history["dissolved"]) > 100
    assert not set(history["dissolved"]) & set(grp["first"].tolist()) and len(grp) + len(history["dissolved"]) == len(fof)
    # a cold blob that converges in one pass with nobody removed
    cold = grp[(grp["iterations"] == 1) & (grp["converged"] == 1) & (grp["count"] == grp["fof_count"])]
    assert (cold["count"] > 100).any() and (cold["count"] == 2).any()


def test_the_last_pass_removes_nobody():
    rec, fof, full, _, _, _ = solved(3000, True)
    _, _, grp, mem, e, history = solved(3000, True, max_iterations=2)
    stopped = grp[grp["converged"] == 0]
    assert len(stopped) >= 1 and (stopped["iterations"] == 2).all() and (e >= 0).any()
    for g in stopped:   # one strip only: what the first pass removed
        assert g["count"] == g["fof_count"] - len(history[int(g["first"])][0])
    _, _, one, mem1, _, _ = solved(3000, True, max_iterations=1)   # one pass: the FoF catalogue, nobody removed, nothing dissolved
    assert len(one) == len(fof[0]) and np.array_equal(mem1, fof[1]) and (one["iterations"] == 1).all()
    assert np.array_equal(one["count"], one["fof_count"]) and (one["converged"] == 0).any() and (one["converged"] == 1).any()
    for f in ("mass", "mx", "mv"):
        assert ref.same_bits(one[f], fof[0][f]), f


def test_the_small_worlds():
    for n in (0, 1):
        _, fof, grp, mem, e, _ = solved(n, True)
        assert len(grp) == len(mem) == len(e) == 0
    _, fof, grp, mem, e, _ = solved(2, False)
    assert len(grp) == 1 and mem.tolist() == [0, 1] and (e < 0).all() and grp["converged"][0] == 1
    for n in (255, 256, 257, 1000):
        _, fof, grp, _, _, history = solved(n, False)
        assert history["dissolved"] and (grp["iterations"] >= 3).any() and ((grp["iterations"] == 1) & (grp["count"] > 2)).any(), n


def test_the_energies_against_an_independent_sum():
    """plain np.sum over the partners: within fof_count 2^-52 (g sum |terms| + the kinetic scale), the bound the association
    order implies"""
    for f64 in (False, True):
        rec, _, grp, mem, e, _ = solved(3000, f64)
        assert len(grp) >= 3
        for g in grp:
            who = mem[g["offset"]:g["offset"] + g["count"]]
            want, scale = ref.brute_energy(rec, who, G, np.float64(G_SOFT) if f64 else np.float32(G_SOFT))
            got = e[g["offset"]:g["offset"] + g["count"]]
            assert (np.abs(got - want) <= g["fof_count"] * 2.0 ** -52 * scale).all(), (int(g["first"]), np.abs(got - want).max())


def test_converged_groups_are_bound():
    rec, _, grp, mem, e, _ = solved(3000, True)
    m = np.asarray(rec["mass"], np.float64)
    assert (grp["converged"] == 1).all() and (e < 0).all()
    for g in grp:
        sl = slice(g["offset"], g["offset"] + g["count"])
        assert g["kinetic"] + g["potential"] < 0 and g["kinetic"] >= 0 and g["potential"] < 0
        total = g["kinetic"] + 2.0 * g["potential"]   # sum m e = sum m (0.5 u2 + phi)
        assert abs(np.sum(m[mem[sl]] * e[sl]) - total) <= g["fof_count"] * 2.0 ** -50 * (g["kinetic"] + 2.0 * abs(g["potential"]))
        assert (np.diff(mem[sl]) > 0).all()
    assert (np.diff(grp["first"]) > 0).all() and np.array_equal(grp["offset"], np.concatenate([[0], np.cumsum(grp["count"])[:-1]]))


def test_dead_positions_keep_their_lane_and_their_tile():
    """lane_tree_sum_alive with flags is not the sum of the compacted terms; an empty tile still adds +0.0"""
    rng = np.random.default_rng(3)
    t = rng.standard_normal(700)
    alive = rng.random(700) < 0.7
    want = np.zeros(64)
    for k in np.nonzero(alive)[0]:
        want[k % 64] = want[k % 64] + t[k]
    half = 32
    while half >= 1:
        want[:half] = want[:half] + want[half:2 * half]
        half //= 2
    assert ref.lane_tree_sum_alive(t, alive) == want[0]
    assert ref.lane_tree_sum_alive(t, np.ones(700, bool)) == fof_ref.lane_tree_sum(t)
    # lanes 0, 2, 3: (1e16 + -1e16) + (0 + 1) = 1; compacted to lanes 0, 1, 2: (1e16 + 1) + -1e16 = 0
    t, alive = np.array([1e16, 1.0, -1e16, 1.0]), np.array([True, False, True, True])
    assert ref.lane_tree_sum_alive(t, alive) == 1.0 and fof_ref.lane_tree_sum(t[alive]) == 0.0
