"""tests/knn_ref.py checked on the CPU, for the restatement alone: against plain Python loops on small worlds; that k = 1 is
merge_ref's nearest; that the k-list is the first k of the 32-list; and the conditions that keep tests/test_knn_gpu.py from
being vacuous -- rows with a tie at the k-th place, padded rows, and for every (world, k) that the GPU tests run with a hint,
both rows that the cells finish and rows that go to the all-pairs pass, or the proof that no hint could give both.  Then that
the header, the ctypes mirror, host/simulation.hpp and the shared object declare the three calls.  No device."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import knn_ref as ref
import merge_ref
import within_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nbody_knn", "nbody_knn_density", "nbody_knn_density_center"]
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
#: the (world, k) with more than k bodies in which no hint can leave both finished and unfinished rows: every row is complete
#: and all stand at one k-th distance (0 among coincident bodies, the spacing in a lattice)
#: (side_lattice: in f64 only -- rounded to f32 its spacings differ)
UNSPLITTABLE = {("coincident", 1), ("coincident", 6), ("coincident", 32), ("lattice", 1), ("side_lattice", 1), ("clumpy2", 1)}


@functools.lru_cache(maxsize=None)
def full(nb, name, f64):
    rec, radii = within_ref.world(nb, name, f64)
    return rec, radii, ref.lists(rec, ref.MAX_K)


def loop_lists(rec, k):
    """rows of (r2, j) by two nested loops over Python floats, sorted as tuples"""
    x = [[float(v) for v in p] for p in rec["position"]]
    out = []
    for i in range(len(x)):
        mine = []
        for j in range(len(x)):
            if j == i:
                continue
            dx, dy, dz = x[j][0] - x[i][0], x[j][1] - x[i][1], x[j][2] - x[i][2]
            r2 = (dx * dx + dy * dy) + dz * dz
            if r2 < math.inf:
                mine.append((r2, j))
        out.append(sorted(mine)[:k])
    return out


@DTYPES
@pytest.mark.parametrize("name", ["clumpy2", "clumpy255", "coincident", "huge", "holed_lattice", "wall_pairs"])
def test_the_restatement_is_the_plain_loop(nb, name, f64):
    rec, _, _ = full(nb, name, f64)
    m = np.ascontiguousarray(rec["mass"], np.float64)
    for k in ref.KS:
        neighbor, dist2 = ref.lists(rec, k)
        want = loop_lists(rec, k)
        rho, rk2 = ref.density(rec, max(k, 2), *ref.lists(rec, max(k, 2)))
        for i, mine in enumerate(want):
            assert [int(j) for j in neighbor[i, : len(mine)]] == [j for _, j in mine]
            assert [float(v) for v in dist2[i, : len(mine)]] == [r2 for r2, _ in mine]
            assert (neighbor[i, len(mine):] == -1).all() and (dist2[i, len(mine):] == np.inf).all()
        kk = max(k, 2)
        for i, mine in enumerate(loop_lists(rec, kk)):
            if len(mine) < kk:
                assert rho[i] == 0.0 and not np.signbit(rho[i]) and rk2[i] == np.inf
                continue
            M = 0.0
            for _, j in mine[: kk - 1]:
                M += float(m[j])
            r = math.sqrt(mine[kk - 1][0])
            with np.errstate(all="ignore"):
                want_rho = np.float64(M) / np.float64(4.1887902047863905 * ((r * r) * r))
            assert ref.same_bits(rho[i], want_rho) and rk2[i] == mine[kk - 1][0]


@DTYPES
@pytest.mark.parametrize("name", within_ref.WORLDS)
def test_k_1_is_nearest_and_the_lists_are_prefixes(nb, name, f64):
    rec, _, (neighbor32, dist32) = full(nb, name, f64)
    n1, d1 = ref.lists(rec, 1)
    want_n, want_d = merge_ref.nearest(rec)
    assert np.array_equal(n1[:, 0], want_n) and n1[:, 0].dtype == np.int32 and d1[:, 0].tobytes() == want_d.tobytes()
    for k in (1, 2, 6, 31):
        nk, dk = ref.lists(rec, k)
        assert np.array_equal(nk, neighbor32[:, :k]) and dk.tobytes() == np.ascontiguousarray(dist32[:, :k]).tobytes()
    # every row: ascending in (r2, j), no body twice, never the row itself, the padding at the end
    for i in range(len(rec)):
        held = int((neighbor32[i] >= 0).sum())
        assert (neighbor32[i, held:] == -1).all() and (dist32[i, :held] < np.inf).all() and i not in neighbor32[i, :held]
        assert len(set(neighbor32[i, :held].tolist())) == held
        pairs = list(zip(dist32[i, :held].tolist(), neighbor32[i, :held].tolist()))
        assert pairs == sorted(pairs)


def test_the_worlds_hold_ties_at_the_k_th_place_and_padded_rows(nb):
    """a tie at the k-th place: the body at place k + 1 of the row's order stands at the same r2 as the k-th"""
    for name in ("lattice", "two_lattices", "coincident"):
        rec, _, (_, dist32) = full(nb, name, True)
        for k in (1, 6):
            assert (dist32[:, k - 1] == dist32[:, k]).any() and (dist32[:, k] < np.inf).any(), (name, k)
    rec, _, (neighbor32, dist32) = full(nb, "coincident", True)
    assert (dist32[:, :32] == 0.0).all() and np.array_equal(neighbor32[5, :6], [0, 1, 2, 3, 4, 6]), "ties resolve to ascending index"
    padded = {}
    for name in within_ref.WORLDS:
        _, _, (neighbor32, _) = full(nb, name, True)
        padded[name] = int((neighbor32[:, 5] < 0).sum()) if len(neighbor32) else 0
    assert padded["holed_lattice"] >= 2 and padded["huge"] >= 2 and padded["clumpy2"] == 2
    rec, _, (neighbor32, _) = full(nb, "huge", True)
    assert (neighbor32[7] == -1).all() and 7 not in neighbor32, "a body at 1e308 has nobody and is nobody's"


@DTYPES
@pytest.mark.parametrize("name", within_ref.WORLDS)
def test_the_hints_leave_finished_and_unfinished_rows(nb, name, f64):
    rec, radii, (_, dist32) = full(nb, name, f64)
    for k in ref.KS:
        dist2 = np.ascontiguousarray(dist32[:, :k])
        hint = ref.split_hint(dist2, k)
        if hint is None:
            # no hint can split these rows: no complete row, or every row complete at one and the same k-th distance
            kth = dist2[:, k - 1] if len(rec) else np.zeros(0)
            assert not (kth < np.inf).any() or ((kth < np.inf).all() and len(np.unique(kth)) == 1), (name, k)
            assert (name, k) in UNSPLITTABLE or len(rec) <= k, (name, k)
            continue
        assert hint > 0.0 and len(rec) > k, (name, k)
        finished, rest = ref.stats(rec, k, hint, dist2)
        if not ref.grid_runs(rec, hint):   # coordinates of +-1e308 in f64: no grid can be drawn, every row goes to all pairs
            assert name == "huge" and f64 and (finished, rest) == (0, len(rec))
            continue
        assert finished > 0 and rest > 0 and finished + rest == len(rec), (name, k, hint, finished, rest)
        wide = ref.stats(rec, k, 4.0 * hint, dist2)
        assert wide[0] >= finished and sum(wide) == len(rec)
        assert ref.stats(rec, k, 0.0, dist2) == (0, len(rec))


def test_header_mirror_and_library_declare_the_calls(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    host = open(os.path.join(ROOT, "nbody-llm_amd", "host", "simulation.hpp")).read()
    lib = C.CDLL(nb.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s + "(" in header and s in nb.DECLARED_SYMBOLS and hasattr(lib, s) and s + "(" in host, s
    assert "enum { NBODY_KNN_MAX_K = 32 };" in header and nb.KNN_MAX_K == ref.MAX_K == 32
    assert "not a k-nearest-neighbour search" not in header
    assert "not a k-nearest-neighbour search" not in open(os.path.join(ROOT, "README.md")).read()
    # a NULL handle is refused without touching a device
    assert nb.lib.nbody_knn(None, 6, 0.0, None, None, 0, None, None) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_knn_density(None, 6, 0.0, None, None, 0, None) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_knn_density_center(None, 6, 0.0, None, None) == nb.NBODY_ERR_INVALID
