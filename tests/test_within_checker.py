"""tests/within_ref.py checked on the CPU against plain Python loops on tiny worlds: the relation is symmetric, the lists are
ascending, offset[n] is even, every body has its own term, a body with a non-finite coordinate has no neighbours and is
nobody's, and r2 == R2 (u exactly 2.0 at the kernel's edge) is excluded -- on the integer lattice, where spacings are exact.
And the conditions that keep tests/test_within_gpu.py from being vacuous, for the restatement alone: lists longer than one
on average in every clumpy world, a list longer than a wave in the star, an empty list beside a full one.  Then that the
header, the ctypes mirror, host/simulation.hpp and the shared object declare the three calls.  No device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import diag_ref
import within_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nbody_neighbors_within", "nbody_density", "nbody_density_center"]
DTYPES = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])


# ------------------------------------------------------------------------------------------------ plain loops
def loop_lists(rec, radius):
    """[[j ...]] by two nested loops over Python floats (IEEE doubles: every operation rounded on its own)"""
    x = [[float(v) for v in p] for p in rec["position"]]
    R2 = float(radius) * float(radius)
    out = []
    for i in range(len(x)):
        mine = []
        for j in range(len(x)):
            if j == i:
                continue
            dx, dy, dz = x[j][0] - x[i][0], x[j][1] - x[i][1], x[j][2] - x[i][2]
            r2 = (dx * dx + dy * dy) + dz * dz
            if r2 < R2:
                mine.append(j)
        out.append(mine)
    return out


def loop_density(rec, radius, kernel):
    x = [[float(v) for v in p] for p in rec["position"]]
    m = [float(v) for v in rec["mass"]]
    radius = float(radius)
    hs = radius * 0.5
    lists = loop_lists(rec, radius)
    rho, count = [], []
    for i, mine in enumerate(lists):
        s = 0.0
        for j in sorted(mine + [i]):
            if kernel == ref.TOP_HAT:
                s += m[j]
                continue
            if j == i:
                u = 0.0
            else:
                dx, dy, dz = x[j][0] - x[i][0], x[j][1] - x[i][1], x[j][2] - x[i][2]
                u = math.sqrt((dx * dx + dy * dy) + dz * dz) / hs
            if u < 1.0:
                w = (1.0 - 1.5 * (u * u)) + 0.75 * ((u * u) * u)
            else:
                t = 2.0 - u
                assert t >= 0.0
                w = 0.25 * ((t * t) * t)
            s += m[j] * w
        norm = 4.1887902047863905 * ((radius * radius) * radius) if kernel == ref.TOP_HAT else 3.141592653589793 * ((hs * hs) * hs)
        rho.append(s / norm)
        count.append(len(mine) + 1)
    return np.array(rho, np.float64), np.array(count, np.int32)


def loop_center(rec, rho):
    """the block tree written out: 256 slots per block, rows past the end +0.0"""
    x = [[float(v) for v in p] for p in rec["position"]]
    n = len(x)
    total = [0.0] * 4
    for b in range(0, n, 256):
        slot = [[0.0] * 4 for _ in range(256)]
        for t in range(min(256, n - b)):
            r = float(rho[b + t])
            slot[t] = [r, r * x[b + t][0], r * x[b + t][1], r * x[b + t][2]]
        half = 128
        while half:
            for t in range(half):
                slot[t] = [slot[t][q] + slot[t + half][q] for q in range(4)]
            half //= 2
        total = [total[q] + slot[0][q] for q in range(4)]
    center = [total[1 + c] / total[0] for c in range(3)] if n else [math.nan] * 3   # (no bodies: 0 / 0)
    return np.array(center), total[0]


def tiny_worlds(nb, f64):
    """[(name, records, radii)]: small enough for the loops"""
    holed = ref.cells_ref.holed_lattice(nb, f64)
    return [("clumpy40", ref.fof_ref.clumpy(nb, 40, seed=40, f64=f64), (0.1, 3.0)),
            ("lattice", ref.fof_ref.lattice(nb, 3, f64), (1.0, 1.001, 1.5)),
            ("holed_lattice", holed[:40].copy(), (1.0, 1.001)),
            ("coincident", ref.cells_ref.coincident(nb, f64, n=9), (1e-3,)),
            ("one", ref.fof_ref.clumpy(nb, 1, seed=1, f64=f64), (0.1,)),
            ("none", ref.fof_ref.clumpy(nb, 0, seed=0, f64=f64), (0.1,))]


# ------------------------------------------------------------------------------------------------ 1. the restatement against loops
@DTYPES
def test_the_restatement_is_the_plain_loops(nb, f64):
    for name, rec, radii in tiny_worlds(nb, f64):
        for radius in radii:
            lists = loop_lists(rec, radius)
            offset, neighbor = ref.neighbors(rec, radius)
            assert offset.dtype == np.uint64 and neighbor.dtype == np.int32 and len(offset) == len(rec) + 1 and offset[0] == 0
            assert [list(neighbor[int(offset[i]):int(offset[i + 1])]) for i in range(len(rec))] == lists, (name, radius)
            assert int(offset[-1]) == sum(len(v) for v in lists) and int(offset[-1]) % 2 == 0, "twice the unordered pairs"
            for i, mine in enumerate(lists):
                assert mine == sorted(mine) and i not in mine
                assert all(i in lists[j] for j in mine), "the relation is symmetric"
            for kernel in ref.KERNELS:
                rho, count = ref.density(rec, radius, kernel)
                want_rho, want_count = loop_density(rec, radius, kernel)
                assert count.dtype == np.int32 and np.array_equal(count, want_count) and (count >= 1).all(), (name, radius, kernel)
                assert ref.same_bits(rho, want_rho), (name, radius, kernel)
                center, rho_sum = ref.density_center(rec, radius, kernel, rho=rho)
                want_center, want_sum = loop_center(rec, want_rho)
                assert ref.same_bits(center, want_center) and ref.same_bits(rho_sum, want_sum), (name, radius, kernel)
                assert ref.same_bits(diag_ref.tree_sum(ref.center_terms(rec, rho))[0], rho_sum)


def test_no_bodies_give_a_nan_centre_and_a_zero_sum(nb):
    rec = ref.fof_ref.clumpy(nb, 0, seed=0, f64=True)
    center, rho_sum = ref.density_center(rec, 0.1, ref.CUBIC_SPLINE)
    assert np.isnan(center).all() and rho_sum == 0.0
    offset, neighbor = ref.neighbors(rec, 0.1)
    assert list(offset) == [0] and len(neighbor) == 0


@DTYPES
def test_the_own_term_is_the_mass_at_u_zero(nb, f64):
    """an isolated body: count 1, rho = m w(0) / norm with w(0) == 1.0 exactly"""
    rec = ref.fof_ref.clumpy(nb, 40, seed=40, f64=f64)
    offset, _ = ref.neighbors(rec, 0.1)
    alone = np.nonzero(np.diff(offset.astype(np.int64)) == 0)[0]
    assert len(alone) >= 1
    assert float(ref.spline_w(0.0)) == 1.0
    m = rec["mass"].astype(np.float64)
    for kernel in ref.KERNELS:
        rho, count = ref.density(rec, 0.1, kernel)
        assert (count[alone] == 1).all()
        assert ref.same_bits(rho[alone], (0.0 + m[alone]) / ref.norm_of(0.1, kernel))


@DTYPES
def test_a_body_with_a_non_finite_coordinate_has_no_neighbours_and_is_nobody_s(nb, f64):
    rec = ref.cells_ref.holed_lattice(nb, f64)
    for radius in (1.0, 1.001, 1.5):
        offset, neighbor = ref.neighbors(rec, radius)
        for bad in (7, 9):
            assert offset[bad] == offset[bad + 1] and bad not in neighbor
        rho, count = ref.density(rec, radius, ref.CUBIC_SPLINE)
        assert count[7] == 1 and count[9] == 1 and np.isfinite(rho).all(), "its own term only"
        center, rho_sum = ref.density_center(rec, radius, ref.CUBIC_SPLINE, rho=rho)
        assert np.isfinite(rho_sum) and not np.isfinite(center[0]) and np.isfinite(center[1]) and np.isnan(center[2])


@DTYPES
def test_the_edge_of_the_radius_is_excluded(nb, f64):
    """the integer lattice: r2 == 1.0 exactly between axis neighbours.  At radius 1.0, R2 == 1.0 == r2: nobody is a neighbour.
    At 1.001 the six (or fewer) axis neighbours are, at u = sqrt(1.0) / (1.001 / 2) < 2"""
    rec = ref.fof_ref.lattice(nb, 5, f64)
    r2 = ref.triangle_r2(rec)
    assert (r2[np.isfinite(r2)] == np.round(r2[np.isfinite(r2)])).all() and (r2 == 1.0).sum() == 2 * 3 * 4 * 25
    offset, neighbor = ref.neighbors(rec, 1.0)
    assert offset[-1] == 0 and len(neighbor) == 0, "r2 == R2 is outside: the comparison is strict"
    rho, count = ref.density(rec, 1.0, ref.CUBIC_SPLINE)
    assert (count == 1).all()
    offset, neighbor = ref.neighbors(rec, 1.001)
    assert offset[-1] == 2 * 3 * 4 * 25
    assert (np.diff(offset.astype(np.int64)) == (r2 == 1.0).sum(axis=1)).all()
    # u exactly 2.0 can only come from sqrt(r2) == radius, i.e. r2 == R2 when radius^2 is exact: the spline is 0 there, and the
    # relation never lets such a pair in
    assert float(ref.spline_w(2.0)) == 0.0 and float(ref.spline_w(1.0)) == 0.25
    radius = 2.0   # R2 == 4.0 exactly: the bodies two spacings away are at u == 2.0 and are excluded, those at sqrt(3) are in
    adj = ref.relation(rec, radius, r2)
    assert not adj[r2 == 4.0].any() and adj[r2 == 3.0].all() and (r2 == 4.0).any()
    # sqrt(fl(radius^2)) == radius: t = 2 - u is never negative
    for radius in (0.1, 0.25, 1.001, 0.3 * (1.0 + 2.0 ** -19), 1e-9, 2.5e-9, 0.05):
        R2 = np.float64(radius) * np.float64(radius)
        assert np.sqrt(R2) == np.float64(radius)
        below = np.nextafter(R2, 0.0)
        assert 2.0 - np.sqrt(below) / (np.float64(radius) * 0.5) >= 0.0


# ------------------------------------------------------------------------------------------------ 2. the GPU tests are not vacuous
@DTYPES
def test_the_worlds_of_the_gpu_tests_hold_what_they_are_chosen_for(nb, f64):
    seen_empty_beside_full = False
    for name in ref.WORLDS:
        rec, radii = ref.world(nb, name, f64)
        for radius in radii:
            offset, neighbor = ref.neighbors(rec, radius)
            lengths = np.diff(offset.astype(np.int64))
            if name.startswith("clumpy") and len(rec) >= 255:
                assert lengths.mean() > 1.0, (name, lengths.mean())
            if name == "star":
                assert lengths.max() >= 64, "a list longer than a wave"
                assert lengths[300] == 600, "the hub sees the whole shell"
            if len(lengths) > 1 and ((lengths[:-1] == 0) & (lengths[1:] > 0)).any():
                seen_empty_beside_full = True
    assert seen_empty_beside_full, "no world has an empty list next to a non-empty one"


def test_the_large_world_s_radius_gives_lists(nb):
    """the 16 384 clumpy bodies of the device test: the sampled bodies' lists are not all empty and not all alike"""
    rec = ref.fof_ref.clumpy(nb, 16384, seed=16384, f64=False)
    who = np.random.default_rng(5).choice(16384, 256, replace=False)
    lengths = np.array([len(v) for v in ref.rows(rec, who, ref.fof_ref.CLUMPY_B)])
    assert (lengths == 0).any() and lengths.max() >= 64 and lengths.mean() > 1.0


# ------------------------------------------------------------------------------------------------ 3. the layers declare the calls
def test_every_layer_declares_the_three_calls(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    host = open(os.path.join(ROOT, "nbody-llm_amd", "host", "simulation.hpp")).read()
    lib = C.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in nb.DECLARED_SYMBOLS and name + "(" in host and hasattr(lib, name), name
    assert (nb.KERNEL_TOP_HAT, nb.KERNEL_CUBIC_SPLINE) == (ref.TOP_HAT, ref.CUBIC_SPLINE) == (0, 1)
    assert "NBODY_KERNEL_TOP_HAT = 0" in header and "NBODY_KERNEL_CUBIC_SPLINE = 1" in header
    for method in ("neighbors_within", "density", "density_center"):
        assert callable(getattr(nb.Simulation, method))
    assert nb.lib.nbody_abi_version() == 4
    # a NULL handle is refused without touching a device
    n, total = C.c_size_t(0), C.c_uint64(0)
    assert nb.lib.nbody_neighbors_within(None, 0.1, None, 0, None, 0, C.byref(n), C.byref(total)) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_density(None, 0.1, 1, None, None, 0, C.byref(n)) == nb.NBODY_ERR_INVALID
    center = (C.c_double * 3)()
    assert nb.lib.nbody_density_center(None, 0.1, 1, center, None) == nb.NBODY_ERR_INVALID
