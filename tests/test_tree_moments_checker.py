"""The tree-moment checker (tests/tree_moments.py) on the CPU: it accepts what the host build -- the reference's own fold --
makes of every world of tests/test_tree_moments_gpu.py, and it rejects planted faults: the moments as plain f64 prefix-sum
differences (what the device build computed before it carried double-doubles), one mass 8 ulp off, one centre 8 u A_a off."""
import numpy as np
import pytest

import tree_moments as tm
from test_bh_device_tree_gpu import close_pairs, lattice_pairs


def host_tree(nb, orc, ics, box):
    """The reference's fold over the records' own precision: nbody_host_build_tree (f32), the oracle's build (f64)."""
    if ics.dtype == nb.PARTICLE_DTYPE:
        return nb.host_build_tree(np.concatenate([ics["position"], ics["mass"][:, None]], axis=1), *box)
    return orc.bh_build_tree(ics.astype(orc.P64), *box)


def worlds(nb, f64):
    """(name, records, box, massless cells) of every world the GPU tests use, at the sizes a CPU test can afford."""
    kind = "f64" if f64 else "f32"
    dt = nb.PARTICLE_DTYPE64 if f64 else nb.PARTICLE_DTYPE
    for n in tm.SIZES:
        yield f"control {n}", tm.control_world(nb, n, f64), tm.BOX, 0
        yield f"far {n}", tm.far_world(nb, n, f64), tm.FAR_BOX, 0
    for n in tm.DUST_SIZES:
        for dm in tm.DUST_MASSES[kind]:
            for first in (True, False):
                yield f"dust {dm:g} {n} {'first' if first else 'last'}", tm.dust_world(nb, n, dm, first, f64), tm.BOX, 0
    yield "massless", tm.massless_world(nb, f64=f64), tm.BOX, tm.MASSLESS_CELLS
    yield "deep clumps", tm.deep_world(nb, f64), tm.BOX, 0
    yield "close pairs", tm.light_pairs(close_pairs(dt)), tm.BOX, 0
    yield "lattice pairs", tm.light_pairs(lattice_pairs(dt)), tm.BOX, 0


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_checker_accepts_the_host_build_of_every_world(nb, orc, f64):
    worst = [0.0, 0.0]
    for name, ics, box, massless in worlds(nb, f64):
        ht = host_tree(nb, orc, ics, box)
        r = tm.check_moments(ht, scheme=False, host_tree=ht, what=name)
        assert r["massless"] == massless, name
        worst = [max(a, b) for a, b in zip(worst, r["reference"])]
    print(f"host build, {'f64' if f64 else 'f32'}: worst mass / centre error {worst[0]:.3f} / {worst[1]:.3f} of (n_c + 2) u")
    assert 0.0 < worst[1] <= 1.0


def planted(tree):
    bad = dict(tree)
    bad["com_mass"] = tm.prefix_difference_moments(tree)
    return bad


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("dust", [1e-12, 1e-15])
def test_checker_rejects_prefix_sum_differences_on_the_dust_worlds(nb, orc, f64, dust):
    for first in (True, False):
        ht = host_tree(nb, orc, tm.dust_world(nb, 5000, dust, first, f64), tm.BOX)
        with pytest.raises(AssertionError, match=r"beyond \(n_c \+ 2\) u"):
            tm.check_moments(planted(ht), scheme=False, what="planted")


def test_checker_rejects_prefix_sum_differences_in_the_far_box_f64(nb, orc):
    ht = host_tree(nb, orc, tm.far_world(nb, 5000, True), tm.FAR_BOX)
    with pytest.raises(AssertionError, match=r"beyond \(n_c \+ 2\) u"):
        tm.check_moments(planted(ht), scheme=False, what="planted")


def test_checker_accepts_prefix_sum_differences_on_the_control(nb, orc):
    """Near-equal masses about the origin on an f32 tree: the f64 rounding the prefixes carry stays far below 2^-24 of any
    cell, under either bound (which is why the suite never saw the fault)."""
    for n in (300, 1025, 5000):
        ht = host_tree(nb, orc, tm.control_world(nb, n), tm.BOX)
        tm.check_moments(planted(ht), scheme=True, what="control")


def test_checker_rejects_prefix_sum_differences_on_the_f64_control(nb, orc):
    """On an f64 tree there is no such room: a prefix of n terms carries n 2^-53 of rounding and a two-body cell feels all
    of it, even among equal masses about the origin ("differ in the last bits only" never held)."""
    ht = host_tree(nb, orc, tm.control_world(nb, 1025, True), tm.BOX)
    with pytest.raises(AssertionError, match=r"beyond \(n_c \+ 2\) u"):
        tm.check_moments(planted(ht), scheme=False, what="planted")


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("what", ["mass", "centre"])
def test_checker_rejects_one_small_fault(nb, orc, f64, what):
    """One two-body cell's mass 8 ulp off (16 u M against a bound of 4 u M), or one component of its centre moved by
    8 u A_a, away from the exact value: both bounds reject either."""
    ics = tm.control_world(nb, 300, f64)
    ht = host_tree(nb, orc, ics, tm.BOX)
    ex = tm.exact_moments(ht)
    q = int(np.flatnonzero(ex["n_c"] == 2)[3])
    cell = int(ex["cell"][q])
    ft = ht["com_mass"].dtype.type
    u = tm.U[ht["com_mass"].dtype]
    tm.check_moments(ht, scheme=False, exact=ex)
    bad = dict(ht)
    bad["com_mass"] = ht["com_mass"].copy()
    if what == "mass":
        m = bad["com_mass"][cell, 3]
        for _ in range(8):
            m = np.nextafter(m, ft(np.inf))
        bad["com_mass"][cell, 3] = m
    else:
        a = int(np.argmax(np.asarray(ex["A"][q], np.float64)))
        x = np.longdouble(bad["com_mass"][cell, a])
        away = 1.0 if x >= ex["X"][q, a] else -1.0
        bad["com_mass"][cell, a] = ft(x + away * 8 * u * ex["A"][q, a])
    for scheme in (False, True):
        with pytest.raises(AssertionError, match="1 of"):
            tm.check_moments(bad, scheme=scheme, exact=ex, what=what)
