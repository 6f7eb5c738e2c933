"""nbody_pm_field's definition without a device (include/nbody_hip.h, "particle-mesh field"): nbody_host_pm_field against the
composition of the three numpy restatements (tests/pm_ref.py) and against the three public host calls chained by hand, byte for
byte; the refused calls; the all-zero grid; Newton's third law as the mesh gives it; two distant bodies against their direct
force."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pm_ref as ref

# |sum m_i acc_i| / sum |m_i acc_i| (the largest component) of the host call on the periodic grids below, as measured when the
# test was written with the exact value 0 as the reference, and two bodies 12 cells apart on an isolated 32^3 grid against the
# direct f64 pair force, |a_pm - a_direct| / |a_direct| (the larger of the two bodies).  The asserted limits are 16 times these
# (DESIGN 3.26's rule; DESIGN 3.27 records the same figures).
MEASURED_MOMENTUM = {("p8x8x8", ref.CIC): 2.650e-16, ("p8x8x8", ref.TSC): 7.138e-16, ("p16x8x4", ref.CIC): 1.453e-16, ("p16x8x4", ref.TSC): 2.691e-16}
MEASURED_PAIR = {ref.CIC: 5.152e-03, ref.TSC: 1.952e-04}   # (a method error -- the bodies are smeared over their stencils -- not a rounding error)


def plan_of(grid_name, gradient):
    """the Poisson constants a grid and a gradient are paired with here: every option of either boundary condition is visited"""
    periodic = ref.GRIDS[grid_name][3]
    if periodic:
        return dict(green=ref.DIFF2, deconvolve=0, soften=0.0) if gradient == ref.GRADIENT2 else dict(green=ref.SPECTRAL, deconvolve=1, soften=0.0)
    return dict(green=0, deconvolve=0, soften=0.0 if gradient == ref.GRADIENT2 else 0.05)


def host(nb, xyz, m, grid_name, scheme, gradient, g=1.25, points=None, phi=True, **kw):
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid_name]
    return nb.host_pm_field(xyz, m, origin, spacing, dims, g, scheme, gradient, periodic, project_axis=axis, points=points, phi=phi, **kw)


def restated(xyz, m, grid_name, scheme, gradient, g=1.25, points=None, **kw):
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid_name]
    return ref.pm_field(xyz, m, origin, spacing, dims, g, scheme, gradient, periodic, project_axis=axis, points=points, **kw)


def same_call(got, want, what):
    for k, name in enumerate(("acc", "phi", "cls", "counts")):
        if name in ("cls", "counts"):
            assert np.array_equal(got[k], want[k]), f"{what}: {name} {got[k]} vs {want[k]}"
        else:
            ref.same_bits(got[k], want[k], f"{what}: {name}")


# ------------------------------------------------------------------------------------------------ 0. the GPU tests' axis world
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_axis_world_meets_every_class_on_the_axis_grids(nb, f64):
    """what tests/test_pm_gpu.py and test_mesh_gpu.py rely on: under AXIS_WORLD the host call reports, on the isolated grids of
    AXIS_GRIDS, bodies inside, partial (of the deposit: CIC and TSC; the one cell of NGP is on the grid or off it), outside (every
    25th body) and skipped (the body that is not finite), and rows of all four classes; on the periodic ones inside and skipped.
    Nothing along the ignored axis."""
    xyz, m = ref.bodies(ref.world(nb, ref.AXIS_WORLD, f64))
    for grid, scheme, gradient in itertools.product(ref.AXIS_GRIDS, ref.SCHEMES, ref.GRADIENTS):
        acc, _, cls, counts = host(nb, xyz, m, grid, scheme, gradient, **plan_of(grid, gradient))
        what = f"{grid} scheme {scheme} gradient {gradient}: {counts}"
        assert int(counts[:4].sum()) == 300 and int(counts[4:].sum()) == 300, what
        if ref.GRIDS[grid][3]:
            assert [int(v) for v in counts] == [299, 0, 0, 1, 299, 0, 0, 1] and set(cls.tolist()) == {0, 3}, what
        else:
            assert all(int(counts[k]) > 0 for k in ((0, 2, 3) if scheme == ref.NGP else (0, 1, 2, 3))), what
            assert all(int(counts[4 + k]) > 0 for k in range(4)) and set(cls.tolist()) == {0, 1, 2, 3}, what
        along = acc[:, ref.GRIDS[grid][4]]
        assert not along.any() and not np.signbit(along).any(), what


# ------------------------------------------------------------------------------------------------ 1. the same bits
@pytest.mark.parametrize("world", ref.WORLDS)
@pytest.mark.parametrize("grid_name", ref.CPU_GRIDS)
def test_host_call_is_the_restatement_byte_for_byte(nb, grid_name, world):
    xyz, m = ref.bodies(ref.world(nb, world, True))
    pts = ref.caller_points(grid_name)
    for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
        kw = plan_of(grid_name, gradient)
        what = f"{grid_name} {world} scheme {scheme} gradient {gradient}"
        got = host(nb, xyz, m, grid_name, scheme, gradient, **kw)
        same_call(got, restated(xyz, m, grid_name, scheme, gradient, **kw), what + " at the bodies")
        assert got[3][:4].sum() == len(m) and got[3][4:].sum() == len(m)
        got = host(nb, xyz, m, grid_name, scheme, gradient, points=pts, **kw)
        same_call(got, restated(xyz, m, grid_name, scheme, gradient, points=pts, **kw), what + " at points")
        assert got[3][:4].sum() == len(m) and got[3][4:].sum() == len(pts)
    if world == "w4099" and not ref.GRIDS[grid_name][3]:
        assert got[3][1] + got[3][2] > 0 and got[3][3] == 1, "some bodies are off the grid and one is not finite"


@pytest.mark.parametrize("grid_name", ref.CPU_GRIDS)
def test_host_call_is_the_three_host_calls_chained_by_hand(nb, grid_name):
    origin, spacing, dims, periodic, axis = ref.GRIDS[grid_name]
    xyz, m = ref.bodies(ref.world(nb, "w4099", True))
    pts = ref.caller_points(grid_name)
    for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
        kw = plan_of(grid_name, gradient)
        mass, c_dep = nb.host_deposit(xyz, m, origin, spacing, dims, scheme, periodic, axis)
        pot = nb.host_grid_poisson(mass, spacing, 1.25, periodic, kw["green"], kw["soften"], kw["deconvolve"], scheme)
        for p in (None, pts):
            at = xyz if p is None else p
            grad, cls, c_smp = nb.host_grid_sample(at, pot, origin, spacing, scheme, gradient, periodic, axis)
            val = nb.host_grid_sample(at, pot, origin, spacing, scheme, nb.SAMPLE_VALUE, periodic, axis)[0][:, 0]
            got = host(nb, xyz, m, grid_name, scheme, gradient, points=p, **kw)
            same_call(got, (0.0 - grad, val, cls, np.concatenate([c_dep, c_smp])), f"{grid_name} scheme {scheme} gradient {gradient}")
    # phi NULL: the rest is the same, and cls and counts may be NULL too
    full = host(nb, xyz, m, grid_name, ref.TSC, ref.GRADIENT4, **plan_of(grid_name, ref.GRADIENT4))
    acc = host(nb, xyz, m, grid_name, ref.TSC, ref.GRADIENT4, phi=False, **plan_of(grid_name, ref.GRADIENT4))
    assert acc[1] is None
    ref.same_bits(acc[0], full[0], "phi NULL")
    spec = nb.grid_spec(origin, spacing, dims, ref.TSC, nb.DEPOSIT_MASS, periodic, axis)
    pm = nb.pm_spec(1.25, ref.GRADIENT4, **plan_of(grid_name, ref.GRADIENT4))
    bare = np.zeros((len(m), 3))
    assert nb.lib.nbody_host_pm_field(xyz.ctypes.data, m.ctypes.data, len(m), C.byref(spec), C.byref(pm), None, 0, bare.ctypes.data, None, None, None) == 0
    ref.same_bits(bare, acc[0], "cls and counts NULL")


# ------------------------------------------------------------------------------------------------ 2. the refused calls
def test_refusals(nb):
    xyz, m = ref.bodies(ref.world(nb, "n65", True))
    n = len(m)
    acc, phi, cls, counts = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint8), np.zeros(8, np.uint64)

    def call(spec, pm, bx=xyz, bm=m, nb_=n, pts=None, npts=0, out=acc):
        return nb.lib.nbody_host_pm_field(None if bx is None else bx.ctypes.data, None if bm is None else bm.ctypes.data, nb_,
                                          None if spec is None else C.byref(spec), None if pm is None else C.byref(pm),
                                          None if pts is None else pts.ctypes.data, npts, None if out is None else out.ctypes.data, phi.ctypes.data,
                                          cls.ctypes.data, counts.ctypes.data)

    def good_spec(**kw):
        a = dict(origin=(-2.0, -2.0, -2.0), spacing=0.5, dims=(8, 8, 8), scheme=ref.CIC, quantity=nb.DEPOSIT_MASS, periodic=True, project_axis=-1)
        a.update(kw)
        return nb.grid_spec(**a)

    ok_pm = nb.pm_spec(1.0, ref.GRADIENT2)
    assert call(good_spec(), ok_pm) == nb.NBODY_OK
    bad = nb.NBODY_ERR_INVALID
    # what the three calls refuse
    assert call(None, ok_pm) == bad
    assert call(good_spec(spacing=0.0), ok_pm) == bad
    assert call(good_spec(dims=(8, 6, 8)), ok_pm) == bad              # not a power of two
    assert call(good_spec(scheme=3), ok_pm) == bad
    assert call(good_spec(project_axis=2), ok_pm) == bad              # dims there must be 1
    assert call(good_spec(periodic=False, dims=(4096, 8, 8)), ok_pm) == bad   # the padded axis exceeds NBODY_POISSON_MAX_AXIS
    s = good_spec()
    s.reserved = 1
    assert call(s, ok_pm) == bad
    assert call(good_spec(), nb.pm_spec(np.nan, ref.GRADIENT2)) == bad
    assert call(good_spec(), nb.pm_spec(1.0, ref.GRADIENT2, soften=0.1)) == bad          # periodic
    assert call(good_spec(), nb.pm_spec(1.0, ref.GRADIENT2, green=2)) == bad
    assert call(good_spec(), nb.pm_spec(1.0, ref.GRADIENT2, deconvolve=3)) == bad
    assert call(good_spec(periodic=False), nb.pm_spec(1.0, ref.GRADIENT2, green=1)) == bad
    assert call(good_spec(periodic=False), nb.pm_spec(1.0, ref.GRADIENT2, soften=-1.0)) == bad
    # the call's own
    for q in (nb.DEPOSIT_MOMENTUM_X, nb.DEPOSIT_MV2, nb.DEPOSIT_NUMBER, 6, -1):
        assert call(good_spec(quantity=q), ok_pm) == bad
    assert call(good_spec(), None) == bad
    for op in (nb.SAMPLE_VALUE, 3, -1):
        assert call(good_spec(), nb.pm_spec(1.0, op)) == bad
    for k in range(3):
        pm = nb.pm_spec(1.0, ref.GRADIENT2)
        pm.reserved[k] = 1
        assert call(good_spec(), pm) == bad
    pm = nb.pm_spec(1.0, ref.GRADIENT2)
    pm.poisson.reserved[1] = 1
    assert call(good_spec(), pm) == bad
    assert call(good_spec(), ok_pm, out=None) == bad                  # acc NULL with rows to write
    assert call(good_spec(), ok_pm, bx=None) == bad and call(good_spec(), ok_pm, bm=None) == bad
    pts = np.zeros((2, 3))
    assert call(good_spec(), ok_pm, pts=pts, npts=2 ** 31) == bad     # n_points > 2^31 - 1
    assert call(good_spec(), ok_pm, nb_=2 ** 31) == bad
    # no row to write: acc may be NULL
    assert call(good_spec(), ok_pm, pts=pts, npts=0, out=None) == nb.NBODY_OK
    assert call(good_spec(), ok_pm, bx=None, bm=None, nb_=0, out=None) == nb.NBODY_OK
    # the device calls refuse a NULL handle without touching a device
    spec = good_spec()
    assert nb.lib.nbody_pm_field(None, C.byref(spec), C.byref(ok_pm), acc.ctypes.data, None, None, n, None, None) == bad
    assert nb.lib.nbody_pm_field_at(None, C.byref(spec), C.byref(ok_pm), pts.ctypes.data, 2, acc.ctypes.data, None, None, None) == bad
    assert nb.lib.nbody_pm_field_stats(None, (C.c_uint64 * 4)()) == bad


# ------------------------------------------------------------------------------------------------ 3. zeros
@pytest.mark.parametrize("grid_name", ref.CPU_GRIDS)
def test_an_all_zero_grid_gives_plus_zero_everywhere(nb, grid_name):
    xyz, m = ref.bodies(ref.world(nb, "n65", True))
    pts = ref.caller_points(grid_name)
    for scheme, gradient in itertools.product(ref.SCHEMES, ref.GRADIENTS):
        kw = plan_of(grid_name, gradient)
        for bx, bm in ((xyz, np.zeros(len(m))), (np.zeros((0, 3)), np.zeros(0))):   # massless bodies | no body at all
            for p in ((None, pts) if len(bm) else (pts,)):
                acc, phi, cls, counts = host(nb, bx, bm, grid_name, scheme, gradient, points=p, **kw)
                for name, v in (("acc", acc), ("phi", phi)):
                    assert not v.any() and not np.signbit(v).any(), f"{grid_name} scheme {scheme} gradient {gradient}: {name}"
                assert counts[:4].sum() == len(bm)


# ------------------------------------------------------------------------------------------------ 4. momentum
def momentum_residual(nb, grid_name, scheme):
    xyz, m = ref.bodies(ref.world(nb, "w4099", True))
    acc, _, cls, _ = host(nb, xyz, m, grid_name, scheme, ref.GRADIENT2, g=1.0, green=ref.DIFF2)
    ok = cls != 3   # (the body that is not finite deposits nothing and feels nothing)
    f = m[ok, None] * acc[ok]
    return float((np.abs(f.sum(0)) / np.abs(f).sum(0)).max())


@pytest.mark.parametrize("scheme", (ref.CIC, ref.TSC))
@pytest.mark.parametrize("grid_name", ("p8x8x8", "p16x8x4"))
def test_newtons_third_law_as_the_mesh_gives_it(nb, grid_name, scheme):
    """periodic grid, one stencil both ways, the mated pair (DIFF2, GRADIENT2): sum m_i acc_i = 0 to rounding"""
    r = momentum_residual(nb, grid_name, scheme)
    print(f"momentum residual {grid_name} scheme {scheme}: {r:.3e} (measured {MEASURED_MOMENTUM[(grid_name, scheme)]:.3e})")
    assert r <= 16.0 * MEASURED_MOMENTUM[(grid_name, scheme)] < 1e-11


# ------------------------------------------------------------------------------------------------ 5. one physical anchor
def pair_residual(nb, scheme):
    origin, spacing, dims = ref.GRIDS["i32x32x32"][:3]
    xyz = np.array([[-1.6, 0.3, -0.45], [1.4, 0.3, -0.45]])   # 12 cells apart along x, neither on a cell centre nor on a face
    m = np.array([0.75, 1.5])
    g = 1.25
    acc, phi, cls, _ = nb.host_pm_field(xyz, m, origin, spacing, dims, g, scheme, ref.GRADIENT4)
    assert (cls == 0).all()
    d = xyz[1] - xyz[0]
    r = np.sqrt((d * d).sum())
    direct = np.stack([g * m[1] * d / r ** 3, -g * m[0] * d / r ** 3])
    # a body's own image pulls it nowhere on this grid to rounding: what is left is its partner's pull
    return float((np.sqrt(((acc - direct) ** 2).sum(1)) / np.sqrt((direct ** 2).sum(1))).max())


@pytest.mark.parametrize("scheme", (ref.CIC, ref.TSC))
def test_two_distant_bodies_feel_their_direct_pair_force(nb, scheme):
    r = pair_residual(nb, scheme)
    print(f"pair residual scheme {scheme}: {r:.3e} (measured {MEASURED_PAIR[scheme]:.3e})")
    assert r <= 16.0 * MEASURED_PAIR[scheme] < 0.1
