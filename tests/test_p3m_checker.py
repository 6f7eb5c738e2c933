"""nbody_p3m_field's definition without a device (include/nbody_hip.h, "P3M field"): nbody_host_p3m_field against the numpy
restatement (tests/p3m_ref.py) bit for bit; the split table against math.erfc and math.exp; the interpolation error; the chain walk
against an all-pairs minimum-image sum; Newton's third law of the short-range part; the force against an Ewald sum; the refusals."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import p3m_ref as ref

G = 1.25

# RMS relative force error against the Ewald sum (ref.rms_relative over the 64 bodies of ref.ewald_world: 32^3, TSC, deconvolve 2,
# GRADIENT4, SPECTRAL, r_split = 1.25 spacing, r_cut = 4.5 r_split, soften 0), as measured when the test was written; the run is
# deterministic, so the factor 1.5 asserted below is for libm differences only.  DESIGN 3.30 records the same figures.
MEASURED_EWALD_PM = 7.109e-01
MEASURED_EWALD_P3M = 1.988e-03


def cut_of(grid_name, cells=4):
    """r_split, r_cut with r_cut just under `cells` cells: the chain cell is exactly `cells` cells wide"""
    spacing = ref.GRIDS[grid_name][1]
    r_cut = cells * spacing * (1.0 - 2.0 ** -10)
    return r_cut / 3.2, r_cut


# ------------------------------------------------------------------------------------------------ 1. the same bits
@pytest.mark.parametrize("green,deconvolve", [(ref.SPECTRAL, 0), (ref.SPECTRAL, 2), (ref.DIFF2, 0), (ref.DIFF2, 2)])
@pytest.mark.parametrize("scheme,gradient", [(ref.CIC, ref.GRADIENT2), (ref.CIC, ref.GRADIENT4), (ref.TSC, ref.GRADIENT2), (ref.TSC, ref.GRADIENT4)])
def test_host_call_is_the_restatement_bit_for_bit(nb, scheme, gradient, green, deconvolve):
    grid = "p16"
    origin, spacing, dims = ref.GRIDS[grid]
    r_split, r_cut = cut_of(grid)
    T = nb.host_p3m_table(r_split, r_cut)
    xyz, m = ref.uniform_world(grid, 257, outside=True)
    xyz[5] = xyz[9]                  # coincident
    xyz[100, 1] = np.nan             # skipped
    m[33] = np.inf                   # skipped by its mass
    pts = np.concatenate([ref.uniform_world(grid, 61, seed=9, outside=True)[0], xyz[5:6], [[np.inf, 0.0, 0.0]]])
    for terms, soften, p in itertools.product((ref.BOTH, ref.MESH_ONLY, ref.SHORT_ONLY), (0.0, 0.01), (None, pts)):
        kw = dict(scheme=scheme, gradient=gradient, green=green, deconvolve=deconvolve, soften=soften, terms=terms, points=p)
        got = nb.host_p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, **kw)
        want = ref.p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, T, **kw)
        what = f"scheme {scheme} gradient {gradient} green {green} deconvolve {deconvolve} terms {terms} soften {soften} points {p is not None}"
        ref.same_bits(got[0], want[0], what + ": acc")
        ref.same_bits(got[1], want[1], what + ": phi")
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what
        assert terms == ref.MESH_ONLY or want[5] > 0, what


def test_unequal_dims_and_a_wider_chain_cell(nb):
    grid = "p16x32x64"
    origin, spacing, dims = ref.GRIDS[grid]
    r_split, r_cut = 0.4 * spacing, 1.7 * spacing          # chain cells of 2 cells: 8 x 16 x 32 of them
    T = nb.host_p3m_table(r_split, r_cut)
    xyz, m = ref.uniform_world(grid, 1500, outside=True)
    got = nb.host_p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, scheme=ref.TSC, deconvolve=2)
    want = ref.p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, T, scheme=ref.TSC, deconvolve=2)
    ref.same_bits(got[0], want[0], "acc")
    ref.same_bits(got[1], want[1], "phi")
    assert want[5] > 0


# ------------------------------------------------------------------------------------------------ 2. the table
def test_the_table_is_the_header_expression_of_libm_values(nb):
    for r_split, r_cut in ((1.0, 1.0), (0.3125, 1.40625), (0.1, 0.8)):
        got, want = nb.host_p3m_table(r_split, r_cut), ref.table(r_split, r_cut)
        rel = np.abs(got - want) / np.abs(want)
        print(f"table r_split {r_split} r_cut {r_cut}: largest relative difference {rel.max():.3e}")
        assert rel.max() <= 2.0 ** -48
        assert got[0, 0] == 1.0 and got[0, 1] == 1.0
    assert ref.SQRT_PI == math.sqrt(math.pi)


# ------------------------------------------------------------------------------------------------ 3. the interpolation
def test_linear_interpolation_stays_within_its_bound(nb):
    """|f - interpolant| <= (h^2 / 8) max |f''| on an interval; the second derivatives are first confirmed to stay below 0.35:
    F'' = (1 - x^2) exp(-x^2 / 4) / (2 sqrt(pi)) ... by central differences of the exact functions on [0, 8]"""
    xs = np.linspace(0.0, 8.0, 16001)
    d = xs[1] - xs[0]
    for f in (ref.exact_F, ref.exact_P):
        v = np.array([f(x) for x in xs])
        second = np.abs(v[2:] - 2.0 * v[1:-1] + v[:-2]) / (d * d)
        print(f"max |{f.__name__}''| on [0, 8]: {second.max():.4f}")
        assert second.max() < 0.35
    for r_split, r_cut in ((0.3125, 1.40625), (0.1, 0.8), (1.0, 1.0)):
        T = nb.host_p3m_table(r_split, r_cut)
        x_max = r_cut / r_split
        h = x_max / ref.INTERVALS
        x = np.linspace(0.0, x_max, 50001)[:-1]
        k = np.minimum((x / h).astype(np.int64), ref.INTERVALS - 1)
        fr = x / h - k
        for col, f in ((0, ref.exact_F), (1, ref.exact_P)):
            got = T[k, col] + fr * (T[k + 1, col] - T[k, col])
            err = np.abs(got - np.array([f(v) for v in x])).max()
            print(f"x_max {x_max}: column {col} error {err:.3e}, bound {(h * h / 8.0) * 0.35:.3e}")
            assert err <= (h * h / 8.0) * 0.35


# ------------------------------------------------------------------------------------------------ 4. and 5. the walk is complete
@pytest.mark.parametrize("grid", ["p16", "p32x16x16"])
@pytest.mark.parametrize("soften", [0.0, 0.02])
def test_short_only_is_the_all_pairs_minimum_image_sum(nb, grid, soften):
    origin, spacing, dims = ref.GRIDS[grid]
    r_split, r_cut = cut_of(grid)
    xyz, m = ref.face_world(grid, r_cut)
    T = nb.host_p3m_table(r_split, r_cut)
    acc, phi, _, _ = nb.host_p3m_field(xyz, m, origin, spacing, dims, G, r_split, r_cut, soften=soften, terms=ref.SHORT_ONLY)
    walk, looked, counted = ref.short_range(xyz, m, origin, spacing, dims, G, r_cut, soften, T)
    ref.same_bits(np.column_stack([acc, phi]), walk, "the host call is the restated walk")
    full, all_looked, all_counted, mag, each = ref.short_range(xyz, m, origin, spacing, dims, G, r_cut, soften, T, all_pairs=True)
    assert all_looked == len(m) * (len(m) - 1) and looked < all_looked
    assert counted == all_counted and counted > 0, f"terms with r2 < R2: the walk {counted}, all pairs {all_counted}"
    # per component: both orders add the same `terms` terms of a target, each sum with fewer than `terms` roundings of at most
    # 2^-53 sum |term| apiece: terms 2^-52 sum |term| bounds their difference, the product by g included (one term: the same bits)
    bound = each[:, None] * 2.0 ** -52 * mag
    diff = np.abs(walk - full)
    print(f"{grid} soften {soften}: {len(m)} bodies, {counted} terms, largest difference / bound {np.max(diff / np.maximum(bound, 1e-300)):.3e}")
    assert (diff <= bound).all()
    # Newton's third law: sum m_i acc_short_i = 0 to the same kind of bound
    f = m[:, None] * walk[:, :3]
    total = np.abs(f.sum(0))
    # (a pair's two terms differ by the roundings of four products each; then a target's sum, then the sum over the targets)
    limit = 2.0 ** -52 * (((each[:, None] + 4) * m[:, None] * mag[:, :3]).sum(0) + len(m) * (m[:, None] * mag[:, :3]).sum(0))
    print(f"momentum {total} against {limit}")
    assert (total <= limit).all()


# ------------------------------------------------------------------------------------------------ 6. the physics
def test_p3m_beats_pm_against_an_ewald_sum(nb):
    xyz, m = ref.ewald_world()
    want = ref.ewald_acc(xyz, m, 1.0, 6.0, 2, 12)
    finer = ref.ewald_acc(xyz, m, 1.0, 6.0, 4, 24)
    # per body, relative to that body's own force: the clump's forces are ~1e4 times the uniform bodies'
    converged = float(np.max(np.sqrt(((want - finer) ** 2).sum(1) / (finer ** 2).sum(1))))
    print(f"Ewald sum, cutoffs doubled: largest change of a body's force, relative to that force, {converged:.3e}")
    assert converged <= 1e-12
    origin, spacing, dims = (0.0, 0.0, 0.0), 1.0 / 32.0, (32, 32, 32)
    r_split = 1.25 * spacing
    r_cut = 4.5 * r_split
    pm = nb.host_pm_field(xyz, m, origin, spacing, dims, 1.0, ref.TSC, ref.GRADIENT4, periodic=True, green=ref.SPECTRAL, deconvolve=2)[0]
    p3m = nb.host_p3m_field(xyz, m, origin, spacing, dims, 1.0, r_split, r_cut, scheme=ref.TSC, gradient=ref.GRADIENT4, green=ref.SPECTRAL,
                            deconvolve=2)[0]
    e_pm, e_p3m = ref.rms_relative(pm, want), ref.rms_relative(p3m, want)
    print(f"RMS relative force error against Ewald: PM {e_pm:.3e} (measured {MEASURED_EWALD_PM:.3e}), P3M {e_p3m:.3e} (measured {MEASURED_EWALD_P3M:.3e})")
    assert e_p3m < e_pm
    assert e_p3m < 1.5 * MEASURED_EWALD_P3M


# ------------------------------------------------------------------------------------------------ 7. the refused calls
def test_refusals(nb):
    xyz, m = ref.uniform_world("p16", 65)
    n = len(m)
    acc, phi, cls, counts = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint8), np.zeros(8, np.uint64)

    def call(spec, p3m, out=acc, bx=xyz, pts=None, npts=0, nb_=n):
        return nb.lib.nbody_host_p3m_field(None if bx is None else bx.ctypes.data, m.ctypes.data, nb_, None if spec is None else C.byref(spec),
                                           None if p3m is None else C.byref(p3m), None if pts is None else pts.ctypes.data, npts,
                                           None if out is None else out.ctypes.data, phi.ctypes.data, cls.ctypes.data, counts.ctypes.data)

    def good_spec(**kw):
        a = dict(origin=(-2.0, -2.0, -2.0), spacing=0.25, dims=(16, 16, 16), scheme=ref.CIC, quantity=nb.DEPOSIT_MASS, periodic=True, project_axis=-1)
        a.update(kw)
        return nb.grid_spec(**a)

    def good(**kw):
        a = dict(g=1.0, r_split=0.3, r_cut=0.9)
        a.update(kw)
        return nb.p3m_spec(**a)

    bad = nb.NBODY_ERR_INVALID
    assert call(good_spec(), good()) == nb.NBODY_OK
    # whatever nbody_pm_field refuses
    assert call(None, good()) == bad and call(good_spec(), None) == bad
    assert call(good_spec(dims=(16, 12, 16)), good()) == bad
    assert call(good_spec(quantity=nb.DEPOSIT_NUMBER), good()) == bad
    assert call(good_spec(), good(gradient=nb.SAMPLE_VALUE)) == bad
    assert call(good_spec(), good(g=np.nan)) == bad
    assert call(good_spec(), good(deconvolve=3)) == bad
    p = good()
    p.pm.reserved[1] = 1
    assert call(good_spec(), p) == bad
    p = good()
    p.pm.poisson.soften = 0.1      # the mesh's own softening: periodic grids take none
    assert call(good_spec(), p) == bad
    # the call's own
    assert call(good_spec(periodic=False), good()) == bad
    assert call(good_spec(dims=(16, 16, 1), project_axis=2), good()) == bad
    assert call(good_spec(dims=(16, 16, 1)), good()) == bad                      # dims_c / c < 4
    assert call(good_spec(), good(r_cut=1.1, r_split=0.3)) == bad                 # c = 8 cells: 16 / 8 = 2 chain cells
    assert call(good_spec(dims=(16, 8, 16)), good()) == bad                       # c = 4: 8 / 4 = 2
    assert call(good_spec(), good(r_cut=0.999, r_split=0.3)) == nb.NBODY_OK       # c = 4: exactly 4 chain cells
    for r_split in (0.0, -0.3, np.nan, np.inf):
        assert call(good_spec(), good(r_split=r_split)) == bad
    for r_cut in (0.29, 2.41, np.nan, np.inf):                                    # below r_split, above 8 r_split
        assert call(good_spec(), good(r_cut=r_cut)) == bad
    assert call(good_spec(), good(r_split=0.3, r_cut=0.3)) == nb.NBODY_OK
    assert call(good_spec(spacing=1.0), good(r_split=0.3, r_cut=2.4)) == nb.NBODY_OK
    for soften in (-0.1, np.nan, np.inf):
        assert call(good_spec(), good(soften=soften)) == bad
    for terms in (3, -1):
        assert call(good_spec(), good(terms=terms)) == bad
    p = good()
    p.reserved = 1
    assert call(good_spec(), p) == bad
    assert call(good_spec(), good(), out=None) == bad and call(good_spec(), good(), bx=None) == bad
    pts = np.zeros((2, 3))
    assert call(good_spec(), good(), pts=pts, npts=2 ** 31) == bad and call(good_spec(), good(), nb_=2 ** 31) == bad
    assert call(good_spec(), good(), pts=pts, npts=0, out=None) == nb.NBODY_OK
    # the table
    out = np.zeros((ref.INTERVALS + 1, 2))
    assert nb.lib.nbody_host_p3m_table(0.3, 0.9, None) == bad
    for r_split, r_cut in ((0.0, 0.9), (0.3, 0.2), (0.3, 2.5), (np.nan, 0.9), (0.3, np.inf)):
        assert nb.lib.nbody_host_p3m_table(r_split, r_cut, out.ctypes.data) == bad
    # the device calls refuse a NULL handle without touching a device
    spec, p = good_spec(), good()
    assert nb.lib.nbody_p3m_field(None, C.byref(spec), C.byref(p), acc.ctypes.data, None, None, n, None, None) == bad
    assert nb.lib.nbody_p3m_field_at(None, C.byref(spec), C.byref(p), pts.ctypes.data, 2, acc.ctypes.data, None, None, None) == bad
    assert nb.lib.nbody_p3m_field_stats(None, (C.c_uint64 * 4)()) == bad


def test_the_mirror_knows_the_struct(nb):
    assert C.sizeof(nb.NbodyP3mSpec) == C.sizeof(nb.NbodyPmSpec) + 32 == 80
