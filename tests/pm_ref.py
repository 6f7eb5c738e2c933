"""nbody_pm_field restated (include/nbody_hip.h, "particle-mesh field"; csrc/pm_grid.h): the composition of the three numpy
restatements -- deposit_ref.deposit, poisson_ref.solve, sample_ref.sample -- and one negation.  Nothing is restated a second time
here.  Also the grids and worlds of tests/test_pm_checker.py and test_pm_gpu.py."""
import numpy as np

import deposit_ref
import poisson_ref
import sample_ref

NGP, CIC, TSC = 0, 1, 2
GRADIENT2, GRADIENT4 = sample_ref.GRADIENT2, sample_ref.GRADIENT4
SPECTRAL, DIFF2 = poisson_ref.SPECTRAL, poisson_ref.DIFF2
SCHEMES = (NGP, CIC, TSC)
GRADIENTS = (GRADIENT2, GRADIENT4)

#: name -> (origin, spacing, dims, periodic, project_axis); every world below lies mostly inside [-2, 2]^3
GRIDS = {
    "p8x8x8": ((-2.0, -2.0, -2.0), 0.5, (8, 8, 8), True, -1),
    "p16x8x4": ((-2.0, -2.0, -2.0), 0.25, (16, 8, 4), True, -1),
    "i8x4x2": ((-1.0, -0.5, -0.25), 0.25, (8, 4, 2), False, -1),       # most bodies are off it
    "i16x16x1_z": ((-2.0, -2.0, 0.0), 0.25, (16, 16, 1), False, 2),
    "i32x32x32": ((-4.0, -4.0, -4.0), 0.25, (32, 32, 32), False, -1),  # (the GPU tests' extra shape)
    "p32x32x32": ((-4.0, -4.0, -4.0), 0.25, (32, 32, 32), True, -1),
    "p1x8x8_x": ((0.0, -2.0, -2.0), 0.5, (1, 8, 8), True, 0),          # the ignored axis is x, then y: the GPU tests run these
    "i1x8x8_x": ((0.0, -2.0, -2.0), 0.5, (1, 8, 8), False, 0),         # four under AXIS_WORLD
    "p8x1x8_y": ((-2.0, 0.0, -2.0), 0.5, (8, 1, 8), True, 1),
    "i8x1x8_y": ((-2.0, 0.0, -2.0), 0.5, (8, 1, 8), False, 1),
}
CPU_GRIDS = ("p8x8x8", "p16x8x4", "i8x4x2", "i16x16x1_z")
AXIS_GRIDS = ("p1x8x8_x", "i1x8x8_x", "p8x1x8_y", "i8x1x8_y")
AXIS_WORLD = "u300"
WORLDS = ("n1", "n65", "w4099")


def world(nb, name, f64):
    """The records of a world, in the handle's dtype: unequal masses, some bodies off a non-periodic grid (a Plummer sphere reaches
    well past [-2, 2]^3) and, from 65 bodies on, one body that is not finite.  u300 (AXIS_WORLD): 300 bodies uniform in +-2.3 on every
    axis, which straddles the faces of AXIS_GRIDS at +-2, with every 25th body moved 3.5 to 6 away from the centre on every axis:
    off an isolated grid with its whole stencil, whatever the scheme."""
    n = {"n1": 1, "n63": 63, "n64": 64, "n65": 65, "n257": 257, "u300": 300, "w4099": 4099}[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    rec = nb.plummer(n, seed=17, f64=f64)
    rec["mass"] = rec["mass"] * rng.uniform(0.5, 1.5, n)
    if name == AXIS_WORLD:
        xyz = rng.uniform(-2.3, 2.3, (n, 3))
        xyz[::25] = rng.uniform(3.5, 6.0, (len(xyz[::25]), 3)) * rng.choice((-1.0, 1.0), (len(xyz[::25]), 3))
        rec["position"] = xyz
    if n >= 65:
        rec["position"][n // 2, 1] = np.nan
        rec["position"][3] = (9.0, -7.5, 0.25)   # off every grid here that is not periodic
    return rec


def bodies(rec):
    """(xyz [n][3], mass [n]) as f64"""
    return np.ascontiguousarray(rec["position"], np.float64).reshape(-1, 3), np.ascontiguousarray(rec["mass"], np.float64).reshape(-1)


def caller_points(grid_name, m=97, seed=5):
    """m points around the grid, a few of them off it and one not finite"""
    origin, spacing, dims, _, _ = GRIDS[grid_name]
    rng = np.random.default_rng(seed + sum(map(ord, grid_name)))
    lo = np.array(origin)
    hi = lo + spacing * np.array(dims)
    xyz = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (m, 3))
    xyz[5] = (1.0e6, 0.0, 0.0)
    xyz[11, 2] = np.inf
    return xyz


def pm_field(body_xyz, body_m, origin, spacing, dims, g, scheme, gradient, periodic=False, green=SPECTRAL, soften=0.0, deconvolve=0,
             project_axis=-1, points=None, parts=False):
    """(acc [n][3], phi [n], cls [n] uint8, counts [8] uint64); parts: also the mass grid and the potential grid"""
    body_xyz = np.asarray(body_xyz, np.float64).reshape(-1, 3)
    mass, c_dep = deposit_ref.deposit(body_xyz, body_m, origin, spacing, dims, scheme, periodic, project_axis)
    pot = poisson_ref.solve(mass, spacing, g, periodic, green, soften, deconvolve, scheme)
    p = body_xyz if points is None else np.asarray(points, np.float64).reshape(-1, 3)
    grad, cls, c_smp = sample_ref.sample(p, pot, origin, spacing, scheme, gradient, periodic, project_axis)
    acc = 0.0 - grad
    phi = sample_ref.sample(p, pot, origin, spacing, scheme, sample_ref.VALUE, periodic, project_axis)[0][:, 0]
    counts = np.concatenate([c_dep, c_smp]).astype(np.uint64)
    return (acc, phi, cls, counts, mass, pot) if parts else (acc, phi, cls, counts)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        r = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first {r}: {got[r]!r} vs {want[r]!r}")
