"""tests/mesh_ref.py checked on the CPU: with g = 0 and no field its loop IS external_ref.leapfrog_orbits' leapfrog, bit for bit,
on a world whose walls drop bodies; the body that is not finite leaves at the first retain; the tracers ride in the bodies' field;
the structs' sizes and what the Python mirror refuses without a device."""
import ctypes as C

import numpy as np
import pytest

import external_ref
import mesh_ref
import pm_ref as ref

DTS = (1.0 / 64, 1.0 / 32, 1.0 / 128, 3.0 / 256)


@pytest.mark.parametrize("grid,scheme,gradient", [("p8x8x8", ref.CIC, ref.GRADIENT2), ("i8x4x2", ref.TSC, ref.GRADIENT4), ("p16x8x4", ref.NGP, ref.GRADIENT2)])
def test_without_gravity_the_loop_is_the_leapfrog_of_the_external_restatement(nb, grid, scheme, gradient):
    rec = ref.world(nb, "n65", False)
    rec["velocity"] *= np.float32(40.0)   # fast enough to reach the walls within four steps
    lo, hi = -1.0, 1.0
    got = mesh_ref.step(nb, rec, DTS, lo, hi, 0.0, grid, scheme, gradient)
    want = external_ref.leapfrog_orbits([], 0.0, rec, DTS, lo, hi)
    assert 0 < len(want) < len(rec) - 1, "the walls must drop more than the body that is not finite"
    assert len(got) == len(want)
    for f in ("position", "velocity", "acceleration", "mass"):
        assert got[f].tobytes() == want[f].tobytes(), f
    assert not got["acceleration"].any() and not np.signbit(got["acceleration"]).any()   # g = 0: every acceleration is +0.0


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_body_that_is_not_finite_leaves_at_the_first_retain(nb, f64):
    rec = ref.world(nb, "n65", f64)
    assert np.isnan(rec["position"]).any()
    one = mesh_ref.step(nb, rec, DTS[:1], -2000.0, 2000.0, 1.25, "p8x8x8", ref.CIC, ref.GRADIENT2)
    assert len(one) == len(rec) - 1 and np.isfinite(one["position"]).all() and one["position"].dtype == rec["position"].dtype
    assert one["acceleration"].any(), "g != 0: the mesh pulls"
    # the kick is the rounded host field at the half-drifted positions, one conversion to the records' dtype
    F = rec["position"].dtype.type
    live = rec[np.isfinite(rec["position"]).all(axis=1)]
    x = live["position"] + (live["velocity"] * F(0.5)) * F(DTS[0])
    origin, spacing, dims, periodic, axis = ref.GRIDS["p8x8x8"]
    acc = nb.host_pm_field(x.astype(np.float64), live["mass"].astype(np.float64), origin, spacing, dims, float(F(1.25)), ref.CIC, ref.GRADIENT2, periodic,
                           phi=False)[0]
    assert one["acceleration"].tobytes() == acc.astype(rec["position"].dtype).tobytes()
    assert one["velocity"].tobytes() == (live["velocity"] + acc.astype(rec["position"].dtype) * F(DTS[0])).tobytes()


def test_tracers_ride_in_the_bodies_field_and_add_nothing_to_it(nb):
    rec = ref.world(nb, "n65", False)
    tracers = np.zeros(9, nb.PARTICLE_DTYPE)
    tracers["position"] = ref.caller_points("p8x8x8", 97, seed=1)[:9].astype(np.float32)   # (the sixth is far away and leaves)
    alone = mesh_ref.step(nb, rec, DTS[:2], -2.0, 2.0, 1.25, "p8x8x8", ref.TSC, ref.GRADIENT2)
    both, tr = mesh_ref.step(nb, rec, DTS[:2], -2.0, 2.0, 1.25, "p8x8x8", ref.TSC, ref.GRADIENT2, tracers=tracers)
    assert both.tobytes() == alone.tobytes()
    assert 0 < len(tr) <= 9 and tr["acceleration"].any() and not tr["mass"].any()
    # with an external field on top: the sum, in the records' precision
    comps = external_ref.FIELDS["plummer"]
    with_ext = mesh_ref.step(nb, rec, DTS[:1], -2.0, 2.0, 1.25, "p8x8x8", ref.TSC, ref.GRADIENT2, ext=comps)
    plain = mesh_ref.step(nb, rec, DTS[:1], -2.0, 2.0, 1.25, "p8x8x8", ref.TSC, ref.GRADIENT2)
    x = plain["position"] - (plain["velocity"] * np.float32(0.5)) * np.float32(DTS[0])   # (not bit-exact: only used to see that the field differs)
    assert len(with_ext) == len(plain) and with_ext["acceleration"].tobytes() != plain["acceleration"].tobytes() and len(x) == len(plain)


def test_struct_sizes_and_the_mirror_s_refusals_without_a_device(nb):
    assert C.sizeof(nb.GridSpec) == 64 and C.sizeof(nb.NbodyPmSpec) == 48 and C.sizeof(nb.NbodyPoissonSpec) == 32
    spec, pm = nb.mesh_gravity_specs(dict(origin=(-2, -2, -2), spacing=0.5, dims=(8, 8, 8), periodic=True, gradient=nb.SAMPLE_GRADIENT4, g=3.0))
    assert isinstance(spec, nb.GridSpec) and isinstance(pm, nb.NbodyPmSpec)
    assert spec.quantity == nb.DEPOSIT_MASS and spec.periodic == 1 and list(spec.dims) == [8, 8, 8] and pm.gradient == nb.SAMPLE_GRADIENT4 and pm.poisson.g == 3.0
    assert nb.mesh_gravity_specs((spec, pm)) == (spec, pm)
    with pytest.raises(ValueError, match="unknown keys"):
        nb.mesh_gravity_specs(dict(origin=(0, 0, 0), spacing=1.0, dims=(8, 8, 8), sofen=0.1))
    with pytest.raises(ValueError, match="missing keys"):
        nb.mesh_gravity_specs(dict(origin=(0, 0, 0), spacing=1.0))
    for bad in (5, (spec,), (spec, spec), (pm, spec), "mesh"):
        with pytest.raises(TypeError):
            nb.mesh_gravity_specs(bad)
    # a NULL handle is refused without touching a device
    out = (C.c_uint64 * 4)()
    on = C.c_int(0)
    assert nb.lib.nbody_set_mesh_gravity(None, C.byref(spec), C.byref(pm)) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_get_mesh_gravity(None, C.byref(spec), C.byref(pm), C.byref(on)) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_mesh_gravity_stats(None, out) == nb.NBODY_ERR_INVALID
