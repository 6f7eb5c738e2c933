"""The static external field without a device: nbody_host_external_eval (the code nbody_external_at runs on the device, and
F = f64 of the expressions the force pass's kernel runs) against tests/external_ref.py, the restatement against calculus, the
refusals, and the agreement of the header, the ctypes mirror and the Rust shim.

(The round trip through nbody_get_external_field needs a handle, and a handle needs a device: tests/test_external_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import external_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nbody_set_external_field", "nbody_get_external_field", "nbody_external_potentials", "nbody_external_energy",
               "nbody_external_at", "nbody_host_external_eval"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def points(n, seed, spread=3.0):
    return np.random.default_rng(seed).uniform(-spread, spread, (n, 3))


# ------------------------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("name", sorted(ref.FIELDS))
@pytest.mark.parametrize("g", [1.0, 0.5])
def test_host_eval_acc_equals_the_f64_restatement_bit_for_bit(nb, name, g):
    comps = ref.FIELDS[name]
    xyz = points(300, seed=len(name))
    # on every component's centre too: the Plummer skip needs b = 0 ("point", mix8[4]), the Hernquist one r = 0
    xyz = np.concatenate([xyz, np.array([c for _, _, c in comps], np.float64)])
    acc, phi = nb.host_external_eval(ref.to_abi(nb, comps), g, xyz)
    want = ref.acc(comps, g, xyz, np.float64)
    assert np.array_equal(bits(acc), bits(want)), f"{name}: {int((bits(acc) != bits(want)).any(1).sum())} points differ"
    assert np.isfinite(acc).all()
    want_phi, mags = ref.phi(comps, g, xyz)
    assert (np.abs(phi - want_phi) <= ref.phi_bound(comps, mags)).all()
    # acc alone and phi alone are the same numbers
    only_acc, none = nb.host_external_eval(ref.to_abi(nb, comps), g, xyz, phi=False)
    assert none is None and np.array_equal(bits(only_acc), bits(acc))
    none, only_phi = nb.host_external_eval(ref.to_abi(nb, comps), g, xyz, acc=False)
    assert none is None and np.array_equal(bits(only_phi), bits(phi))


def test_the_skip_cases_are_exact_zeros(nb):
    centre = (0.5, -0.25, 0.125)
    at = np.array([centre], np.float64)
    acc, phi = nb.host_external_eval(ref.to_abi(nb, [(ref.PLUMMER, (2.0, 0.0), centre)]), 1.0, at)
    assert (acc == 0).all() and phi[0] == 0.0   # |d|^2 + b^2 == 0: the whole term is skipped
    acc, phi = nb.host_external_eval(ref.to_abi(nb, [(ref.HERNQUIST, (2.0, 0.5), centre)]), 1.0, at)
    assert (acc == 0).all() and phi[0] == -4.0   # r == 0: the acceleration is skipped, phi = -g M / a
    acc, phi = nb.host_external_eval(ref.to_abi(nb, [(ref.PLUMMER, (2.0, 0.5), centre)]), 1.0, at)
    assert (acc == 0).all() and phi[0] == -4.0   # b > 0 on the centre: evaluated, d = 0 gives zeros
    # a skipped term leaves the other components' sum alone
    both = [(ref.PLUMMER, (2.0, 0.0), centre), (ref.LOGARITHMIC, (1.0, 0.5, 0.9, 0.8), (0.0, 0.0, 0.0))]
    acc, _ = nb.host_external_eval(ref.to_abi(nb, both), 1.0, at)
    alone, _ = nb.host_external_eval(ref.to_abi(nb, both[1:]), 1.0, at)
    assert np.array_equal(bits(acc), bits(alone)) and (acc != 0).all()


def test_no_components_is_no_field_and_a_non_finite_probe_gets_nan(nb):
    xyz = points(5, seed=1)
    acc, phi = nb.host_external_eval([], 1.0, xyz)
    assert (acc == 0).all() and (phi == 0).all()
    xyz[1, 2] = np.inf
    xyz[3, 0] = np.nan
    acc, phi = nb.host_external_eval(ref.to_abi(nb, ref.FIELDS["mix8"]), 1.0, xyz)
    bad = np.array([False, True, False, True, False])
    assert np.isnan(acc[bad]).all() and np.isnan(phi[bad]).all()
    assert np.isfinite(acc[~bad]).all() and np.isfinite(phi[~bad]).all()
    clean, _ = nb.host_external_eval(ref.to_abi(nb, ref.FIELDS["mix8"]), 1.0, xyz[~bad])
    assert np.array_equal(bits(acc[~bad]), bits(clean))


# ------------------------------------------------------------------------------------- 2. acc = -grad phi
# Central differences of the f64 phi along each axis with step H.  The points lie on a grid of 2^-20 and H = 2^-13, so
# x +- H is exact.  |(phi(x + H) - phi(x - H)) / 2H + a| is at most
#     H^2 / 6 * M3          M3 >= |d^3 phi / dx_c^3| on [x - H, x + H]: the truncation of the central difference
#   + (PHI_K + 1) 2^-53 |phi| / H    each phi is within (PHI_K + 1) 2^-53 of its magnitude (external_ref.PHI_K roundings and the
#                                    sum), two of them divided by 2H: the cancellation
#   + 16 2^-53 |a|          the acceleration's own roundings (at most 13 on its longest chain)
# M3 per kind, with rho the kind's softened distance, taken H sqrt(3) closer than at the point (it moves by at most that
# much on the segment):
#   PLUMMER, and MIYAMOTO_NAGAI along x and y (A = a + B is constant there): phi = -g M / rho, rho^2 = |d|^2 + const: the
#     third derivatives of 1 / |y| are at most 15 / |y|^4                                        M3 = 15 g M / rho^4
#   HERNQUIST: radial f = -g M / (r + a); d^3/dx^3 = f''' n^3 + 3 (f''/r - f'/r^2) n (1 - n^2), n (1 - n^2) <= 0.385:
#                                        M3 = g M (6 / (r + a)^4 + 1.2 (2 / ((r + a)^3 r) + 1 / ((r + a)^2 r^2)))
#   MIYAMOTO_NAGAI along z: psi = u^-1/2, u = R^2 + A^2, A = a + B, |B'| <= 1, |B''| <= 1 / b, |B'''| <= 3 / b^2, so
#     |u'| <= 2 rho, |u''| <= 2 + 2 A / b, |u'''| <= 6 / b + 6 A / b^2 and
#     |psi'''| <= 15 / rho^4 + 9 (1 + A / b) / rho^4 + 3 (1 / b + A / b^2) / rho^3               M3 = g M times that (A + H for A)
#   LOGARITHMIC: f = ln(c + w^2) in the scaled coordinate w = d / q has |f'''| <= 12 |w| / S^2 + 16 |w|^3 / S^3 <= 28 / S^(3/2),
#     S >= rc^2:                                                                                  M3 = 14 v0^2 / (rc q)^3
H = 2.0 ** -13


def third_derivative_bound(comp, g, xyz):
    kind, p, c = comp
    p = ref.padded(p)
    d = xyz - np.array(c)
    r = np.sqrt((d * d).sum(1))
    slack = H * np.sqrt(3.0)
    out = np.zeros((len(xyz), 3))
    gm = abs(g * p[0])
    if kind == ref.PLUMMER:
        rho = np.sqrt(r * r + p[1] * p[1]) - slack
        out[:] = (15.0 * gm / rho ** 4)[:, None]
    elif kind == ref.HERNQUIST:
        rr = r - slack
        ra = rr + p[1]
        out[:] = (gm * (6.0 / ra ** 4 + 1.2 * (2.0 / (ra ** 3 * rr) + 1.0 / (ra ** 2 * rr ** 2))))[:, None]
    elif kind == ref.MIYAMOTO_NAGAI:
        a, b = p[1], p[2]
        A = a + np.sqrt(d[:, 2] ** 2 + b * b)
        rho = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + A * A) - slack
        out[:, 0] = out[:, 1] = 15.0 * gm / rho ** 4
        Ah = A + H
        out[:, 2] = gm * (15.0 / rho ** 4 + 9.0 * (1.0 + Ah / b) / rho ** 4 + 3.0 * (1.0 / b + Ah / (b * b)) / rho ** 3)
    else:
        v0, rc = p[0], p[1]
        for axis, q in enumerate((1.0, p[2], p[3])):
            out[:, axis] = 14.0 * v0 * v0 / (rc * q) ** 3
    return out


@pytest.mark.parametrize("name", ["plummer", "point", "hernquist", "mn", "mn_a0", "log"])
def test_acc_is_minus_the_gradient_of_phi(nb, name):
    comps = ref.FIELDS[name]
    g = 0.75
    xyz = np.round(points(400, seed=7 + len(name)) * 2.0 ** 20) / 2.0 ** 20
    centre = np.array(comps[0][2])
    xyz = xyz[np.sqrt(((xyz - centre) ** 2).sum(1)) >= 0.5]   # (the point mass and the Hernquist cusp: stay off the centre)
    assert len(xyz) > 300
    abi = ref.to_abi(nb, comps)
    acc, phi = nb.host_external_eval(abi, g, xyz)
    m3 = third_derivative_bound(comps[0], g, xyz)
    worst = 0.0
    for axis in range(3):
        step = np.zeros(3)
        step[axis] = H
        assert np.array_equal((xyz + step) - step, xyz)
        _, up = nb.host_external_eval(abi, g, xyz + step, acc=False)
        _, down = nb.host_external_eval(abi, g, xyz - step, acc=False)
        grad = (up - down) / (2.0 * H)
        bound = H * H / 6.0 * m3[:, axis] + (ref.PHI_K + 1) * 2.0 ** -53 * np.abs(phi) / H + 16 * 2.0 ** -53 * np.abs(acc[:, axis])
        err = np.abs(grad + acc[:, axis])
        assert (err <= bound).all(), f"{name} axis {axis}: worst ratio to the bound {float((err / bound).max())}"
        worst = max(worst, float((err / bound).max()))
    print(f"{name}: acc + grad phi, worst ratio to the bound {worst:.3g}")
    # the restatement is the same function (so the device's f32 bits are checked against calculus too)
    assert np.array_equal(bits(acc), bits(ref.acc(comps, g, xyz, np.float64)))


# ------------------------------------------------------------------------------------- 3. refusals
def bad_components(nb):
    ok = dict(plummer=(1.0, 0.1), hernquist=(1.0, 0.5), mn=(1.0, 0.5, 0.2), log=(1.0, 0.5, 0.9, 0.8))
    kind = dict(plummer=ref.PLUMMER, hernquist=ref.HERNQUIST, mn=ref.MIYAMOTO_NAGAI, log=ref.LOGARITHMIC)
    out = []

    def with_p(name, index, value):
        p = list(ref.padded(ok[name]))
        p[index] = value
        return nb.external_component(kind[name], p)

    for name in ok:
        for index in range(4):
            for value in (np.nan, np.inf, -np.inf):
                out.append((f"{name} p[{index}] = {value}", with_p(name, index, value)))
        for axis in range(3):
            centre = [0.0, 0.0, 0.0]
            centre[axis] = np.nan
            out.append((f"{name} center[{axis}] = nan", nb.external_component(kind[name], ref.padded(ok[name]), centre)))
    out += [("plummer b < 0", with_p("plummer", 1, -0.1)),
            ("hernquist a = 0", with_p("hernquist", 1, 0.0)), ("hernquist a < 0", with_p("hernquist", 1, -1.0)),
            ("mn a < 0", with_p("mn", 1, -0.5)), ("mn b = 0", with_p("mn", 2, 0.0)), ("mn b < 0", with_p("mn", 2, -0.2)),
            ("log rc = 0", with_p("log", 1, 0.0)), ("log rc < 0", with_p("log", 1, -0.5)),
            ("log qy = 0", with_p("log", 2, 0.0)), ("log qy < 0", with_p("log", 2, -0.9)),
            ("log qz = 0", with_p("log", 3, 0.0)), ("log qz < 0", with_p("log", 3, -0.8)),
            ("kind 4", nb.external_component(4, (1.0, 0.1))), ("kind -1", nb.external_component(-1, (1.0, 0.1))),
            ("reserved = 1", nb.external_component(ref.PLUMMER, (1.0, 0.1), reserved=1))]
    return out


def test_every_invalid_parameter_is_refused(nb):
    xyz = points(3, seed=2)
    good = ref.to_abi(nb, ref.FIELDS["plummer"])
    cases = bad_components(nb)
    assert len(cases) > 70
    for what, comp in cases:
        for comps in ([comp], good + [comp]):
            with pytest.raises(nb.NbodyError) as e:
                nb.host_external_eval(comps, 1.0, xyz)
            assert e.value.code == nb.NBODY_ERR_INVALID, what
            assert "nbody_host_external_eval" in str(e.value), what
    with pytest.raises(nb.NbodyError) as e:
        nb.host_external_eval(good * 9, 1.0, xyz)
    assert e.value.code == nb.NBODY_ERR_INVALID and "NBODY_EXTERNAL_MAX" in str(e.value)
    nb.host_external_eval(good * 8, 1.0, xyz)
    # the edges of the ranges are inside: b = 0 (a point mass), a = 0 (a Miyamoto-Nagai disc without a scale length)
    nb.host_external_eval(ref.to_abi(nb, [(ref.PLUMMER, (1.0, 0.0), (0, 0, 0)), (ref.MIYAMOTO_NAGAI, (1.0, 0.0, 0.2), (0, 0, 0))]), 1.0, xyz)


# ------------------------------------------------------------------------------------- 4. header, mirror and shim agree
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)


def test_header_mirror_and_rust_block_agree(nb):
    text = header_text()
    declared = set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text))
    rust = open(os.path.join(ROOT, "nbody-llm_amd", "rust", "src", "lib.rs")).read()
    block = re.search(r'unsafe extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    lib = C.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in nb.DECLARED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"fn\s+%s\s*\(" % name, block), f"{name} is missing from the Rust extern block"
    assert sorted(declared) == sorted(nb.DECLARED_SYMBOLS)
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(NBODY_EXT_[A-Z_]+)\s*=\s*(\d+)", text))
    assert enums == {"NBODY_EXT_PLUMMER": nb.EXT_PLUMMER, "NBODY_EXT_HERNQUIST": nb.EXT_HERNQUIST,
                     "NBODY_EXT_MIYAMOTO_NAGAI": nb.EXT_MIYAMOTO_NAGAI, "NBODY_EXT_LOGARITHMIC": nb.EXT_LOGARITHMIC}
    assert (ref.PLUMMER, ref.HERNQUIST, ref.MIYAMOTO_NAGAI, ref.LOGARITHMIC) == (0, 1, 2, 3)
    assert int(re.search(r"#define NBODY_EXTERNAL_MAX (\d+)", text).group(1)) == nb.EXTERNAL_MAX == 8
    for c_name, value in enums.items():
        assert re.search(r"pub const %s: i32 = %d;" % (c_name, value), rust)
    assert re.search(r"pub const NBODY_EXTERNAL_MAX: usize = 8;", rust)
    # the record: 2 x int32 + 3 + 4 doubles = 64 bytes, the same fields in the same order in all three
    assert C.sizeof(nb.NbodyExternalComponent) == 64
    body = re.search(r"typedef struct NbodyExternalComponent \{(.*?)\} NbodyExternalComponent;", text, flags=re.S).group(1)
    c_fields = [re.match(r"[\w\s]+?\s+(\w+)(\[\d+\])?$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert c_fields == [f for f, _ in nb.NbodyExternalComponent._fields_] == ["kind", "reserved", "center", "p"]
    rs_body = re.search(r"pub struct NbodyExternalComponent \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):\s*([^,\n]+)", rs_body) == [("kind", "i32"), ("reserved", "i32"), ("center", "[f64; 3]"), ("p", "[f64; 4]")]


def test_the_abi_version_stays_4(nb):
    assert nb.lib.nbody_abi_version() == 4
    assert re.search(r"#define NBODY_ABI_VERSION 4\b", header_text())


# ------------------------------------------------------------------------------------- 5. the command line
def test_cli_refuses_a_malformed_external_argument():
    import subprocess
    cli = os.path.join(ROOT, "nbody-llm_amd", "nbody_cli")
    for arg in ("bogus", "plummer", "plummer:1", "plummer:1:0.1:0:0", "mn:1:2", "log:1:2:3:4:5", "hernquist:1:x"):
        out = subprocess.run([cli, "--external", arg], capture_output=True, text=True)
        assert out.returncode == 2 and "--external" in out.stderr, arg
