"""tests/hermite_block_ref.py, the numpy restatement of a Hermite handle's block individual time steps, checked on the CPU:
the scheme's invariants, the shared step as its eta -> infinity limit, the work-for-accuracy table the feature was proposed
with, the sensitivity of the per-row bounds to a dropped partner, and the mirror's declarations."""
import os
import re

import numpy as np
import pytest

import hermite_block_ref as br
import hermite_ref as hr

G_SOFT = 0.005
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def eq(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_every_macro_step_ends_at_T_and_no_step_doubles_off_its_grid():
    x, v, m = br.tight_pair_world(48)
    h = br.Handle(x, v, m, 0.02, 6, eps=G_SOFT)
    for dt in (1 / 16, 1 / 16, -1 / 16, 1 / 32):
        h.step_by(dt)
    log = h.log
    assert log["all_at_T"] and log["off_grid"] == 0
    assert h.levels.max() >= 3 and h.levels.min() == 0, "the tight pair must sit levels below the field bodies"
    assert log["block_steps"] > 4 and log["updates"] < log["block_steps"] * 48
    assert h.interactions == 48 * 47 + log["pair_terms"] and h.steps == 4 and h.elapsed == 1 / 16 + 1 / 32


def test_huge_eta_is_the_shared_step_bit_for_bit():
    x, v, m = br.tight_pair_world(40)
    h = br.Handle(x, v, m, 1e30, 6, eps=G_SOFT)
    ref = hr.start(x, v, m, eps=G_SOFT)
    for dt in (1 / 64, 1 / 64, -1 / 128):
        h.step_by(dt)
        ref = hr.hermite_step(ref, dt, eps=G_SOFT)
        assert not h.levels.any()
        assert all(eq(a, b) for a, b in zip(h.state, ref))
    assert h.log["block_steps"] == 3 and h.log["updates"] == 120


def test_strict_rows_is_strict_aj_on_any_row_list():
    x, v, m = hr.world(70)
    a, j = hr.strict_aj(x, v, m, hr.G, hr.EPS)
    rows = np.random.default_rng(3).permutation(70)[:33]
    ra, rj = br.strict_rows(x, v, m, hr.G, hr.EPS, rows)
    assert eq(ra, a[rows]) and eq(rj, j[rows])


#: the table of the proposal: run -> (directed pair terms, relative energy error over T = 1); n = 64, g_soft 0.005, macro
#: step 1/16, 8 levels, eta 0.02, bodies 0 and 1 a bound pair at separation 0.02
TABLE = {"block": (6.05e5, 2.1e-6), 4: (1.03e6, 0.20), 6: (4.13e6, 5.9e-4), 7: (8.26e6, 1.9e-5), 8: (1.65e7, 6.1e-7)}


@pytest.mark.parametrize("run", list(TABLE), ids=[str(k) for k in TABLE])
def test_the_restatement_reproduces_the_proposals_table(run):
    x, v, m = br.tight_pair_world(64)
    terms, err = TABLE[run]
    if run == "block":
        h = br.Handle(x, v, m, 0.02, 8, eps=G_SOFT, force=br.fast_rows)
        h.update_forces()
        e0 = br.energy(h.state, hr.G, G_SOFT)
        for _ in range(16):
            h.step_by(1 / 16)
        got_terms, got_err = h.log["pair_terms"], abs((br.energy(h.state, hr.G, G_SOFT) - e0) / e0)
        assert h.log["all_at_T"] and h.log["off_grid"] == 0
    else:
        st = hr.start(x, v, m, eps=G_SOFT, force=hr.fast_aj)
        e0 = br.energy(st, hr.G, G_SOFT)
        steps = 16 << run
        for _ in range(steps):
            st = hr.hermite_step(st, 1 / steps, eps=G_SOFT, force=hr.fast_aj)
        got_terms, got_err = steps * 64 * 63, abs((br.energy(st, hr.G, G_SOFT) - e0) / e0)
    print(f"\n[hermite block table] {run}: pair terms {got_terms:.3e} (table {terms:.3e}), energy error {got_err:.3e} (table {err:.3e})")
    assert terms / 2 <= got_terms <= terms * 2
    assert err / 10 <= got_err <= err * 10


def test_a_dropped_partner_breaks_the_row_bounds():
    x, v, m = hr.world(257)
    rows = np.arange(0, 257, 5)
    Sa, Ta, Sj, Tj = hr.direct_aj(x, v, m, hr.G, hr.EPS, rows)

    def worst(a, j):
        ea = np.abs(a - Sa).max(1) / Ta
        ej = np.abs(j - Sj).max(1) / Tj
        return float(ea.max()), float(ej.max())

    a, j = br.strict_rows(x, v, m, hr.G, hr.EPS, rows)
    ea, ej = worst(a, j)
    assert ea <= hr.R and ej <= hr.RJ
    m2 = m.copy()
    m2[200] = 0.0                                 # partner 200 dropped from every row's sum
    a, j = br.strict_rows(x, v, m2, hr.G, hr.EPS, rows)
    ea, ej = worst(a, j)
    assert ea > hr.R and ej > hr.RJ


def test_the_mirror_and_the_header_declare_the_entry_points():
    names = ["nbody_set_block_steps", "nbody_get_block_steps", "nbody_download_levels", "nbody_block_step_counts",
             "nbody_debug_hermite_forces_of"]
    with open(os.path.join(ROOT, "nbody-llm_amd", "__init__.py")) as f:
        mirror = f.read()
    with open(os.path.join(ROOT, "include", "nbody_hip.h")) as f:
        header = f.read()
    declared = mirror[mirror.index("DECLARED_SYMBOLS"):mirror.index("class NbodyConfig")]
    for name in names:
        assert f'"{name}"' in declared, name
        assert re.search(rf'_sig\("{name}"', mirror), name
        assert re.search(rf"\bint {name}\(", header), name
    assert "#define NBODY_ABI_VERSION 4" in header
