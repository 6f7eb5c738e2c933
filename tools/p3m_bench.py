"""Times of nbody_p3m_field next to nbody_pm_field on the same inputs, one JSON line per (bodies, world, call):

    python tools/p3m_bench.py [--repeats 3] [--json-out FILE]

2^18 and 2^20 bodies on an f32 handle, 128^3 periodic cells over [-4, 4]^3, TSC, SPECTRAL, deconvolve 2, GRADIENT4,
r_split = 1.25 spacing, r_cut = 4.5 r_split (chain cells of 8 cells: 16^3 of them).  Two worlds: `uniform`, and `clustered` --
three quarters uniform, one quarter in 64 Gaussian clumps of sigma 0.1 (1.6 cells), so a few chain cells hold thousands of bodies
while most hold the uniform share.  Per case: nbody_pm_field, then nbody_p3m_field under p3m_lds = 1 and 0.  Wall time of whole
calls (every call ends in a stream synchronise): one warm-up call, then --repeats calls timed one by one; reported are the median,
the spread (max - min) / median, the call's stats, and that both plans returned the same bytes.

The parent process never opens the GPU.  Each case runs ONCE, in a child process of its own under a time limit of its own; the first
child that fails, is killed by a signal or runs into its limit ends the run -- nothing more is started on the device after that.
Needs a GPU: there is no fallback.  No time is asserted anywhere."""
import argparse
import itertools
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(itertools.product((1 << 18, 1 << 20), ("uniform", "clustered")))
ORIGIN, HALF, CELLS, G = (-4.0, -4.0, -4.0), 4.0, 128, 1.0
CASE_LIMIT_S = 240


def timed(fn, repeats):
    """(median ms, spread, the last result) of `repeats` calls of fn after one warm-up call"""
    out = fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(t))
    return med, (max(t) - min(t)) / med, out


def make_world(nb, bodies, kind):
    rng = np.random.default_rng(bodies + len(kind))
    rec = nb.plummer(bodies, seed=3)
    xyz = rng.uniform(-HALF, HALF, (bodies, 3))
    if kind == "clustered":
        k = bodies // 4
        centres = rng.uniform(-HALF, HALF, (64, 3))
        xyz[:k] = centres[rng.integers(0, 64, k)] + rng.normal(0.0, 0.1, (k, 3))
    rec["position"] = xyz
    rec["mass"] = 1.0 / bodies
    return rec


def run_case(bodies, kind, repeats):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("p3m_bench needs a HIP device")
    spacing, dims = 2.0 * HALF / CELLS, (CELLS, CELLS, CELLS)
    r_split = 1.25 * spacing
    r_cut = 4.5 * r_split
    rec = make_world(nb, bodies, kind)
    kw = dict(scheme=nb.DEPOSIT_TSC, gradient=nb.SAMPLE_GRADIENT4, green=nb.POISSON_SPECTRAL, deconvolve=2)
    base = dict(bodies=bodies, world=kind, cells=CELLS, repeats=repeats)
    lines = []
    with nb.Simulation(rec, (0.0, 0.0, 0.0), 4.0e3, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        med, spread, _ = timed(lambda: sim.pm_field(ORIGIN, spacing, dims, G, periodic=True, **kw), repeats)
        lines.append(dict(base, call="pm_field", ms=med, spread=spread))
        outs = []
        for lds in (1, 0):
            sim.set_tuning("p3m_lds", lds)
            med, spread, got = timed(lambda: sim.p3m_field(ORIGIN, spacing, dims, G, r_split, r_cut, **kw), repeats)
            outs.append(got)
            lines.append(dict(base, call="p3m_field", p3m_lds=lds, ms=med, spread=spread, ratio_to_pm_field=med / lines[0]["ms"],
                              stats=[int(v) for v in sim.p3m_field_stats()]))
        lines[-1]["same_bytes_under_both_plans"] = all(a.tobytes() == b.tobytes() for a, b in zip(outs[0], outs[1]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json-out")
    ap.add_argument("--case", type=int, default=-1, help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.case >= 0:
        for line in run_case(*CASES[args.case], args.repeats):
            print(json.dumps(line), flush=True)
        return 0
    out = open(args.json_out, "w") if args.json_out else None
    for k in range(len(CASES)):
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(k), "--repeats", str(args.repeats)], capture_output=True,
                                 text=True, timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"case {CASES[k]} ran into its limit of {CASE_LIMIT_S} s: nothing more is started", file=sys.stderr)
            return 124
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if out:
            out.write(run.stdout)
            out.flush()
        if run.returncode != 0:
            print(f"case {CASES[k]} ended with status {run.returncode}: nothing more is started\n{run.stderr}", file=sys.stderr)
            return run.returncode if run.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
