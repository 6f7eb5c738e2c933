"""Times of nbody_pm_field against the three-call composition on the same handle, one JSON line per (grid,
boundary condition, scheme, plan):

    python tools/pm_bench.py [--repeats 5] [--bodies 1048576] [--json-out FILE]

2^20 Plummer bodies on an f32 handle, 64^3 and 128^3 cells over [-4, 4]^3, periodic (DIFF2, GRADIENT2) and isolated (GRADIENT2), CIC
and TSC.  Per case: the composition deposit -> grid_poisson -> grid_sample(gradient) -> grid_sample(value) through the Python
mirror, then nbody_pm_field under the four plans pm_gather x pm_share_sort and, on the default plan, with deposit_sort =
sample_sort = 0 and with poisson_lds = 0.  Wall time of whole calls (every call ends in a stream synchronise): one warm-up call,
then --repeats calls timed one by one; reported are the median, the spread (max - min) / median, the call's stats, and that every
plan and the composition returned the same bytes.  The composition's time includes what the mirror does between its calls (three
numpy grids allocated): that is part of what a caller of the three calls pays.

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
CASES = [(cells, periodic, scheme) for cells, periodic, scheme in itertools.product((64, 128), (True, False), (1, 2))]
ORIGIN, HALF, G = (-4.0, -4.0, -4.0), 4.0, 1.0
CASE_LIMIT_S = 240
# (pm_gather, pm_share_sort, deposit_sort, sample_sort, poisson_lds)
PLANS = [(1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (0, 1, 1, 1, 1), (0, 0, 1, 1, 1), (1, 1, 0, 0, 1), (1, 1, 1, 1, 0)]
KNOBS = ("pm_gather", "pm_share_sort", "deposit_sort", "sample_sort", "poisson_lds")


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


def run_case(cells, periodic, scheme, bodies, repeats):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("pm_bench needs a HIP device")
    spacing, dims = 2.0 * HALF / cells, (cells, cells, cells)
    green = nb.POISSON_DIFF2 if periodic else 0
    rec = nb.plummer(bodies, seed=3)
    with nb.Simulation(rec, (0.0, 0.0, 0.0), 4.0e3, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        def composition():
            mass, c_dep = sim.deposit(ORIGIN, spacing, dims, scheme=scheme, periodic=periodic)
            pot = sim.grid_poisson(mass, spacing, G, periodic, green, 0.0, 0, scheme)
            grad, cls, c_smp = sim.grid_sample(pot, ORIGIN, spacing, scheme=scheme, op=nb.SAMPLE_GRADIENT2, periodic=periodic)
            val = sim.grid_sample(pot, ORIGIN, spacing, scheme=scheme, op=nb.SAMPLE_VALUE, periodic=periodic)[0][:, 0]
            return 0.0 - grad, val, cls, np.concatenate([c_dep, c_smp])

        def fused():
            return sim.pm_field(ORIGIN, spacing, dims, G, scheme, nb.SAMPLE_GRADIENT2, periodic, green)

        base = dict(cells=cells, periodic=periodic, scheme=scheme, bodies=bodies, repeats=repeats)
        med, spread, want = timed(composition, repeats)
        lines = [dict(base, call="composition", ms=med, spread=spread)]
        for plan in PLANS:
            for knob, v in zip(KNOBS, plan):
                sim.set_tuning(knob, v)
            med, spread, got = timed(fused, repeats)
            same = all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
            lines.append(dict(base, call="pm_field", plan=dict(zip(KNOBS, plan)), ms=med, spread=spread, ratio_to_composition=med / lines[0]["ms"],
                              stats=[int(v) for v in sim.pm_field_stats()], same_bytes_as_composition=same))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bodies", type=int, default=1 << 20)
    ap.add_argument("--json-out")
    ap.add_argument("--case", type=int, default=-1, help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.case >= 0:
        for line in run_case(*CASES[args.case], args.bodies, args.repeats):
            print(json.dumps(line), flush=True)
        return 0
    out = open(args.json_out, "w") if args.json_out else None
    for k in range(len(CASES)):
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(k), "--repeats", str(args.repeats), "--bodies", str(args.bodies)],
                                 capture_output=True, text=True, timeout=CASE_LIMIT_S)
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
