"""Steps per second under mesh gravity against one nbody_pm_field call per step, one JSON line per (bodies, grid,
boundary condition, plan):

    python tools/mesh_bench.py [--repeats 5] [--steps 20] [--json-out FILE]

65 536 and 1 048 576 Plummer bodies on an f32 handle, 64^3 and 128^3 cells over [-4, 4]^3, periodic (DIFF2) and isolated, CIC,
GRADIENT2.  Per case, on one handle:
    pm_field   one nbody_pm_field call (acc only) per step -- what a caller had before mesh gravity, without the host kick and the
               upload that it also paid: the time of that call alone, so the comparison flatters the older path
    mesh       nbody_steps(--steps) under nbody_set_mesh_gravity and one nbody_count to drain the stream, under the four plans
               mesh_kick_fuse x mesh_keep_kernel
Wall time: one warm-up round, then --repeats rounds timed one by one; reported are the median per step, the spread (max - min) /
median, the stats words, and that every plan left the same bytes after the same number of steps.

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
CASES = list(itertools.product((1 << 16, 1 << 20), (64, 128), (True, False)))
ORIGIN, HALF = (-4.0, -4.0, -4.0), 4.0
CASE_LIMIT_S = 240
PLANS = [(1, 1), (0, 1), (1, 0), (0, 0)]   # (mesh_kick_fuse, mesh_keep_kernel)
KNOBS = ("mesh_kick_fuse", "mesh_keep_kernel")


def timed(fn, repeats):
    """(median ms, spread) of `repeats` calls of fn after one warm-up call"""
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(t))
    return med, (max(t) - min(t)) / med


def run_case(bodies, cells, periodic, steps, repeats):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("mesh_bench needs a HIP device")
    spacing, dims = 2.0 * HALF / cells, (cells, cells, cells)
    green = nb.POISSON_DIFF2 if periodic else 0
    rec = nb.plummer(bodies, seed=3)
    mesh = dict(origin=ORIGIN, spacing=spacing, dims=dims, scheme=nb.DEPOSIT_CIC, gradient=nb.SAMPLE_GRADIENT2, periodic=periodic, green=green)
    base = dict(bodies=bodies, cells=cells, periodic=periodic, steps=steps, repeats=repeats)
    lines = []

    def make():
        sim = nb.Simulation(rec, (0.0, 0.0, 0.0), 4.0e3, method=nb.BRUTE_FORCE, math_mode=nb.FAST)
        sim.settings = nb.Settings(g=1.0, g_soft=0.05, dt=1.0 / 1024, theta2=0.5)
        sim.init()
        return sim

    with make() as sim:
        def calls():
            for _ in range(steps):
                sim.pm_field(ORIGIN, spacing, dims, 1.0, nb.DEPOSIT_CIC, nb.SAMPLE_GRADIENT2, periodic, green, phi=False)
        med, spread = timed(calls, repeats)
        lines.append(dict(base, call="pm_field", ms_per_step=med / steps, steps_per_s=1e3 * steps / med, spread=spread))
    want = None
    for plan in PLANS:
        with make() as sim:
            for knob, v in zip(KNOBS, plan):
                sim.set_tuning(knob, v)
            sim.mesh_gravity = mesh

            def run():
                sim.steps(steps)
                len(sim)   # (one read-back of the count: the stream is drained)
            med, spread = timed(run, repeats)
            got = sim.get_points().tobytes()
            want = got if want is None else want
            lines.append(dict(base, call="mesh", plan=dict(zip(KNOBS, plan)), ms_per_step=med / steps, steps_per_s=1e3 * steps / med, spread=spread,
                              ratio_to_pm_field=(med / steps) / lines[0]["ms_per_step"], stats=[int(v) for v in sim.mesh_gravity_stats()],
                              same_bytes_as_first_plan=got == want))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json-out")
    ap.add_argument("--case", type=int, default=-1, help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.case >= 0:
        for line in run_case(*CASES[args.case], args.steps, args.repeats):
            print(json.dumps(line), flush=True)
        return 0
    out = open(args.json_out, "w") if args.json_out else None
    for k in range(len(CASES)):
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(k), "--repeats", str(args.repeats), "--steps", str(args.steps)],
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
