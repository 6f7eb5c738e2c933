#!/usr/bin/env python3
"""Leapfrog against the fourth-order Hermite step on one brute-force f64 handle pair.

  kernels  (default) both integrators step the same N bodies in fast math in THIS process, so that a kernel trace of the run
           holds k_bf64_sym and k_hm_sym side by side:
               rocprofv3 --kernel-trace --stats -- python tools/hermite_bench.py --n 65536 --steps 20
           Prints steps/s of both.
  energy   halve dt until each integrator reaches --target relative energy error over T = --t-end on hermite_ref.world(N)
           (energy_world(PAIRS) before and after); prints, per integrator, the dt, the error and the wall time of that run.

One JSON line per result on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import hermite_ref as hr  # noqa: E402


def handle(nb, rec, hermite, dt, eps):
    sim = nb.Simulation(rec, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, f64=True)
    sim.settings = nb.Settings(g=1.0, g_soft=eps, dt=dt, theta2=0.5)
    if hermite:
        sim.integrator = nb.HERMITE4
    return sim


def kernels(nb, args):
    rec = nb.plummer(args.n, seed=7, f64=True)
    for name, hermite in (("leapfrog", False), ("hermite4", True)):
        with handle(nb, rec, hermite, 1e-4, 0.01) as sim:
            sim.steps(args.warmup)
            sim.sync()
            t0 = time.perf_counter()
            sim.steps(args.steps)
            sim.sync()
            secs = time.perf_counter() - t0
            print(json.dumps(dict(mode="kernels", integrator=name, n=args.n, steps=args.steps, steps_per_s=args.steps / secs,
                                  ms_per_step=1e3 * secs / args.steps)), flush=True)


def energy(nb, args):
    x, v, m = hr.world(args.n)
    rec = hr.records(nb.PARTICLE_DTYPE64, x, v, m)
    for name, hermite in (("hermite4", True), ("leapfrog", False)):
        steps = args.first_steps
        while steps <= args.max_steps:
            with handle(nb, rec, hermite, args.t_end / steps, hr.EPS) as sim:
                e0 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
                sim.sync()
                t0 = time.perf_counter()
                sim.steps(steps)
                sim.sync()
                secs = time.perf_counter() - t0
                e1 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
            err = abs((e1 - e0) / e0)
            print(json.dumps(dict(mode="energy", integrator=name, n=args.n, steps=steps, dt=args.t_end / steps, rel_energy_error=err,
                                  wall_s=secs, reached=bool(err <= args.target))), flush=True)
            if err <= args.target:
                break
            steps *= 2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", nargs="?", default="kernels", choices=["kernels", "energy"])
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--t-end", type=float, default=1.0)
    ap.add_argument("--target", type=float, default=1e-9)
    ap.add_argument("--first-steps", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=1 << 15)
    args = ap.parse_args()
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise SystemExit("hermite_bench.py needs a HIP device")
    (kernels if args.mode == "kernels" else energy)(nb, args)


if __name__ == "__main__":
    main()
