#!/usr/bin/env python3
"""Tracers against the same particles uploaded as zero-mass bodies.

For (N bodies, M tracers) in {(2, 2^20), (1024, 2^20), (65536, 4096)} on a fast brute-force handle: ms per step of
  tracers    N bodies + M tracers (nbody_tracers_upload): N^2 + N M pair terms per step;
  zero-mass  the API without tracers: N + M bodies, the last M of mass 0: (N + M)^2 pair terms per step.
and for (65536, 2^20) on a fast Barnes-Hut handle (device build): the tracers walk the bodies' tree; as zero-mass bodies they
are sorted into it as 2^20 massless leaves.

One JSON line per row on stdout.  --routes picks a subset (the zero-mass rows at M = 2^20 take ~1e12 pairs a step)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402

BOX = ((0.0, 0.0, 0.0), 1024.0)   # nobody leaves
SHAPES = [(2, 1 << 20), (1024, 1 << 20), (65536, 4096)]
BH_SHAPE = (65536, 1 << 20)


def world(nb, n, m):
    bodies = nb.plummer(max(n, 2), seed=7)[:n].copy()
    bodies["mass"] = 1.0 / n
    tracers = nb.plummer(m, seed=8)
    tracers["position"] *= 2.0
    return bodies, tracers


def timed(sim, steps, warmup):
    sim.steps(warmup)
    sim.sync()
    t0 = time.perf_counter()
    sim.steps(steps)
    sim.sync()
    return 1e3 * (time.perf_counter() - t0) / steps


def row(nb, method, n, m, route, steps, warmup):
    bodies, tracers = world(nb, n, m)
    name = "bf" if method == nb.BRUTE_FORCE else "bh"
    extra = {}
    if route == "tracers":
        with nb.Simulation(bodies, *BOX, method=method, math_mode=nb.FAST) as sim:
            sim.settings = nb.Settings(g=1.0, g_soft=0.01, dt=1e-4, theta2=0.25)
            sim.set_tracers(tracers)
            ms = timed(sim, steps, warmup)
            pairs = n * (n - 1) + n * m if method == nb.BRUTE_FORCE else None
            plan = nb.host_tracer_plan(m, n) if method == nb.BRUTE_FORCE else None
            if pairs is None:
                accepted, visited = sim.tracer_stats()
                extra = dict(tracer_accepted_per_step=accepted // (steps + warmup), tracer_visits_per_step=visited // (steps + warmup))
    else:
        z = tracers.copy()
        z["mass"] = 0.0
        with nb.Simulation(np.concatenate([bodies, z]), *BOX, method=method, math_mode=nb.FAST) as sim:
            sim.settings = nb.Settings(g=1.0, g_soft=0.01, dt=1e-4, theta2=0.25)
            ms = timed(sim, steps, warmup)
            pairs = (n + m) * (n + m - 1) if method == nb.BRUTE_FORCE else None
            plan = None
    out = dict(method=name, n=n, m=m, route=route, steps=steps, ms_per_step=ms)
    out.update(extra)
    if pairs:
        out["pair_terms_per_step"] = pairs
        out["pair_terms_per_s"] = pairs / (ms * 1e-3)
    if plan:
        out["plan"] = plan
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--routes", default="tracers,zero-mass")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--slow-steps", type=int, default=2, help="steps of the rows with ~1e12 pair terms a step")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-bh", action="store_true")
    args = ap.parse_args()
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise SystemExit("tracer_bench.py needs a HIP device")
    for route in args.routes.split(","):
        for n, m in SHAPES:
            slow = route == "zero-mass" and m >= 1 << 20
            print(json.dumps(row(nb, nb.BRUTE_FORCE, n, m, route, args.slow_steps if slow else args.steps, 1 if slow else args.warmup)), flush=True)
        if not args.no_bh:
            print(json.dumps(row(nb, nb.BARNES_HUT, *BH_SHAPE, route, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
