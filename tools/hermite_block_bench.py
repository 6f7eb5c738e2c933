#!/usr/bin/env python3
"""Block individual time steps against the shared Hermite step on one brute-force f64 handle.

hermite_ref.world(N) with --pairs tight pairs (separation 0.02, g_soft 0.005) runs over T = --t-end in fast math:
  block   macro steps of --macro with --levels levels and --eta (nbody_set_block_steps)
  shared  the shared step, halved from --macro until its relative energy error (energy_world(PAIRS) before and after) is no
          larger than the block run's (at most --max-halvings times)
and prints, per run, one JSON line: block steps, body updates, directed pair terms (NbodyStats.interactions), relative
energy error and wall time.  `--only block` or `--only shared --shared-level K` run one side alone (the shared side also
runs on a commit that has no block steps), e.g. for the per-kernel split:
    rocprofv3 --kernel-trace --stats -- python tools/hermite_block_bench.py --only block
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hermite_ref as hr  # noqa: E402

G_SOFT = 0.005


def world(n, pairs, sep=0.02):
    """hermite_ref.world(n) with bodies (2k, 2k + 1), k < pairs, made bound pairs (tests/hermite_block_ref.tight_pair_world's rule)."""
    x, v, m = hr.world(n)
    for k in range(pairs):
        i, j = 2 * k, 2 * k + 1
        M = m[i] + m[j]
        c, u = x[i].copy(), v[i].copy()
        vrel = np.sqrt(hr.G * M / sep)
        x[i], x[j] = c + np.array([sep * m[j] / M, 0, 0]), c - np.array([sep * m[i] / M, 0, 0])
        v[i], v[j] = u + np.array([0, vrel * m[j] / M, 0]), u - np.array([0, vrel * m[i] / M, 0])
    return x, v, m


def run(nb, rec, dt, steps, block):
    with nb.Simulation(rec, *hr.BOX, method=nb.BRUTE_FORCE, math_mode=nb.FAST, f64=True) as sim:
        sim.settings = nb.Settings(g=hr.G, g_soft=G_SOFT, dt=dt, theta2=0.5)
        sim.integrator = nb.HERMITE4
        if block:
            sim.block_steps = block
        e0 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
        sim.update_forces()
        sim.sync()
        t0 = time.perf_counter()
        sim.steps(steps)
        sim.sync()
        secs = time.perf_counter() - t0
        e1 = sum(sim.energy_world(nb.POTENTIAL_PAIRS))
        counts = sim.block_step_counts() if block else (steps, steps * len(rec))
        return dict(dt=dt, steps=steps, block_steps=counts[0], body_updates=counts[1], pair_terms=int(sim.stats().interactions),
                    rel_energy_error=abs((e1 - e0) / e0), seconds=secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--t-end", type=float, default=1.0)
    ap.add_argument("--macro", type=float, default=1 / 16)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--eta", type=float, default=0.02)
    ap.add_argument("--only", choices=["block", "shared"])
    ap.add_argument("--shared-level", type=int, default=6)
    ap.add_argument("--max-halvings", type=int, default=9)
    args = ap.parse_args()
    import __graft_entry__ as graft
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise SystemExit("hermite_block_bench.py needs a HIP device")
    rec = hr.records(nb.PARTICLE_DTYPE64, *world(args.n, args.pairs))
    macros = round(args.t_end / args.macro)
    target = None
    if args.only != "shared":
        r = run(nb, rec, args.macro, macros, (args.eta, args.levels))
        target = r["rel_energy_error"]
        print(json.dumps(dict(mode="block", n=args.n, pairs=args.pairs, eta=args.eta, levels=args.levels, **r)), flush=True)
    if args.only == "shared":
        k = args.shared_level
        print(json.dumps(dict(mode="shared", n=args.n, pairs=args.pairs, level=k, **run(nb, rec, args.macro / (1 << k), macros << k, None))), flush=True)
    elif args.only is None:
        for k in range(args.max_halvings + 1):
            r = run(nb, rec, args.macro / (1 << k), macros << k, None)
            print(json.dumps(dict(mode="shared", n=args.n, pairs=args.pairs, level=k, **r)), flush=True)
            if r["rel_energy_error"] <= target:
                break


if __name__ == "__main__":
    main()
