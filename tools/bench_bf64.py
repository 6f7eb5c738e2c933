"""f64 brute force: strict (k_bf_strict, the reference's loop) against fast (kernels_bf64.hip) in one process, the two
alternated per size.  Per size and mode: warm-up steps, then steps/s from a host clock around nbody_sync, then the force
kernel's time from nbody_set_profiling (HIP events around the dominant launch).  One JSON line per size.

    python tools/bench_bf64.py [--sizes 4096,16384,65536,262144] [--reps 3] [--tuning name=value,...]
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
import __graft_entry__ as graft  # noqa: E402


def steps_for(n: int, fast: bool) -> int:
    """enough steps for ~0.2 s of strict work, at least 2"""
    per_step_s = n * n * (0.3e-12 if fast else 1.2e-12)
    return max(2, min(200, int(0.2 / max(per_step_s, 1e-6))))


def measure(nb, ics, fast: bool, tuning: dict) -> dict:
    n = len(ics)
    with nb.Simulation(ics, (0.0, 0.0, 0.0), 1e6, method=nb.BRUTE_FORCE, math_mode=nb.FAST if fast else nb.STRICT, tuning=tuning) as sim:
        assert sim.config["math_mode"] == (nb.FAST if fast else nb.STRICT)
        sim.settings = nb.Settings(g=1.0, g_soft=1e-2, dt=1e-6, theta2=0.5)
        k = steps_for(n, fast)
        sim.steps(max(2, k // 4))   # warm-up
        sim.sync()
        t0 = time.perf_counter()
        sim.steps(k)
        sim.sync()
        wall = time.perf_counter() - t0
        sim.set_profiling(1)
        sim.reset_stats()
        sim.steps(k)
        sim.sync()
        st = sim.stats()
        sim.set_profiling(0)
    return dict(steps_per_s=k / wall, step_ms=1e3 * wall / k, force_kernel_ms=st.force_kernel_ms / max(1, st.force_launches),
                force_kernel_interactions=int(st.force_kernel_interactions // max(1, st.force_launches)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536,262144")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tuning", default="", help="knobs of the fast handles, name=value,...")
    a = ap.parse_args()
    nb = graft.load_package()
    tuning = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in a.tuning.split(",") if kv}
    for n in (int(s) for s in a.sizes.split(",")):
        ics = nb.plummer(n, seed=n, f64=True)
        runs = {"strict": [], "fast": []}
        for _ in range(a.reps):   # alternated: each mode sees the same clock and thermal history
            runs["strict"].append(measure(nb, ics, False, {}))
            runs["fast"].append(measure(nb, ics, True, tuning))
        best = {m: min(r, key=lambda x: x["force_kernel_ms"]) for m, r in runs.items()}
        med = {m: float(np.median([x["steps_per_s"] for x in r])) for m, r in runs.items()}
        pairs = n * (n - 1) / 2
        out = dict(n=n, tuning=tuning, reps=a.reps,
                   strict=dict(steps_per_s=med["strict"], force_kernel_ms=best["strict"]["force_kernel_ms"]),
                   fast=dict(steps_per_s=med["fast"], force_kernel_ms=best["fast"]["force_kernel_ms"],
                             force_kernel_interactions=best["fast"]["force_kernel_interactions"]),
                   speedup_steps=med["fast"] / med["strict"], speedup_force_kernel=best["strict"]["force_kernel_ms"] / best["fast"]["force_kernel_ms"],
                   fast_timed_directed_per_s=best["fast"]["force_kernel_interactions"] / (best["fast"]["force_kernel_ms"] * 1e-3),
                   strict_directed_per_s=n * (n - 1) / (best["strict"]["force_kernel_ms"] * 1e-3), unordered_pairs=pairs)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
