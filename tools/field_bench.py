"""Times of nbody_field_at for M probes against N bodies, one JSON line per (N, M):

    python tools/field_bench.py [--bodies 65536,1048576] [--probes 4096,65536,1048576] [--pairs-max 2e11] [--mode 1|2]

Plummer sphere, f32 fast device-build handle, theta2 = 0.25, eps = 1e-2.  Wall time of the whole call after a warm-up call
(tree build, key sort, walk / pair kernels, read-back); for kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/field_bench.py ...`.  Per pair of sizes:
    tree_random_ms     TREE, uniform random probes in the bodies' bounding cube, in random order
    tree_sorted_ms     the same probes passed already in Morton order of a 2^10 grid (what the key sort buys: (b))
    pairs_ms           PAIRS at the random probes, when M x N <= --pairs-max
and with M = N (a): tree_own_ms, TREE at the bodies' own positions, beside potentials_tree_ms and update_forces_ms (the force
walk, which shares node fetches between the bodies of a lane) on the same handle.  --mode 2: every tree call in
NBODY_POTENTIAL_TREE_QUADRUPOLE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps):
    """ms per call after a warm-up call; at least `reps` calls and at least 0.3 s of them (at most 400 calls)"""
    fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(reps, min(400, int(0.3 / one) + 1))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def morton_order(p, lo, hi):
    q = np.clip(((p - lo) / (hi - lo) * 1024).astype(np.int64), 0, 1023)
    key = np.zeros(len(p), np.int64)
    for b in range(10):
        for c in range(3):
            key |= ((q[:, c] >> b) & 1) << (3 * b + c)
    return np.argsort(key, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536,1048576")
    ap.add_argument("--probes", default="4096,65536,1048576")
    ap.add_argument("--pairs-max", type=float, default=2e11)
    ap.add_argument("--mode", type=int, default=1, choices=(1, 2), help="the tree calls' mode: 1 NBODY_POTENTIAL_TREE, 2 NBODY_POTENTIAL_TREE_QUADRUPOLE")
    args = ap.parse_args()
    nb = graft.load_package()
    tree_mode = args.mode
    rng = np.random.default_rng(1)
    for n in (int(x) for x in args.bodies.split(",")):
        rec = nb.plummer(n)
        own = rec["position"].astype(np.float64)
        lo, hi = own.min(), own.max()
        with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
            sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
            def forces():
                sim.update_forces()
                sim.sync()
            out = {"n": n, "m": n, "mode": tree_mode, "update_forces_ms": timed(forces, 5), "potentials_tree_ms": timed(lambda: sim.potentials(tree_mode), 5),
                   "tree_own_ms": timed(lambda: sim.field_at(own, tree_mode), 5),
                   "tree_own_shuffled_ms": timed(lambda p=own[rng.permutation(n)]: sim.field_at(p, tree_mode), 5)}
            print(json.dumps(out), flush=True)
            for m in (int(x) for x in args.probes.split(",")):
                pts = rng.uniform(lo, hi, (m, 3))
                srt = pts[morton_order(pts, lo, hi)]
                out = {"n": n, "m": m, "mode": tree_mode, "tree_random_ms": timed(lambda: sim.field_at(pts, tree_mode), 5),
                       "tree_sorted_ms": timed(lambda: sim.field_at(srt, tree_mode), 5)}
                if float(m) * n <= args.pairs_max:
                    out["pairs_ms"] = timed(lambda: sim.field_at(pts, nb.POTENTIAL_PAIRS), 1 if float(m) * n > 1e10 else 3)
                    out["pairs_ns_per_interaction"] = out["pairs_ms"] * 1e6 / (float(m) * n)
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
