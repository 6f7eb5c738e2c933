"""Times of nbody_potentials beside the calls they stand next to, one JSON line per size:

    python tools/potentials_bench.py [--sizes 65536,1048576,4194304] [--pairs-max 1048576] [--energy-max 1048576] [--mode 1|2] [--theta2 0.25]

TREE against update_forces on the same Barnes-Hut handle (fast math, device build, LEAF_DIRECT, theta2 = 0.25, eps = 1e-2),
PAIRS against nbody_energy on the same handle.  Wall time of the whole call after a warm-up call (tree build, walk / pair
kernels, read-back of the results); for kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/...`.
nbody_energy is O(N^2) with every pair twice: above --energy-max it is measured on the first `--energy-max` bodies of the
set and scaled by (N / energy-max)^2 -- marked "extrapolated" in the output.  --mode 2: the tree call in
NBODY_POTENTIAL_TREE_QUADRUPOLE, with the median |phi - phi_PAIRS| / |phi_PAIRS| beside it where PAIRS is run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576,4194304")
    ap.add_argument("--pairs-max", type=int, default=1 << 20)
    ap.add_argument("--energy-max", type=int, default=1 << 20)
    ap.add_argument("--mode", type=int, default=1, choices=(1, 2), help="the tree call's mode: 1 NBODY_POTENTIAL_TREE, 2 NBODY_POTENTIAL_TREE_QUADRUPOLE")
    ap.add_argument("--theta2", type=float, default=0.25)
    ap.add_argument("--f32-sum", action="store_true", help="tuning build: TREE alone, with the f64 and with an f32 running sum (bh_walk_debug = 2)")
    args = ap.parse_args()
    nb = graft.load_package(tuning=args.f32_sum)
    if args.f32_sum:
        for n in (int(x) for x in args.sizes.split(",")):
            with nb.Simulation(nb.plummer(n), (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE,
                               leaf_mode=nb.LEAF_DIRECT) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                out = {"n": n, "potentials_tree_f64_sum_ms": timed(lambda: sim.potentials(nb.POTENTIAL_TREE), 5)}
                sim.set_tuning("bh_walk_debug", 2)
                out["potentials_tree_f32_sum_ms"] = timed(lambda: sim.potentials(nb.POTENTIAL_TREE), 5)
            print(json.dumps(out), flush=True)
        return
    for n in (int(x) for x in args.sizes.split(",")):
        rec = nb.plummer(n)
        out = {"n": n, "mode": args.mode, "theta2": args.theta2}
        with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE,
                           leaf_mode=nb.LEAF_DIRECT) as sim:
            sim.settings = nb.Settings(1.0, 1e-2, 1e-3, args.theta2)

            def forces():
                sim.update_forces()
                sim.sync()
            out["update_forces_ms"] = timed(forces, 5)
            out["potentials_tree_ms"] = timed(lambda: sim.potentials(args.mode), 5)
            if n <= args.pairs_max:
                out["potentials_pairs_ms"] = timed(lambda: sim.potentials(nb.POTENTIAL_PAIRS), 1 if n > 200000 else 3)
                exact, phi = sim.potentials(nb.POTENTIAL_PAIRS)[0], sim.potentials(args.mode)[0]
                out["tree_median_rel_error"] = float(np.median(np.abs(phi - exact) / np.abs(exact)))
            if n <= args.energy_max:
                out["energy_ms"] = timed(sim.energy, 1 if n > 200000 else 3)
        if n > args.energy_max:
            m = args.energy_max
            with nb.Simulation(rec[:m], (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                out["energy_ms"] = timed(sim.energy, 3) * (n / m) ** 2
                out["energy_ms_extrapolated_from"] = m
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
