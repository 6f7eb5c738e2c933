#!/usr/bin/env python3
"""Quadrupole walk (nbody_set_multipole(h, 2)) beside the monopole walks: kernel launches for a trace, error against the
direct sum, steps per second.

  trace N        -- device build, NBODY_LEAF_DIRECT, Plummer N bodies: for theta2 in 0.25, 1.0 three force passes each of
                    order 1 with bh_walk_duo = 0, order 1 with the default walk, order 2.  Run it under
                    `rocprofv3 --kernel-trace --stats -- python tools/quad_bench.py trace N` (DESIGN 3.8's table:
                    k_bh_walk / k_bh_walk_duo / k_bh_walk_quad / k_tree_quad rows).
  match N        -- median |a - a_exact| / |a_exact| (a_exact: the strict brute-force kernel) of order 1 at theta2 = 0.25, the
                    theta2 at which order 2 reaches it (bisection on the median), and steps per second of both there.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

BOX = ((0.0, 0.0, 0.0), 64.0)


def bodies(nb, n):
    rec = nb.plummer(2 * n + 64, seed=n)
    return np.ascontiguousarray(rec[np.abs(rec["position"]).max(1) < 30.0][:n])


def bh(nb, rec, order, **tuning):
    sim = nb.Simulation(rec, *BOX, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE, leaf_mode=nb.LEAF_DIRECT, tuning=tuning)
    sim.multipole = order
    return sim


def trace(nb, n):
    rec = bodies(nb, n)
    for theta2 in (0.25, 1.0):
        for order, tuning in ((1, dict(bh_walk_duo=0)), (1, {}), (2, {})):
            with bh(nb, rec, order, **tuning) as sim:
                sim.settings = nb.Settings(1.0, 0.0, 1e-3, theta2)
                for _ in range(3):
                    sim.update_forces()
                sim.sync()
                s = sim.stats()
                print(f"n={n} theta2={theta2} order={order} {tuning}: accepted {s.interactions // 3} visited {s.node_visits // 3}", flush=True)


def median_error(nb, rec, exact, order, theta2):
    with bh(nb, rec, order) as sim:
        sim.settings = nb.Settings(1.0, 0.0, 1e-3, theta2)
        sim.update_forces()
        a = sim.get_points()["acceleration"].astype(np.float64)
    return float(np.median(np.linalg.norm(a - exact, axis=1) / np.linalg.norm(exact, axis=1)))


def steps_per_second(nb, rec, order, theta2, steps=200):
    with bh(nb, rec, order) as sim:
        sim.settings = nb.Settings(1.0, 0.0, 1e-4, theta2)
        sim.steps(20)
        sim.sync()
        t0 = time.perf_counter()
        sim.steps(steps)
        sim.sync()
        return steps / (time.perf_counter() - t0)


def match(nb, n):
    rec = bodies(nb, n)
    with nb.Simulation(rec, *BOX, method=nb.BRUTE_FORCE, math_mode=nb.STRICT) as sim:
        sim.settings = nb.Settings(1.0, 0.0, 1e-3, 0.25)
        sim.update_forces()
        exact = sim.get_points()["acceleration"].astype(np.float64)
    target = median_error(nb, rec, exact, 1, 0.25)
    print(f"n={n}: order 1 theta2=0.25 median error {target:.4e}; order 2 there {median_error(nb, rec, exact, 2, 0.25):.4e}", flush=True)
    lo, hi = 0.25, 4.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        if median_error(nb, rec, exact, 2, mid) <= target:
            lo = mid
        else:
            hi = mid
    print(f"n={n}: order 2 reaches it at theta2={lo:.3f} (median {median_error(nb, rec, exact, 2, lo):.4e})", flush=True)
    steps = 200 if n <= 1 << 17 else 40
    for order, theta2 in ((1, 0.25), (2, 0.25), (2, lo)):
        print(f"n={n}: order {order} theta2={theta2:.3f}: {steps_per_second(nb, rec, order, theta2, steps):.1f} steps/s", flush=True)


if __name__ == "__main__":
    nb = graft.load_package()
    {"trace": trace, "match": match}[sys.argv[1]](nb, int(sys.argv[2]))
