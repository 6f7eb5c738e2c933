"""Times of nbody_pair_counts over all pairs and over the cells of a grid, beside nbody_nearest on the same handle in the same
run -- the same frame without a histogram -- (DESIGN 3.22), one JSON line per (world, N, bins):

    python tools/pair_counts_bench.py [--bodies 65536,262144] [--worlds plummer,clumpy] [--bins 32,1024] [--dtype f32]
                                      [--repeats 5] [--json-out FILE]

Worlds: the Plummer sphere the sibling tools use, and a clumpy one -- nine bodies in ten in 64 normal clumps of sigma 0.05
scattered over [-8, 8]^3, the rest a uniform background there --, in which most pairs fall into the few bins about the
distance between two clumps.  Brute-force handle, no step taken.  Two sets of log bins:
    wide   1e-3 .. 32: every separation of the world; all pairs only (a grid for that length is one cell), once for each
           value of the pair_hist_combine knob (0 each lane adds its own count, 1 the first counting lane's slot is combined,
           2 every distinct slot is)
    near   from 2e-3 to 2 mean inter-particle spacings inside the half-mass radius (tools/fof_bench.py linking_length): all
           pairs and cells
Wall time of the whole call (scratch, kernel, read-back: every call ends in a stream synchronise): one warm-up call, then
--repeats calls timed one by one; reported are the median and the spread (max - min) / median.  Beside the times: the ratio
to nbody_nearest, the share of the fullest bin, the statistics of the search and that every variant returned the same
integers.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from fof_bench import linking_length  # noqa: E402


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


def log_edges(lo, hi, n_bins):
    e = lo * (hi / lo) ** (np.arange(n_bins + 1, dtype=np.float64) / n_bins)
    e[0], e[-1] = lo, hi
    return e


def clumpy(nb, n, f64, seed=7):
    rng = np.random.default_rng(seed)
    rec = nb.plummer(n, f64=f64)   # (masses and velocities; the positions are replaced)
    x = rng.uniform(-8.0, 8.0, (n, 3))
    centres = rng.uniform(-8.0, 8.0, (64, 3))
    in_clump = n - n // 10
    x[:in_clump] = centres[rng.integers(0, 64, in_clump)] + 0.05 * rng.standard_normal((in_clump, 3))
    rec["position"] = x[rng.permutation(n)]
    return rec


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("pair_counts_bench needs a HIP device")
    f64 = args.dtype == "f64"
    rows = []
    for world in args.worlds.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=f64) if world == "plummer" else clumpy(nb, n, f64)
            near_hi = linking_length(rec, 2.0)
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                near = np.zeros(n, np.int32)
                dist2 = np.zeros(n, np.float64)

                def nearest():
                    sim._check(nb.lib.nbody_nearest(sim._h, near.ctypes.data, dist2.ctypes.data, n, None))

                t_near, s_near = timed(nearest, args.repeats)
                for n_bins in (int(x) for x in args.bins.split(",")):
                    row = {"world": world, "n": n, "dtype": args.dtype, "bins": n_bins, "nearest_ms": round(t_near, 3), "nearest_spread": round(s_near, 3)}
                    wide = log_edges(1e-3, 32.0, n_bins)
                    close = log_edges(1e-3 * near_hi, near_hi, n_bins)
                    got = {}
                    sim.pair_search = nb.SEARCH_ALL_PAIRS
                    for combine in (0, 1, 2):
                        sim.set_tuning("pair_hist_combine", combine)
                        t, s = timed(lambda: got.__setitem__(("wide", combine), sim.pair_counts(wide)), args.repeats)
                        row.update({f"wide_combine{combine}_ms": round(t, 3), f"wide_combine{combine}_spread": round(s, 3),
                                    f"wide_combine{combine}_over_nearest": round(t / t_near, 2)})
                    sim.set_tuning("pair_hist_combine", 0)
                    t, s = timed(lambda: got.__setitem__(("near", "all"), sim.pair_counts(close)), args.repeats)
                    row.update(near_all_pairs_ms=round(t, 3), near_all_pairs_spread=round(s, 3), near_all_pairs_over_nearest=round(t / t_near, 2))
                    sim.pair_search = nb.SEARCH_CELLS
                    t, s = timed(lambda: got.__setitem__(("near", "cells"), sim.pair_counts(close)), args.repeats)
                    ran, gridded, occupied, candidates = sim.pair_search_stats()
                    row.update(near_cells_ms=round(t, 3), near_cells_spread=round(s, 3), near_hi=near_hi, cell_search_ran=ran, gridded=gridded,
                               occupied_cells=occupied, candidate_pairs=candidates)
                    counts, outside = got[("wide", 0)]
                    pairs = n * (n - 1) // 2
                    row.update(fullest_bin_share=round(float(counts.max()) / pairs, 4), wide_outside=[int(outside[0]), int(outside[1])],
                               sums_to_all_pairs=int(counts.sum()) + int(outside.sum()) == pairs,
                               same_results=all(got[("wide", c)][0].tobytes() == counts.tobytes() and got[("wide", c)][1].tobytes() == outside.tobytes()
                                                for c in (1, 2)) and
                               got[("near", "all")][0].tobytes() == got[("near", "cells")][0].tobytes() and
                               got[("near", "all")][1].tobytes() == got[("near", "cells")][1].tobytes())
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536,262144")
    ap.add_argument("--worlds", default="plummer,clumpy")
    ap.add_argument("--bins", default="32,1024")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
