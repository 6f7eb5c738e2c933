"""Times of nbody_knn over all pairs and over the cells of a grid with a hint, beside nbody_nearest on the same handle in the
same run, one JSON line per (dtype, N, k):

    python tools/knn_bench.py [--bodies 65536,262144] [--ks 6,32] [--dtypes f32] [--json-out FILE]

Plummer sphere, device-built Barnes-Hut handle, no step taken.  The hint is one mean inter-particle spacing inside the
half-mass radius (tools/fof_bench.py linking_length(rec, 1.0)) times cbrt(k).  Wall time of the whole call (scratch, kernels,
read-back: every call ends in a stream synchronise) after a warm-up call of each; three windows of at least 0.3 s (or two
calls) each, the spread is the largest deviation of a window from the mean of the three.  Beside the times: how many rows the
cells answered and how many went to the all-pairs pass, and that both modes returned the same bytes.  Needs a GPU: there is no
fallback.  No time is asserted anywhere."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from fof_bench import linking_length, windows  # noqa: E402


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("knn_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            spacing = linking_length(rec, 1.0)
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                h = sim._h
                near = np.zeros(n, np.int32)
                near_d2 = np.zeros(n, np.float64)

                def nearest():
                    sim._check(nb.lib.nbody_nearest(h, near.ctypes.data, near_d2.ctypes.data, n, None))

                t_near, s_near = windows(nearest)
                for k in (int(x) for x in args.ks.split(",")):
                    hint = spacing * float(np.cbrt(k))
                    neighbor = np.zeros((n, k), np.int32)
                    dist2 = np.zeros((n, k), np.float64)
                    stats = (C.c_uint64 * 2)()

                    def knn():
                        sim._check(nb.lib.nbody_knn(h, k, hint, neighbor.ctypes.data, dist2.ctypes.data, n, None, stats))

                    row = {"dtype": dtype, "n": n, "k": k, "hint": hint, "nearest_ms": round(t_near, 4), "nearest_spread": round(s_near, 3)}
                    seen = {}
                    for mode, name in ((nb.SEARCH_ALL_PAIRS, "all_pairs"), (nb.SEARCH_CELLS, "cells")):
                        sim.pair_search = mode
                        t, s = windows(knn)
                        row[name + "_ms"] = round(t, 4)
                        row[name + "_spread"] = round(s, 3)
                        row[name + "_rows"] = [int(stats[0]), int(stats[1])]
                        seen[name] = (neighbor.tobytes(), dist2.tobytes())
                    sim.pair_search = nb.SEARCH_ALL_PAIRS
                    row.update(same_results=seen["all_pairs"] == seen["cells"],
                               k1_is_nearest=bool(k != 1 or (neighbor[:, 0].tobytes() == near.tobytes())))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536,262144")
    ap.add_argument("--ks", default="6,32")
    ap.add_argument("--dtypes", default="f32")
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
