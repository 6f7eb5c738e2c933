"""Times of nbody_neighbors_within, nbody_density and nbody_density_center under NBODY_SEARCH_ALL_PAIRS and NBODY_SEARCH_CELLS,
beside nbody_nearest and nbody_fof_labels on the same state in the same run, one JSON line per (dtype, N):

    python tools/within_bench.py [--bodies 262144] [--dtypes f32] [--link 0.2] [--json-out FILE]

Plummer sphere, device-built Barnes-Hut handle, no step taken.  The radius (and the linking length of nbody_fof_labels) is
--link times the mean inter-particle spacing inside the half-mass radius, as in tools/fof_bench.py and tools/cells_bench.py.
Wall time of the whole call (scratch, kernels, read-back: every call ends in a stream synchronise) after a warm-up call of
each; three windows of at least 0.3 s (or two calls) each, the spread is the largest deviation of a window from the mean of
the three.  Beside the times: the directed neighbours, the longest list, the statistics of the search, and that both modes
returned the same bytes.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
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
        raise RuntimeError("within_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            radius = linking_length(rec, args.link)
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                h = sim._h
                n_out, total = C.c_size_t(0), C.c_uint64(0)
                sim._check(nb.lib.nbody_neighbors_within(h, radius, None, 0, None, 0, C.byref(n_out), C.byref(total)))
                offset = np.zeros(n + 1, np.uint64)
                neighbor = np.zeros(max(int(total.value), 1), np.int32)
                rho = np.zeros(n, np.float64)
                count = np.zeros(n, np.int32)
                center = (C.c_double * 3)()
                rho_sum = C.c_double(0)
                label = np.zeros(n, np.int32)
                near = np.zeros(n, np.int32)
                dist2 = np.zeros(n, np.float64)
                n_groups = C.c_size_t(0)

                def lists():
                    sim._check(nb.lib.nbody_neighbors_within(h, radius, offset.ctypes.data, n, neighbor.ctypes.data, len(neighbor), None, None))

                def density():
                    sim._check(nb.lib.nbody_density(h, radius, nb.KERNEL_CUBIC_SPLINE, rho.ctypes.data, count.ctypes.data, n, None))

                def centre():
                    sim._check(nb.lib.nbody_density_center(h, radius, nb.KERNEL_CUBIC_SPLINE, center, C.byref(rho_sum)))

                def labels():
                    sim._check(nb.lib.nbody_fof_labels(h, radius, label.ctypes.data, n, None, C.byref(n_groups)))

                def nearest():
                    sim._check(nb.lib.nbody_nearest(h, near.ctypes.data, dist2.ctypes.data, n, None))

                row = {"dtype": dtype, "n": n, "radius": radius, "directed_neighbors": int(total.value)}
                t, s = windows(nearest)
                row.update(nearest_ms=round(t, 4), nearest_spread=round(s, 3))
                seen = {}
                for mode, name in ((nb.SEARCH_ALL_PAIRS, "all_pairs"), (nb.SEARCH_CELLS, "cells")):
                    sim.pair_search = mode
                    spread = 0.0
                    for call, what in ((lists, "neighbors_within"), (density, "density"), (centre, "density_center"), (labels, "fof_labels")):
                        t, s = windows(call)
                        row[f"{name}_{what}_ms"] = round(t, 4)
                        spread = max(spread, s)
                    row[name + "_spread"] = round(spread, 3)
                    seen[name] = (offset.tobytes(), neighbor.tobytes(), rho.tobytes(), count.tobytes(), bytes(center), rho_sum.value, label.tobytes())
                ran, gridded, occupied, candidates = sim.pair_search_stats()
                row.update(longest_list=int(count.max()) - 1, cell_search_ran=ran, gridded=gridded, occupied_cells=occupied,
                           candidate_pairs=candidates, same_results=seen["all_pairs"] == seen["cells"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="262144")
    ap.add_argument("--dtypes", default="f32")
    ap.add_argument("--link", type=float, default=0.2, help="radius in mean inter-particle spacings inside the half-mass radius")
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
