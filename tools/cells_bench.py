"""Times of nbody_fof_labels and nbody_contacts under NBODY_SEARCH_ALL_PAIRS and NBODY_SEARCH_CELLS on the same handle (DESIGN
3.19), one JSON line per (dtype, N):

    python tools/cells_bench.py [--bodies 65536,262144,1048576] [--all-pairs-up-to 262144] [--dtypes f32] [--link 0.2] [--json-out FILE]

Plummer sphere, device-built Barnes-Hut handle, no step taken.  The linking length (and the contact radius) is --link times the
mean inter-particle spacing inside the half-mass radius, as in tools/fof_bench.py.  Wall time of the whole call (scratch,
kernels, read-back: every call ends in a stream synchronise) after a warm-up call of each; three windows of at least 0.3 s (or
two calls) each, the spread is the largest deviation of a window from the mean of the three.  Above --all-pairs-up-to bodies
only the cell search is timed: those rows have no all-pairs twin.  Beside the times: the occupied cells and the candidate pairs
of the search (nbody_pair_search_stats), and that both modes returned the same labels and the same contact list wherever both
ran.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
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
        raise RuntimeError("cells_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            b = linking_length(rec, args.link)
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                label = np.zeros(n, np.int32)
                contact = np.zeros(n // 2 + 1, nb.CONTACT_DTYPE)
                n_groups, n_contacts = C.c_size_t(0), C.c_size_t(0)

                def labels():
                    sim._check(nb.lib.nbody_fof_labels(sim._h, b, label.ctypes.data, n, None, C.byref(n_groups)))

                def contacts():
                    sim._check(nb.lib.nbody_contacts(sim._h, b, contact.ctypes.data, len(contact), C.byref(n_contacts)))

                row = {"dtype": dtype, "n": n, "length": b}
                seen = {}
                for mode, name in ((nb.SEARCH_ALL_PAIRS, "all_pairs"), (nb.SEARCH_CELLS, "cells")):
                    if mode == nb.SEARCH_ALL_PAIRS and n > args.all_pairs_up_to:
                        row.update(all_pairs_fof_labels_ms=None, all_pairs_contacts_ms=None)
                        continue
                    sim.pair_search = mode
                    tl, sl = windows(labels)
                    tc, sc = windows(contacts)
                    seen[name] = (label.tobytes(), int(n_groups.value), contact[: n_contacts.value].tobytes())
                    row.update({name + "_fof_labels_ms": round(tl, 4), name + "_contacts_ms": round(tc, 4), name + "_spread": round(max(sl, sc), 3)})
                ran, gridded, occupied, candidates = sim.pair_search_stats()
                row.update(components=int(n_groups.value), contacts=int(n_contacts.value), cell_search_ran=ran, gridded=gridded,
                           occupied_cells=occupied, candidate_pairs=candidates,
                           same_results=seen["all_pairs"] == seen["cells"] if "all_pairs" in seen else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536,262144,1048576")
    ap.add_argument("--all-pairs-up-to", type=int, default=262144, help="larger worlds are timed under the cell search only")
    ap.add_argument("--dtypes", default="f32")
    ap.add_argument("--link", type=float, default=0.2, help="linking length in mean inter-particle spacings inside the half-mass radius")
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
