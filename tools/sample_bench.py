"""Times of nbody_grid_sample under the four plans of its knobs, one JSON line per (grid, op, scheme, plan):

    python tools/sample_bench.py [--bodies 1048576] [--dtype f32] [--repeats 5] [--json-out FILE]

A Plummer sphere of --bodies bodies (brute-force handle, no step taken) sampling a random grid of 128^3 cells over [-4, 4)^3 and
one of 512 x 512 x 1 over [-4, 4)^2 (project_axis 2), value / order-2 gradient / order-4 gradient, NGP / CIC / TSC, under the four
plans sample_sort x sample_pregrad; (0, 0) -- unsorted points, differences on the fly -- is the baseline every other plan's ratio
is taken to at the same commit.  A value has no differences: its two sample_pregrad rows run the same plan and tell the spread.
Wall time of the whole call (scratch, the copy of the grid to the device, the passes, the copies back: every call ends in a
stream synchronise): one warm-up call, then --repeats calls timed one by one; reported are the median, the spread (max - min) /
median, the plan used and the grid reads of the sample kernel (nbody_grid_sample_stats), and that every plan returned the same
bytes.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

GRIDS = {"128^3": ((-4.0, -4.0, -4.0), 0.0625, (128, 128, 128), -1), "512x512x1": ((-4.0, -4.0, 0.0), 0.015625, (512, 512, 1), 2)}
SCHEMES = ("ngp", "cic", "tsc")
OPS = ("value", "grad2", "grad4")
KNOBS = ("sample_sort", "sample_pregrad")


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


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("sample_bench needs a HIP device")
    rec = nb.plummer(args.bodies, f64=args.dtype == "f64")
    rows = []
    with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        for (grid, (origin, spacing, dims, axis)), (op, op_name), (scheme, name) in itertools.product(GRIDS.items(), enumerate(OPS), enumerate(SCHEMES)):
            cells = np.random.default_rng(1).standard_normal(dims)

            def call():
                return sim.grid_sample(cells, origin, spacing, scheme=scheme, op=op, project_axis=axis)
            base_ms, base_bytes = None, None
            for plan in itertools.product((0, 1), (0, 1)):
                for knob, v in zip(KNOBS, plan):
                    sim.set_tuning(knob, v)
                got = call()
                blob = got[0].tobytes() + got[1].tobytes() + got[2].tobytes()
                ms, spread = timed(call, args.repeats)
                stats = sim.grid_sample_stats()
                if base_ms is None:
                    base_ms, base_bytes = ms, blob
                row = dict(grid=grid, op=op_name, scheme=name, bodies=args.bodies, dtype=args.dtype, sort=plan[0], pregrad=plan[1],
                           plan_used=int(stats[1]), ms=round(ms, 3), spread=round(spread, 3), reads=int(stats[2]),
                           ratio_to_00=round(ms / base_ms, 3), same_bytes=blob == base_bytes)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bodies", type=int, default=1 << 20)
    ap.add_argument("--dtype", default="f32", choices=("f32", "f64"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
