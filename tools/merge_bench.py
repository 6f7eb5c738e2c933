"""Times of nbody_nearest, nbody_contacts and nbody_merge_contacts, one JSON line per (dtype, N):

    python tools/merge_bench.py [--bodies 4096,65536,262144] [--dtypes f32,f64] [--radius 1e-3] [--json-out FILE]

Plummer sphere, brute-force handle, no step taken.  nbody_nearest and nbody_contacts: wall time of the whole call (scratch,
kernels, read-back: the call ends in a stream synchronise) after a warm-up call of each; three windows of at least 0.3 s (or two
calls) each, the spread is the largest deviation of a window from the mean of the three.  nbody_merge_contacts changes the
state, so it is timed ONCE per handle, after the warm-up of the other two, and carries no spread.  Gpairs/s counts N (N - 1)
ordered squared distances per nbody_nearest call.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def windows(fn):
    """(ms per call, spread) of fn"""
    fn()
    t0 = time.perf_counter()
    fn()
    reps = max(2, min(200, int(0.3 / max(time.perf_counter() - t0, 1e-6)) + 1))
    w = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        w.append((time.perf_counter() - t0) / reps * 1e3)
    mean = float(np.mean(w))
    return mean, max(abs(x - mean) / mean for x in w)


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("merge_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                near = np.zeros(n, np.int32)
                dist2 = np.zeros(n, np.float64)
                lst = np.zeros(n // 2 + 1, nb.CONTACT_DTYPE)
                count = C.c_size_t(0)

                def nearest():
                    sim._check(nb.lib.nbody_nearest(sim._h, near.ctypes.data, dist2.ctypes.data, n, None))

                def contacts():
                    sim._check(nb.lib.nbody_contacts(sim._h, args.radius, lst.ctypes.data, len(lst), C.byref(count)))

                tn, sn = windows(nearest)
                tc, sc = windows(contacts)
                t0 = time.perf_counter()
                sim._check(nb.lib.nbody_merge_contacts(sim._h, args.radius, lst.ctypes.data, len(lst), C.byref(count)))
                tm = (time.perf_counter() - t0) * 1e3
                row = {"dtype": dtype, "n": n, "radius": args.radius, "nearest_ms": round(tn, 4), "contacts_ms": round(tc, 4),
                       "merge_once_ms": round(tm, 4), "spread": round(max(sn, sc), 3),
                       "gpairs_per_s": round(n * (n - 1.0) / (tn * 1e-3) / 1e9, 2), "n_contacts": int(count.value)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="4096,65536,262144")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--radius", type=float, default=1e-3)
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
