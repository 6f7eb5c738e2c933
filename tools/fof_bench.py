"""Times of nbody_fof_labels and nbody_fof_groups beside nbody_nearest on the same handle, one JSON line per
(dtype, N):

    python tools/fof_bench.py [--bodies 65536,262144] [--dtypes f32,f64] [--link 0.2] [--min-members 2] [--json-out FILE]

Plummer sphere, brute-force handle, no step taken.  The linking length is --link times the mean inter-particle spacing inside
the half-mass radius r_h about the centre of mass: ((4 pi / 3) r_h^3 / (N / 2))^(1/3).  Wall time of the whole call (scratch,
kernels, read-back: every call ends in a stream synchronise) after a warm-up call of each; three windows of at least 0.3 s (or
two calls) each, the spread is the largest deviation of a window from the mean of the three.  nbody_nearest evaluates N (N - 1)
ordered squared distances with no union-find traffic, the group finder half as many: it is the yardstick.  Needs a GPU: there
is no fallback.  No time is asserted anywhere."""
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


def linking_length(rec, fraction):
    x = np.asarray(rec["position"], np.float64)
    m = np.asarray(rec["mass"], np.float64)
    r = np.linalg.norm(x - (m[:, None] * x).sum(axis=0) / m.sum(), axis=1)
    r_half = float(np.median(r))   # (equal masses: half the bodies lie inside)
    return fraction * ((4.0 * np.pi / 3.0) * r_half ** 3 / (len(rec) / 2.0)) ** (1.0 / 3.0)


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("fof_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            b = linking_length(rec, args.link)
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                near = np.zeros(n, np.int32)
                dist2 = np.zeros(n, np.float64)
                label = np.zeros(n, np.int32)
                groups = np.zeros(n // args.min_members + 1, nb.GROUP_DTYPE)
                members = np.zeros(n, np.int32)
                n_all, n_groups, n_members = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)

                def nearest():
                    sim._check(nb.lib.nbody_nearest(sim._h, near.ctypes.data, dist2.ctypes.data, n, None))

                def labels():
                    sim._check(nb.lib.nbody_fof_labels(sim._h, b, label.ctypes.data, n, None, C.byref(n_all)))

                def catalogue():
                    sim._check(nb.lib.nbody_fof_groups(sim._h, b, args.min_members, groups.ctypes.data, len(groups), C.byref(n_groups),
                                                       members.ctypes.data, n, C.byref(n_members)))

                tn, sn = windows(nearest)
                tl, sl = windows(labels)
                tg, sg = windows(catalogue)
                row = {"dtype": dtype, "n": n, "linking_length": b, "min_members": args.min_members, "nearest_ms": round(tn, 4),
                       "fof_labels_ms": round(tl, 4), "fof_groups_ms": round(tg, 4), "spread": round(max(sn, sl, sg), 3),
                       "components": int(n_all.value), "groups": int(n_groups.value), "members": int(n_members.value),
                       "largest": int(groups["count"][: n_groups.value].max()) if n_groups.value else 0}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536,262144")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--link", type=float, default=0.2, help="linking length in mean inter-particle spacings inside the half-mass radius")
    ap.add_argument("--min-members", type=int, default=2)
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
