"""Times of nbody_fof_groups and nbody_fof_bound_groups on the same state, one JSON line per dtype:

    python tools/fof_bound_bench.py [--bodies 262144] [--dtypes f64] [--link 0.2] [--blobs 3,3] [--blob-bodies 16384]
                                    [--max-iterations 32] [--repeats 5] [--json-out FILE]

The world: a Plummer sphere plus --blobs COLD,HOT Gaussian blobs of --blob-bodies bodies each (sigma 0.03, well away from the
sphere), all of equal mass.  Cold blobs get speeds uniform in [0, 1.3 v) in random directions, v = sqrt(2 g M_blob / sigma): the
fastest members escape, the well gets shallower and more follow, so these groups strip over several passes; hot blobs get 3 v
to 6 v and dissolve.  The linking length is --link times the mean inter-particle spacing inside the sphere's half-mass radius,
as in tools/fof_bench.py.  Brute-force handle, no step taken.  Wall time of the whole call (scratch, kernels, the read-back per
pass; every call ends in a stream synchronise) after a warm-up call of each: the median of --repeats calls, and the largest
deviation from it.  Passes and pair terms are counted from the records: a listed group ran `iterations` passes of fof_count^2
terms each; a dissolved group ran at least one, so its terms are a lower bound and are reported apart.  Needs a GPU: there is
no fallback.  No time is asserted anywhere."""
import argparse
import ctypes as C
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

SIGMA = 0.03


def world(nb, n, f64, cold, hot, blob_bodies, g, seed=11):
    k = cold + hot
    n_sphere = n - k * blob_bodies
    assert n_sphere > 0
    sphere = nb.plummer(n_sphere, f64=f64)
    rec = np.zeros(n, sphere.dtype)
    rec[:n_sphere] = sphere
    rec["mass"] = 1.0 / n
    rng = np.random.default_rng(seed)
    v_esc = np.sqrt(2.0 * g * (blob_bodies / n) / SIGMA)
    for j in range(k):
        sl = slice(n_sphere + j * blob_bodies, n_sphere + (j + 1) * blob_bodies)
        angle = 2.0 * np.pi * j / k
        rec["position"][sl] = np.array([6.0 * np.cos(angle), 6.0 * np.sin(angle), 0.0]) + SIGMA * rng.standard_normal((blob_bodies, 3))
        u = rng.standard_normal((blob_bodies, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        lo, hi = (0.0, 1.3) if j < cold else (3.0, 6.0)
        rec["velocity"][sl] = rng.uniform(lo * v_esc, hi * v_esc, (blob_bodies, 1)) * u
    return rec[rng.permutation(n)], sphere   # (the blobs' members lie at random indices)


def timed(fn, repeats):
    """(median ms, largest relative deviation from it) of `repeats` calls of fn after a warm-up call"""
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(t))
    return med, max(abs(x - med) / med for x in t)


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("fof_bound_bench needs a HIP device")
    cold, hot = (int(x) for x in args.blobs.split(","))
    rows = []
    for dtype in args.dtypes.split(","):
        n, g = args.bodies, 1.0
        rec, sphere = world(nb, n, dtype == "f64", cold, hot, args.blob_bodies, g)
        b = linking_length(sphere, args.link)
        with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
            sim.settings = nb.Settings(g, 1e-2, 1e-3, 0.25)
            fof = np.zeros(n // 2 + 1, nb.GROUP_DTYPE)
            bound = np.zeros(n // 2 + 1, nb.BOUND_GROUP_DTYPE)
            members = np.zeros(n, np.int32)
            energy = np.zeros(n, np.float64)
            n_fof, n_fof_members, n_bound, n_bound_members = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)

            def catalogue():
                sim._check(nb.lib.nbody_fof_groups(sim._h, b, 2, fof.ctypes.data, len(fof), C.byref(n_fof), members.ctypes.data, n,
                                                   C.byref(n_fof_members)))

            def unbind():
                sim._check(nb.lib.nbody_fof_bound_groups(sim._h, b, 2, args.max_iterations, bound.ctypes.data, len(bound), C.byref(n_bound),
                                                         members.ctypes.data, n, C.byref(n_bound_members), energy.ctypes.data))

            tg, sg = timed(catalogue, args.repeats)
            tb, sb = timed(unbind, args.repeats)
            f, r = fof[: n_fof.value], bound[: n_bound.value]
            gone = ~np.isin(f["first"], r["first"])
            row = {"dtype": dtype, "n": n, "linking_length": b, "max_iterations": args.max_iterations, "fof_groups_ms": round(tg, 3),
                   "fof_bound_groups_ms": round(tb, 3), "spread": round(max(sg, sb), 3), "fof_groups": int(n_fof.value),
                   "fof_members": int(n_fof_members.value), "largest_fof": int(f["count"].max()) if len(f) else 0,
                   "bound_groups": int(n_bound.value), "bound_members": int(n_bound_members.value), "dissolved": int(gone.sum()),
                   "largest_bound": int(r["count"].max()) if len(r) else 0, "passes": int(r["iterations"].max()) if len(r) else 1,
                   "unconverged": int((r["converged"] == 0).sum()),
                   "pair_terms_listed": int((r["iterations"].astype(np.int64) * r["fof_count"].astype(np.int64) ** 2).sum()),
                   "pair_terms_dissolved_at_least": int((f["count"][gone].astype(np.int64) ** 2).sum())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--dtypes", default="f64")
    ap.add_argument("--link", type=float, default=0.2, help="linking length in mean inter-particle spacings inside the sphere's half-mass radius")
    ap.add_argument("--blobs", default="3,3", help="COLD,HOT")
    ap.add_argument("--blob-bodies", type=int, default=16384)
    ap.add_argument("--max-iterations", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json-out")
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
