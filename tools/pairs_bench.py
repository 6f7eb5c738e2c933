"""Times of nbody_partners and nbody_bound_pairs, one JSON line per (dtype, N):

    python tools/pairs_bench.py [--bodies 4096,65536,262144] [--dtypes f32,f64] [--json-out FILE] [--write-design] [--from-json FILE]

Plummer sphere, brute-force handle, g_soft = 1e-2, no step taken.  Wall time of the whole call (scratch, kernels, read-back: the
call ends in a stream synchronise) after a warm-up call of each; three windows of at least 0.3 s (or two calls) each, the
spread is the largest deviation of a window from the mean of the three.  Gpairs/s counts N (N - 1) ordered pair energies per
call.  Needs a GPU: there is no fallback.  --write-design puts the lines (of this run, or of --from-json FILE written earlier
by --json-out) into DESIGN.md between the pairs_bench markers of section 3.16.  No time is asserted anywhere."""
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

BEGIN, END = "<!-- pairs_bench:begin -->", "<!-- pairs_bench:end -->"


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
        raise RuntimeError("pairs_bench needs a HIP device")
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                partner = np.zeros(n, np.int32)
                energy = np.zeros(n, np.float64)
                pairs = np.zeros(n // 2 + 1, nb.BOUND_PAIR_DTYPE)
                count, total = C.c_size_t(0), C.c_double(0)

                def partners():
                    sim._check(nb.lib.nbody_partners(sim._h, partner.ctypes.data, energy.ctypes.data, n, None))

                def bound_pairs():
                    sim._check(nb.lib.nbody_bound_pairs(sim._h, pairs.ctypes.data, len(pairs), C.byref(count), C.byref(total)))

                tp, sp = windows(partners)
                tb, sb = windows(bound_pairs)
                row = {"dtype": dtype, "n": n, "partners_ms": round(tp, 4), "bound_pairs_ms": round(tb, 4), "spread": round(max(sp, sb), 3),
                       "gpairs_per_s": round(n * (n - 1.0) / (tp * 1e-3) / 1e9, 2), "n_pairs": int(count.value)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def write_design(rows):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    lines = ["", "| dtype | N | nbody_partners ms | nbody_bound_pairs ms | pair energies, G/s | bound pairs | largest spread |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['dtype']} | {r['n']} | {r['partners_ms']:.3f} | {r['bound_pairs_ms']:.3f} | {r['gpairs_per_s']:.1f} | {r['n_pairs']} | {r['spread']:.1%} |")
    open(path, "w").write(text[:a] + "\n".join(lines) + "\n" + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="4096,65536,262144")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--json-out")
    ap.add_argument("--from-json")
    ap.add_argument("--write-design", action="store_true")
    args = ap.parse_args()
    if args.from_json:
        rows = [json.loads(line) for line in open(args.from_json) if line.strip()]
    else:
        rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    if args.write_design:
        write_design(rows)


if __name__ == "__main__":
    main()
