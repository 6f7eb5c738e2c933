"""Times of nbody_tidal_at beside nbody_field_at at the same shapes, one JSON line per (dtype, N, M):

    python tools/tidal_bench.py [--bodies 65536] [--probes 4096,65536] [--dtypes f32,f64] [--pairs-max 1e10]
                                [--json-out FILE] [--write-design] [--from-json FILE]

Plummer sphere, fast device-build Barnes-Hut handle, theta2 = 0.25, eps = 1e-2, uniform random probes in the bodies' bounding
cube.  nbody_field_at's kernels and host path are the parent commit's, untouched by nbody_tidal_at, so its time on the same
handle is the comparison the section asks for.  Wall time of the whole call (preparation, sort, kernels, read-back: the
call ends in a stream synchronise) after a warm-up call of each, the two calls alternating inside the timed window, at least
0.3 s of each; the spread is the largest deviation of three such windows from their mean.  Needs a GPU: there is no fallback.
    tree_tidal_ms / tree_field_ms      NBODY_POTENTIAL_TREE
    pairs_tidal_ms / pairs_field_ms    NBODY_POTENTIAL_PAIRS, when M x N <= --pairs-max
--write-design puts the lines (of this run, or of --from-json FILE written earlier by --json-out) into DESIGN.md between the
tidal_bench markers of section 3.14.  No time is asserted anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

BEGIN, END = "<!-- tidal_bench:begin -->", "<!-- tidal_bench:end -->"


def alternating(fa, fb):
    """(ms of fa, ms of fb, spread): a warm-up of each, then three windows of alternating calls, each at least 0.3 s per function"""
    fa()
    fb()
    t0 = time.perf_counter()
    fa()
    fb()
    reps = max(2, min(200, int(0.6 / max(time.perf_counter() - t0, 1e-6)) + 1))
    wa, wb = [], []
    for _ in range(3):
        ta = tb = 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            fa()
            t1 = time.perf_counter()
            fb()
            ta, tb = ta + (t1 - t0), tb + (time.perf_counter() - t1)
        wa.append(ta / reps * 1e3)
        wb.append(tb / reps * 1e3)
    ma, mb = float(np.mean(wa)), float(np.mean(wb))
    spread = max(max(abs(w - ma) / ma for w in wa), max(abs(w - mb) / mb for w in wb))
    return ma, mb, spread


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("tidal_bench needs a HIP device")
    rng = np.random.default_rng(1)
    rows = []
    for dtype in args.dtypes.split(","):
        for n in (int(x) for x in args.bodies.split(",")):
            rec = nb.plummer(n, f64=dtype == "f64")
            own = rec["position"].astype(np.float64)
            lo, hi = own.min(), own.max()
            with nb.Simulation(rec, (0.0, 0.0, 0.0), 64.0, method=nb.BARNES_HUT, math_mode=nb.FAST, tree_build=nb.TREE_DEVICE) as sim:
                sim.settings = nb.Settings(1.0, 1e-2, 1e-3, 0.25)
                for m in (int(x) for x in args.probes.split(",")):
                    pts = rng.uniform(lo, hi, (m, 3))
                    row = {"dtype": dtype, "n": n, "m": m}
                    modes = [("tree", nb.POTENTIAL_TREE)] + ([("pairs", nb.POTENTIAL_PAIRS)] if float(m) * n <= args.pairs_max else [])
                    for name, mode in modes:
                        t, f, spread = alternating(lambda: sim.tidal_at(pts, mode), lambda: sim.field_at(pts, mode))
                        row[f"{name}_tidal_ms"], row[f"{name}_field_ms"], row[f"{name}_spread"] = round(t, 4), round(f, 4), round(spread, 3)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    return rows


def write_design(rows):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    lines = ["", "| dtype | N | M | TREE tidal ms | TREE field ms | PAIRS tidal ms | PAIRS field ms | largest spread |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        cell = lambda k: f"{r[k]:.3f}" if k in r else "not measured"   # noqa: E731
        spread = max(r.get("tree_spread", 0.0), r.get("pairs_spread", 0.0))
        lines.append(f"| {r['dtype']} | {r['n']} | {r['m']} | {cell('tree_tidal_ms')} | {cell('tree_field_ms')} | {cell('pairs_tidal_ms')} | {cell('pairs_field_ms')} | {spread:.1%} |")
    open(path, "w").write(text[:a] + "\n".join(lines) + "\n" + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="65536")
    ap.add_argument("--probes", default="4096,65536")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--pairs-max", type=float, default=1e10)
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
