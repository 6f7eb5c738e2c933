"""Times of nbody_grid_poisson under both plans, one JSON line per (grid, boundary condition, plan), and beside
each the same solve written with torch.fft.fftn on the device -- hipFFT, the yardstick:

    python tools/poisson_bench.py [--repeats 5] [--json-out FILE]

Whole calls on 64^3, 128^3 and 256^3 periodic (spectral Green's function) and on 64^3 and 128^3 isolated (padded to 128^3 and
256^3), random masses, under poisson_lds = 1 (whole lines through LDS, the default tile) and poisson_lds = 0 (one launch per
stage).  Wall time of the whole call (scratch, the tables, the copy of the grid up, the passes, the copy down: every call ends
in a stream synchronise): one warm-up call, then --repeats calls timed one by one; reported are the median, the spread (max -
min) / median, the stats of the call and that both plans returned the same bytes.  The torch solve is complex-to-complex in
f64 like ours, timed twice: as a whole call from a numpy array to a numpy array, and on the device alone with the grid and
the Green's function (the transformed kernel) already there.  It rounds differently: the largest difference to our phi over the
largest |phi| is reported, nothing more.  Needs a GPU: there is no fallback.  No time is asserted anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import poisson_ref as ref  # noqa: E402  (the per-axis tables and Kr, for the yardstick)

CASES = [(64, True), (128, True), (256, True), (64, False), (128, False)]
SPACING, G, SOFTEN = 0.125, 1.0, 0.05


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


def torch_solver(n, periodic, mass):
    """(whole call numpy -> numpy, device-only call) of the same solve through torch.fft"""
    dev = torch.device("cuda")
    if periodic:
        factor = torch.from_numpy(ref.green_factor((n, n, n), SPACING, G, ref.SPECTRAL, 0, ref.CIC)).to(dev)
        on_dev = torch.from_numpy(mass).to(dev)

        def device_only():
            out = torch.fft.ifftn(factor * torch.fft.fftn(on_dev.to(torch.complex128))).real
            torch.cuda.synchronize()
            return out

        def whole():
            m = torch.from_numpy(mass).to(dev)
            return torch.fft.ifftn(factor * torch.fft.fftn(m.to(torch.complex128))).real.cpu().numpy()
        return whole, device_only
    kr = torch.from_numpy(ref.kernel_grid((n, n, n), SPACING, SOFTEN)).to(dev)
    kr_hat = torch.fft.fftn(kr.to(torch.complex128))
    on_dev = torch.zeros((2 * n,) * 3, dtype=torch.float64, device=dev)
    on_dev[:n, :n, :n] = torch.from_numpy(mass).to(dev)

    def device_only():
        out = (-G) * torch.fft.ifftn(kr_hat * torch.fft.fftn(on_dev.to(torch.complex128))).real[:n, :n, :n]
        torch.cuda.synchronize()
        return out

    def whole():   # (Kr is transformed in every call, as nbody_grid_poisson does)
        big = torch.zeros((2 * n,) * 3, dtype=torch.float64, device=dev)
        big[:n, :n, :n] = torch.from_numpy(mass).to(dev)
        k_hat = torch.fft.fftn(kr.to(torch.complex128))
        return ((-G) * torch.fft.ifftn(k_hat * torch.fft.fftn(big.to(torch.complex128))).real[:n, :n, :n]).cpu().numpy()
    return whole, device_only


def measure(args):
    nb = graft.load_package()
    if nb.device_count() < 1:
        raise RuntimeError("poisson_bench needs a HIP device")
    rows = []
    with nb.Simulation(nb.plummer(64), (0.0, 0.0, 0.0), 64.0, method=nb.BRUTE_FORCE, math_mode=nb.FAST) as sim:
        for n, periodic in CASES:
            mass = np.random.default_rng(n).uniform(0.5, 1.5, (n, n, n))
            kw = dict(periodic=True, green=nb.POISSON_SPECTRAL) if periodic else dict(soften=SOFTEN)

            def call():
                return sim.grid_poisson(mass, SPACING, G, **kw)
            whole, device_only = torch_solver(n, periodic, mass)
            torch_ms, torch_spread = timed(whole, args.repeats)
            torch_dev_ms, _ = timed(device_only, args.repeats)
            theirs = whole()
            base = None
            for lds in (1, 0):
                sim.set_tuning("poisson_lds", lds)
                phi = call()
                ms, spread = timed(call, args.repeats)
                stats = [int(v) for v in sim.grid_poisson_stats()]
                if base is None:
                    base = phi.tobytes()
                row = dict(grid=f"{n}^3", boundary="periodic" if periodic else "isolated", lds=lds, plan_used=stats[1], butterfly_launches=stats[2],
                           points=stats[3], ms=round(ms, 3), spread=round(spread, 3), same_bytes=phi.tobytes() == base,
                           torch_whole_ms=round(torch_ms, 3), torch_whole_spread=round(torch_spread, 3), torch_device_ms=round(torch_dev_ms, 3),
                           diff_to_torch=float(np.abs(phi - theirs).max() / np.abs(phi).max()))
                rows.append(row)
                print(json.dumps(row), flush=True)
            sim.set_tuning("poisson_lds", 1)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    rows = measure(args)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
