#!/usr/bin/env python3
"""What option "hold_odd_nz" buys and costs (include/mgx.h), with device events around solve_p, median of --reps:
  per size (default: 512 x 512 x 40 and x 80 held, their even neighbours x 32 and x 48 on the default hierarchy, and x 48 held, whose
  coarsest level is 4 x 4 x 3 instead of 32 x 32 x 3), per relax_method (FC, RB) and per "krylov" (0, 4)
    to_1e-6, to_1e-10     iterations, ms and launches of a cold solve_p to that tolerance (seamount, u = v = 0, w = -1), final residual
    ms_per_iteration      the 1e-10 solve's ms / iterations; launches_per_iteration likewise
No threshold: the figure to compare is the per-iteration time of the even neighbours in the same run.
  python3 scripts/hold_time.py --out profiles/hold_odd_nz_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import resting_column_state, seamount_geometry  # noqa: E402


def timed_solve(tol, maxit):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n0 = nhydro.counters()["launches"]
    e0.record()
    n, hist = mg.solve_p(tol, maxit)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), nhydro.counters()["launches"] - n0, n, float(hist[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--cases", nargs="+", default=["32:0", "48:0", "48:1", "40:1", "80:1"], help="nz:hold_odd_nz")
    ap.add_argument("--methods", nargs="+", default=["FC", "RB"])
    ap.add_argument("--krylov", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--maxit", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nx, ny = a.plane
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    doc = {"plane": [nx, ny], "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "cases": []}
    dx, dy, zeta, h = seamount_geometry(nx, ny, 1, 1, 0)
    try:
        for case in a.cases:
            nz, hold = (int(v) for v in case.split(":"))
            u, v, w = resting_column_state(nx, ny, nz)
            for method in a.methods:
                mg.nhydro_clean()
                nhydro.set_option("hold_odd_nz", hold)
                mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method))
                mg.nhydro_matrices(dx, dy, zeta, h, None, 4e3, 0.0, 0.0)
                nhydro.compute_rhs(u, v, w)
                levels = [[mg.grid(l).nx, mg.grid(l).ny, mg.grid(l).nz] for l in range(1, mg.nlevs() + 1)]
                for kr in a.krylov:
                    nhydro.set_option("krylov", kr)
                    row = {"nz": nz, "hold_odd_nz": hold, "relax_method": method, "krylov": kr, "levels_nz": [l[2] for l in levels], "coarsest": levels[-1]}
                    for tol, key in ((1e-6, "to_1e-6"), (1e-10, "to_1e-10")):
                        runs = [timed_solve(tol, a.maxit) for _ in range(a.warmup + a.reps)][a.warmup:]
                        ms = [r[0] for r in runs]
                        row[key] = {"iterations": runs[0][2], "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                    "launches": runs[0][1], "final_residual": runs[0][3], "converged": bool(runs[0][3] <= tol)}
                    t = row["to_1e-10"]
                    row["ms_per_iteration"] = round(t["ms_median"] / max(t["iterations"], 1), 4)
                    row["launches_per_iteration"] = round(t["launches"] / max(t["iterations"], 1), 1)
                    nhydro.set_option("krylov", 0)
                    doc["cases"].append(row)
                    print(json.dumps(row))
    finally:
        mg.nhydro_clean()
        nhydro.set_option("hold_odd_nz", 0); nhydro.set_option("krylov", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
