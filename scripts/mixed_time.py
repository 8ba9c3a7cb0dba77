#!/usr/bin/env python3
"""fp64 against mixed-precision solve_p (option "cycle_precision" = 32) on the seamount problem, timed with HIP events:
one solve_p iteration, and the time to reach solver_prec = 1e-6 and 1e-12 from a cold start, with the iteration counts (a solve that
stops at the --maxite cap reports the residual it reached).

    python3 scripts/mixed_time.py [--out FILE.json] [CASE ...]      CASE = NXxNYxNZ:METHOD, default: the three cases below

Prints one JSON line per (case, precision) and a table; --out also writes the lines to a file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import seamount_geometry, resting_column_state  # noqa: E402

DEFAULT = ["512x512x64:FC", "512x512x64:RB", "512x1024x128:RB"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_case(nx, ny, nz, method, maxite, iters=10, reps=3):
    nhydro.set_verbose(0)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, solver_prec=1e-12, solver_maxiter=maxite))
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
    rows = []
    for prec in (64, 32):
        nhydro.set_option("cycle_precision", prec)
        mg.solve_p(1e-12, 2)  # warm-up (and, for 32, the shadow's allocation and conversion)
        # one iteration: solve_p(0, iters) minus solve_p(0, 0) (the norm of b and the first residual), best of reps
        t_it = min((timed(lambda: mg.solve_p(0.0, iters))[0] - timed(lambda: mg.solve_p(0.0, 0))[0]) / iters for _ in range(reps))
        row = dict(case=f"{nx}x{ny}x{nz}", method=method, cycle_precision=prec, ms_per_iteration=round(t_it, 4))
        for tol in (1e-6, 1e-12):
            t, (n, hist) = timed(lambda: mg.solve_p(tol, maxite))   # one run, after the warm-up above
            key = "1e-6" if tol == 1e-6 else "1e-12"
            row[f"ms_to_{key}"] = round(t, 3)
            row[f"iterations_to_{key}"] = n
            row[f"res_{key}"] = float(hist[-1])
        row["mixed_iterations"] = nhydro.get_option("mixed_iterations")
        rows.append(row)
        print(json.dumps(row), flush=True)
    nhydro.set_option("cycle_precision", 64)
    mg.nhydro_clean()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--maxite", type=int, default=200, help="iteration cap of the time-to-tolerance solves (the seamount converges slowly at these sizes)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for c in a.cases:
        dims, method = c.split(":")
        nx, ny, nz = (int(x) for x in dims.split("x"))
        rows += run_case(nx, ny, nz, method, a.maxite)
    print(f"\n{'case':>14} {'meth':>4} {'prec':>4} {'ms/it':>8} {'ms->1e-6':>9} {'it':>3} {'ms->1e-12':>10} {'it':>3}")
    for r in rows:
        print(f"{r['case']:>14} {r['method']:>4} {r['cycle_precision']:>4} {r['ms_per_iteration']:8.3f} {r['ms_to_1e-6']:9.2f} "
              f"{r['iterations_to_1e-6']:3d} {r['ms_to_1e-12']:10.2f} {r['iterations_to_1e-12']:3d}")
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
