#!/usr/bin/env python3
"""Plain against Krylov-accelerated solve_p (option "krylov" = m) on the seamount problem, timed with HIP events: one solve_p
iteration, and the time and iterations from a cold start to 1e-6 and to 1e-10 (a solve that stops at --maxite reports the residual
it reached).

    python3 scripts/krylov_time.py [--out FILE.json] [--m 0 2 4 8] [--precision 64 32] [CASE ...]      CASE = NXxNYxNZ:METHOD

--precision: the values of option "krylov_precision" to time for every m > 0 (64: fp64 cycles under the loop, 32: fp32 cycles).
Prints one JSON line per (case, m, precision); --out also writes the lines to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import seamount_geometry, resting_column_state  # noqa: E402

DEFAULT = ["512x512x64:FC", "512x512x64:RB"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_case(nx, ny, nz, method, ms, maxite, precisions=(64,), iters=10, reps=3):
    nhydro.set_verbose(0)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, solver_prec=1e-10, solver_maxiter=maxite))
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
    rows = []
    for m, prec in [(m, p) for m in ms for p in (precisions if m else (64,))]:
        nhydro.set_option("krylov", m)
        nhydro.set_option("krylov_precision", prec)
        mg.solve_p(1e-12, 2)  # warm-up (and the allocation of the direction pairs)
        # one iteration: solve_p(0, iters) minus solve_p(0, 0) (the norm of b and the first residual), best of reps
        t_it = min((timed(lambda: mg.solve_p(0.0, iters))[0] - timed(lambda: mg.solve_p(0.0, 0))[0]) / iters for _ in range(reps))
        row = dict(case=f"{nx}x{ny}x{nz}", method=method, krylov=m, krylov_precision=prec, ms_per_iteration=round(t_it, 4))
        for key, tol in (("1e-6", 1e-6), ("1e-10", 1e-10)):
            t, (n, hist) = min((timed(lambda: mg.solve_p(tol, maxite)) for _ in range(2)), key=lambda r: r[0])
            row[f"ms_to_{key}"] = round(t, 3)
            row[f"iterations_to_{key}"] = n
            row[f"res_{key}"] = float(hist[-1])
        row["restarts"] = nhydro.get_option("krylov_restarts")
        rows.append(row)
        print(json.dumps(row), flush=True)
    nhydro.set_option("krylov", 0)
    nhydro.set_option("krylov_precision", 64)
    mg.nhydro_clean()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--m", type=int, nargs="*", default=[0, 2, 4, 8])
    ap.add_argument("--precision", type=int, nargs="*", default=[64], choices=[32, 64])
    ap.add_argument("--maxite", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for c in a.cases:
        dims, method = c.split(":")
        nx, ny, nz = (int(x) for x in dims.split("x"))
        rows += run_case(nx, ny, nz, method, a.m, a.maxite, a.precision)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
