#!/usr/bin/env python3
"""fp64 against mixed-precision solve_p (option "cycle_precision" = 32) on the seamount problem, timed with HIP events:
one solve_p iteration, and the time to reach solver_prec = 1e-6 and 1e-12 from a cold start, with the iteration counts (a solve that
stops at the --maxite cap reports the residual it reached).  The mixed solve is timed with option "mixed_tail" = 0 (one launch per colour
pass and transfer on every level) and 1 (the small levels of a cycle in one launch).

    python3 scripts/mixed_time.py [--out FILE.json] [--reps N] [--iteration-only] [--lib LIBMGX] [CASE ...]
                                                           CASE = NXxNYxNZ:METHOD, default: the three cases below

--lib: another build of the library, e.g. one made with `make EXTRA=-DMIXED_TAIL_MAX_CELLS=8192 OBJDIR=build_8192 OUT=../libmgx_8192.so`
for the sweep of that bound.  Prints one JSON line per (case, precision, mixed_tail) and a table; --out also writes the lines to a file."""
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


def run_case(nx, ny, nz, method, maxite, iters=10, reps=20, tolerance=True):
    nhydro.set_verbose(0)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, solver_prec=1e-12, solver_maxiter=maxite))
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
    keep = nhydro.get_option("mixed_tail")
    rows = []
    for prec, tail in ((64, None), (32, 0), (32, 1)):
        nhydro.set_option("cycle_precision", prec)
        if tail is not None:
            nhydro.set_option("mixed_tail", tail)
        mg.solve_p(1e-12, 2)  # warm-up (and, for 32, the shadow's allocation and conversion)
        # one iteration: solve_p(0, iters) minus solve_p(0, 0) (the norm of b and the first residual); median of reps, with the spread
        t_it = sorted((timed(lambda: mg.solve_p(0.0, iters))[0] - timed(lambda: mg.solve_p(0.0, 0))[0]) / iters for _ in range(reps))
        c0 = nhydro.counters()["launches"]
        mg.solve_p(0.0, iters)
        c1 = nhydro.counters()["launches"]
        mg.solve_p(0.0, 0)
        row = dict(case=f"{nx}x{ny}x{nz}", method=method, cycle_precision=prec, mixed_tail=tail, tail_first=nhydro.mixed_tail_first(nx, ny, nz),
                   ms_per_iteration=round(float(np.median(t_it)), 4), ms_min=round(t_it[0], 4), ms_max=round(t_it[-1], 4), reps=reps,
                   launches_per_iteration=(c1 - c0 - (nhydro.counters()["launches"] - c1)) // iters)
        for tol in (1e-6, 1e-12) if tolerance else ():
            t, (n, hist) = timed(lambda: mg.solve_p(tol, maxite))   # one run, after the warm-up above
            key = "1e-6" if tol == 1e-6 else "1e-12"
            row[f"ms_to_{key}"] = round(t, 3)
            row[f"iterations_to_{key}"] = n
            row[f"res_{key}"] = float(hist[-1])
        row["mixed_iterations"] = nhydro.get_option("mixed_iterations")
        rows.append(row)
        print(json.dumps(row), flush=True)
    nhydro.set_option("cycle_precision", 64)
    nhydro.set_option("mixed_tail", keep)
    mg.nhydro_clean()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--maxite", type=int, default=200, help="iteration cap of the time-to-tolerance solves (the seamount converges slowly at these sizes)")
    ap.add_argument("--reps", type=int, default=20, help="timings of one iteration; the median is reported, with the smallest and the largest")
    ap.add_argument("--iteration-only", action="store_true", help="skip the time-to-tolerance solves")
    ap.add_argument("--lib", default=None, help="path of the libmgx.so to load instead of the package's own")
    a = ap.parse_args()
    if a.lib:
        from mgroms_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    torch.cuda.set_device(0)
    rows = []
    for c in a.cases:
        dims, method = c.split(":")
        nx, ny, nz = (int(x) for x in dims.split("x"))
        rows += run_case(nx, ny, nz, method, a.maxite, reps=a.reps, tolerance=not a.iteration_only)
    print(f"\n{'case':>14} {'meth':>4} {'prec':>4} {'tail':>4} {'ms/it':>8} {'min':>8} {'max':>8} {'launches':>8}" + ("" if a.iteration_only else f" {'ms->1e-6':>9} {'it':>3} {'ms->1e-12':>10} {'it':>3}"))
    for r in rows:
        tail = "-" if r["mixed_tail"] is None else r["mixed_tail"]
        line = f"{r['case']:>14} {r['method']:>4} {r['cycle_precision']:>4} {tail:>4} {r['ms_per_iteration']:8.3f} {r['ms_min']:8.3f} {r['ms_max']:8.3f} {r['launches_per_iteration']:8d}"
        if not a.iteration_only:
            line += f" {r['ms_to_1e-6']:9.2f} {r['iterations_to_1e-6']:3d} {r['ms_to_1e-12']:10.2f} {r['iterations_to_1e-12']:3d}"
        print(line)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
