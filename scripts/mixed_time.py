#!/usr/bin/env python3
"""fp64 against mixed-precision solve_p (option "cycle_precision" = 32) on the seamount problem, timed with HIP events:
one solve_p iteration, and the time to reach solver_prec = 1e-6 and 1e-12 from a cold start, with the iteration counts (a solve that
stops at the --maxite cap reports the residual it reached).  The mixed solve is timed with option "mixed_tail" = 0 (one launch per colour
pass and transfer on every level) and 1 (the small levels of a cycle in one launch), and with option "mixed_ring" = 0 (the row-by-row
colour pass k_relax32 on every level) and 1 (the pipelined pass k_relax32r on the levels that are not small), and with option
"mixed_direct" = 0 (the coarsest solve of a cycle by ns_coarsest sweeps) and 1 (by one matrix-vector product).  The configurations of a
case take turns within every repetition; with "mixed_ring" = 1 the row also holds the gap of p after the timed iterations to the same
cycles with "mixed_ring" = 0, over max|p| (other roundings: expected within 1e-5).  The yardstick of a "mixed_direct" = 1 row is the
"mixed_direct" = 0 row of the same run with the same "mixed_tail" and "mixed_ring".

    python3 scripts/mixed_time.py [--out FILE.json] [--reps N] [--iteration-only] [--rings 0,1] [--directs 0,1] [--lib LIBMGX] [CASE ...]
                                                           CASE = NXxNYxNZ:METHOD, default: the three cases below

--lib: another build of the library, e.g. one made with `make EXTRA=-DMIXED_TAIL_MAX_CELLS=8192 OBJDIR=build_8192 OUT=../libmgx_8192.so`
for the sweep of that bound, or with one constant of choose_relax32 (mgx_choice.h) edited (profiles/mixed_ring_time.json names the edits).  Prints one JSON line per
(case, precision, mixed_tail, mixed_ring, mixed_direct) and a table; --out also writes the lines to a file."""
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


def run_case(nx, ny, nz, method, maxite, iters=10, reps=20, tolerance=True, rings=(0, 1), directs=(0,)):
    nhydro.set_verbose(0)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, solver_prec=1e-12, solver_maxiter=maxite))
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
    keep = {k: nhydro.get_option(k) for k in ("mixed_tail", "mixed_ring", "mixed_direct")}
    configs = [(64, None, None, None)] + [(32, tail, ring, direct) for tail in (0, 1) for ring in rings for direct in directs]

    def select(prec, tail, ring, direct):
        nhydro.set_option("cycle_precision", prec)
        if tail is not None:
            nhydro.set_option("mixed_tail", tail)
            nhydro.set_option("mixed_ring", ring)
            nhydro.set_option("mixed_direct", direct)

    for cfg in configs:
        select(*cfg)
        mg.solve_p(1e-12, 2)  # warm-up (and, for 32, the shadow's allocation and conversion, and the operator of mixed_direct)
    # one iteration: solve_p(0, iters) minus solve_p(0, 0) (the norm of b and the first residual); the configurations take turns within
    # every repetition, so that a drift of the machine falls on all of them; median of reps, with the spread
    t_it = {cfg: [] for cfg in configs}
    for _ in range(reps):
        for cfg in configs:
            select(*cfg)
            t_it[cfg].append((timed(lambda: mg.solve_p(0.0, iters))[0] - timed(lambda: mg.solve_p(0.0, 0))[0]) / iters)
    rows, p_after = [], {}
    for cfg in configs:
        prec, tail, ring, direct = cfg
        select(*cfg)
        t = sorted(t_it[cfg])
        c0, r0, d0 = nhydro.counters()["launches"], nhydro.get_option("mixed_ring_passes"), nhydro.get_option("mixed_direct_solves")
        mg.solve_p(0.0, iters)
        c1, r1, d1 = nhydro.counters()["launches"], nhydro.get_option("mixed_ring_passes"), nhydro.get_option("mixed_direct_solves")
        p_after[cfg] = mg.grid(1).p
        mg.solve_p(0.0, 0)
        row = dict(case=f"{nx}x{ny}x{nz}", method=method, cycle_precision=prec, mixed_tail=tail, mixed_ring=ring, mixed_direct=direct,
                   tail_first=nhydro.mixed_tail_first(nx, ny, nz), ring_levels=nhydro.mixed_ring_levels(nx, ny, nz),
                   ms_per_iteration=round(float(np.median(t)), 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4), reps=reps,
                   launches_per_iteration=(c1 - c0 - (nhydro.counters()["launches"] - c1)) // iters, ring_passes_per_iteration=(r1 - r0) // iters,
                   mixed_direct_solves=(d1 - d0) // iters, direct_cells=nhydro.mixed_direct_cells(nx, ny, nz))
        if ring and (prec, tail, 0, direct) in p_after:   # p after `iters` iterations against the same cycles with the row-by-row pass, over max|p|
            ref = p_after[(prec, tail, 0, direct)]
            row["p_gap_to_ring0"] = float(np.abs(p_after[cfg] - ref).max() / np.abs(ref).max())
        for tol in (1e-6, 1e-12) if tolerance else ():
            t1, (n, hist) = timed(lambda: mg.solve_p(tol, maxite))   # one run, after the warm-up above
            key = "1e-6" if tol == 1e-6 else "1e-12"
            row[f"ms_to_{key}"] = round(t1, 3)
            row[f"iterations_to_{key}"] = n
            row[f"res_{key}"] = float(hist[-1])
        row["mixed_iterations"] = nhydro.get_option("mixed_iterations")
        rows.append(row)
        print(json.dumps(row), flush=True)
    nhydro.set_option("cycle_precision", 64)
    for k, v in keep.items():
        nhydro.set_option(k, v)
    mg.nhydro_clean()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--maxite", type=int, default=200, help="iteration cap of the time-to-tolerance solves (the seamount converges slowly at these sizes)")
    ap.add_argument("--reps", type=int, default=20, help="timings of one iteration; the median is reported, with the smallest and the largest")
    ap.add_argument("--iteration-only", action="store_true", help="skip the time-to-tolerance solves")
    ap.add_argument("--rings", default="0,1", help="values of option mixed_ring to time: 0,1 or 0 alone (0 is the yardstick of the gap of p)")
    ap.add_argument("--directs", default="0,1", help="values of option mixed_direct to time: 0,1 or 0 alone (0 is the yardstick of the rows of 1)")
    ap.add_argument("--lib", default=None, help="path of the libmgx.so to load instead of the package's own")
    a = ap.parse_args()
    rings = tuple(int(x) for x in a.rings.split(","))
    if rings not in ((0,), (0, 1), (1,)):
        ap.error("--rings takes 0, 0,1 or 1 (1 alone: no gap of p to the rows of mixed_ring = 0)")
    directs = tuple(int(x) for x in a.directs.split(","))
    if directs not in ((0,), (0, 1)):
        ap.error("--directs takes 0 or 0,1: the rows of mixed_direct = 1 are compared with those of 0")
    if a.lib:
        from mgroms_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    torch.cuda.set_device(0)
    rows = []
    for c in a.cases:
        dims, method = c.split(":")
        nx, ny, nz = (int(x) for x in dims.split("x"))
        rows += run_case(nx, ny, nz, method, a.maxite, reps=a.reps, tolerance=not a.iteration_only, rings=rings, directs=directs)
    print(f"\n{'case':>14} {'meth':>4} {'prec':>4} {'tail':>4} {'ring':>4} {'drct':>4} {'ms/it':>8} {'min':>8} {'max':>8} {'launches':>8}" + ("" if a.iteration_only else f" {'ms->1e-6':>9} {'it':>3} {'ms->1e-12':>10} {'it':>3}"))
    for r in rows:
        tail = "-" if r["mixed_tail"] is None else r["mixed_tail"]
        ring = "-" if r["mixed_ring"] is None else r["mixed_ring"]
        direct = "-" if r["mixed_direct"] is None else r["mixed_direct"]
        line = f"{r['case']:>14} {r['method']:>4} {r['cycle_precision']:>4} {tail:>4} {ring:>4} {direct:>4} {r['ms_per_iteration']:8.3f} {r['ms_min']:8.3f} {r['ms_max']:8.3f} {r['launches_per_iteration']:8d}"
        if not a.iteration_only:
            line += f" {r['ms_to_1e-6']:9.2f} {r['iterations_to_1e-6']:3d} {r['ms_to_1e-12']:10.2f} {r['iterations_to_1e-12']:3d}"
        print(line)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
