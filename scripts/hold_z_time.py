#!/usr/bin/env python3
"""What option "hold_z_levels" buys and costs (include/mgx.h), with device events around solve_p, median of --reps:
  per size (default 512 x 512 x 64 and 512 x 512 x 32, seamount, u = v = 0, w = -1), per relax_method (FC, RB), per m (0, the hint of
  mgx_hold_z_hint and the hint - 1 and + 1), per "krylov" (0, 4) and, for m >= 1, per "hold_z_fuse" (1: the down leg of a held pair as one
  kernel, 0: two launches)
    iterations_to_1e-6, iterations_to_1e-10   from the history of ONE cold solve_p to 1e-10 with at most --maxit (50) iterations; null = not reached
    ms_per_iteration, launches_per_iteration  that solve's time and launches over its iterations
  --parent-lib PATH: the m = 0 rows are also taken, in the same run and in a process of its own, from the library of another commit (the
  parent's libmgx.so): "parent" beside "this"; m = 0 must cost nothing, i.e. the two agree within the spread of the repeats.
  python3 scripts/hold_z_time.py --parent-lib /path/to/parent/libmgx.so --out profiles/hold_z_time.json"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(libpath):
    """the package on the library at libpath (None: the tree's own); a library of another commit lacks the newer entries: they are left out"""
    from mgroms_amd import _lib
    if libpath:
        _lib.LIB_PATH = os.path.abspath(libpath)
        import torch  # noqa: F401  (the HIP runtime first, as _lib.lib() does)
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGS if not hasattr(probe, n)]:
            del _lib._SIGS[name]
    import mgroms_amd as mg
    return mg


def first_below(hist, tol):
    for n, r in enumerate(hist):
        if r <= tol:
            return n
    return None


def rows(mg, size, methods, ms_list, krylovs, reps, warmup, maxit, fuse_ab):
    import numpy as np
    import torch
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import resting_column_state, seamount_geometry
    nx, ny, nz = size
    dx, dy, zeta, h = seamount_geometry(nx, ny, 1, 1, 0)
    u, v, w = resting_column_state(nx, ny, nz)
    out = []
    for method in methods:
        for m in ms_list:
            mg.nhydro_clean()
            if m:
                nhydro.set_option("hold_z_levels", m)
            mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method))
            mg.nhydro_matrices(dx, dy, zeta, h, None, 4e3, 0.0, 0.0)
            nhydro.compute_rhs(u, v, w)
            levels = [[mg.grid(l).nx, mg.grid(l).ny, mg.grid(l).nz] for l in range(1, mg.nlevs() + 1)]
            for kr in krylovs:
                for fuse in ((1, 0) if (m and fuse_ab) else (1,)):
                    nhydro.set_option("krylov", kr)
                    if m:
                        nhydro.set_option("hold_z_fuse", fuse)
                    runs = []
                    for _ in range(warmup + reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        n0 = nhydro.counters()["launches"]
                        e0.record()
                        n, hist = mg.solve_p(1e-10, maxit)
                        e1.record()
                        e1.synchronize()
                        runs.append((e0.elapsed_time(e1), nhydro.counters()["launches"] - n0, n, hist))
                    runs = runs[warmup:]
                    per = [r[0] / max(r[2], 1) for r in runs]
                    n, hist = runs[0][2], runs[0][3]
                    row = {"size": [nx, ny, nz], "relax_method": method, "hold_z_levels": m, "krylov": kr, "hold_z_fuse": fuse if m else None,
                           "levels": len(levels), "levels_nz": [l[2] for l in levels], "level_2": levels[1],
                           "iterations": n, "final_residual": float(hist[-1]), "iterations_to_1e-6": first_below(hist, 1e-6), "iterations_to_1e-10": first_below(hist, 1e-10),
                           "ms_per_iteration": round(float(np.median(per)), 4), "ms_per_iteration_min": round(min(per), 4), "ms_per_iteration_max": round(max(per), 4),
                           "launches_per_iteration": round(runs[0][1] / max(n, 1), 1)}
                    out.append(row)
                    print(json.dumps(row), flush=True)
            nhydro.set_option("krylov", 0)
            if m:
                nhydro.set_option("hold_z_fuse", 1); mg.nhydro_clean(); nhydro.set_option("hold_z_levels", 0)
    mg.nhydro_clean()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["512x512x64", "512x512x32"])
    ap.add_argument("--methods", nargs="+", default=["FC", "RB"])
    ap.add_argument("--krylov", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--maxit", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-m0-of", default=None, help="(internal) the child's mode: the m = 0 rows on the library at this path, as JSON lines")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes]
    mg = load(a.only_m0_of)
    import torch
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import seamount_geometry
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    if a.only_m0_of:
        for size in sizes:
            rows(mg, size, a.methods, [0], a.krylov, a.reps, a.warmup, a.maxit, False)
        return
    doc = {"reps": a.reps, "warmup": a.warmup, "maxit": a.maxit, "device": torch.cuda.get_device_name(0), "hints": {}, "this": [], "parent": []}
    for size in sizes:
        dx, dy, _, h = seamount_geometry(size[0], size[1], 1, 1, 0)
        hint = nhydro.hold_z_hint(dx, dy, h, size[2])
        doc["hints"]["x".join(map(str, size))] = hint
        ms_list = sorted({0, max(hint - 1, 0), hint, min(hint + 1, 8)})
        doc["this"] += rows(mg, size, a.methods, ms_list, a.krylov, a.reps, a.warmup, a.maxit, True)
    if a.parent_lib:
        # a fresh process: one library per process (and a process that has initialised the GPU keeps its program)
        cmd = [sys.executable, os.path.abspath(__file__), "--only-m0-of", a.parent_lib, "--sizes", *a.sizes, "--methods", *a.methods,
               "--krylov", *map(str, a.krylov), "--reps", str(a.reps), "--warmup", str(a.warmup), "--maxit", str(a.maxit)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("the run on the parent's library failed")
        doc["parent"] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        # m = 0 must cost nothing: the medians agree within the spread of the repeats
        doc["m0_against_parent"] = []
        for p in doc["parent"]:
            t = next(q for q in doc["this"] if q["hold_z_levels"] == 0 and all(q[k] == p[k] for k in ("size", "relax_method", "krylov")))
            doc["m0_against_parent"].append({"size": p["size"], "relax_method": p["relax_method"], "krylov": p["krylov"],
                                             "this_ms": [t["ms_per_iteration_min"], t["ms_per_iteration"], t["ms_per_iteration_max"]],
                                             "parent_ms": [p["ms_per_iteration_min"], p["ms_per_iteration"], p["ms_per_iteration_max"]],
                                             "same_iterations_and_launches": t["iterations"] == p["iterations"] and t["launches_per_iteration"] == p["launches_per_iteration"],
                                             "within_spread": t["ms_per_iteration_min"] <= p["ms_per_iteration_max"] and p["ms_per_iteration_min"] <= t["ms_per_iteration_max"]})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
