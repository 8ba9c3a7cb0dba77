#!/usr/bin/env python3
"""What option "small_any_nz" buys (include/mgx.h), with device events:
  classes   per class of the new instances (kernel family x nz x threads) a relax call of 3 and of 40 sweeps on a level of that class, per
            mode (FC; RB = the red-black default, the sequential order at speed; RB_parallel = rb_seq 0; RB_exact = rb_exact 1; RB_simple =
            cmatrix 'simple'), option 0 and 1, each --reps times: min, median, max in microseconds and the launches of one call
  solves    a cold solve_p to 1e-10 (seamount, u = v = 0, w = -1) at 512 x 512 x 48 and x 96 on the default hierarchy and x 40 and x 80 with
            "hold_odd_nz" = 1, FC and RB, option 0 and 1: ms and launches per iteration (median of --reps)
--lib PATH loads another build of libmgx.so (the parent commit's, which has no such option: only the option-0 rows are run then), so that the
two builds are timed by the same script on the same card; --merge adds such a document's rows to this one's under "parent".
  python3 scripts/small_any_nz_time.py --out profiles/small_any_nz_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

# class name -> (level-1 size, hold_odd_nz, level of the class, its size)
CLASSES = {
    "wave_nz3_64": ((32, 32, 6), 0, 2, (16, 16, 3)),
    "wave_nz3_256": ((64, 64, 6), 0, 2, (32, 32, 3)),
    "reg_nz5_256": ((32, 32, 10), 1, 2, (16, 16, 5)),
    "reg_nz6_256": ((32, 32, 12), 0, 2, (16, 16, 6)),
    "reg_nz7_256": ((32, 32, 14), 1, 2, (16, 16, 7)),
    "reg_nz5_64": ((32, 32, 10), 1, 3, (8, 8, 5)),
    "small_nz5_1024": ((64, 64, 10), 1, 2, (32, 32, 5)),
    "small_nz6_1024": ((64, 64, 12), 0, 2, (32, 32, 6)),
    "small_nz7_1024": ((64, 64, 14), 1, 2, (32, 32, 7)),
}


# mode -> (namelist, options)
MODES = {"FC": (dict(relax_method="FC"), {}), "RB": (dict(relax_method="RB"), {}), "RB_parallel": (dict(relax_method="RB"), {"rb_seq": 0}),
         "RB_exact": (dict(relax_method="RB"), {"rb_exact": 1}), "RB_simple": (dict(relax_method="RB", cmatrix="simple"), {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libmgx.so to time (only option 0 is run)")
    ap.add_argument("--what", nargs="+", default=["classes", "solves"])
    ap.add_argument("--classes", nargs="+", default=list(CLASSES))
    ap.add_argument("--cases", nargs="+", default=["48:0", "96:0", "40:1", "80:1"], help="nz:hold_odd_nz")
    ap.add_argument("--modes", nargs="+", default=list(MODES), help="of the classes")
    ap.add_argument("--methods", nargs="+", default=["FC", "RB"], help="of the solves")
    ap.add_argument("--plane", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maxit", type=int, default=40)
    ap.add_argument("--merge", default=None, help="a document written with --lib: its rows go under \"parent\"")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        import mgroms_amd._lib as _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import resting_column_state, seamount_geometry
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    options = [0] if a.lib else [0, 1]

    def set_small(v):
        if not a.lib:
            nhydro.set_option("small_any_nz", v)

    def init(dims, hold, mode):
        mg.nhydro_clean()
        nhydro.set_option("hold_odd_nz", hold)
        nhydro.set_option("rb_seq", 1); nhydro.set_option("rb_exact", 0)
        for k, v in MODES[mode][1].items():
            nhydro.set_option(k, v)
        mg.nhydro_init(*dims, 1, 1, 0, nhydro.default_params(**MODES[mode][0]))
        mg.nhydro_matrices(*seamount_geometry(dims[0], dims[1], 1, 1, 0), None, 4e3, 0.0, 0.0)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        n0 = nhydro.counters()["launches"]
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), nhydro.counters()["launches"] - n0, out

    doc = {"device": torch.cuda.get_device_name(0), "library": a.lib or "this tree", "reps": a.reps, "warmup": a.warmup, "classes": [], "solves": []}
    try:
        if "classes" in a.what:
            for name in a.classes:
                dims, hold, lev, want = CLASSES[name]
                for method in a.modes:
                    init(dims, hold, method)
                    g = mg.grid(lev)
                    assert (g.nx, g.ny, g.nz) == want, (name, g.nx, g.ny, g.nz)
                    rng = np.random.default_rng(1)
                    g.set("p", rng.standard_normal(g._shape("p"))); g.set("b", rng.standard_normal(g._shape("b"))); mg.fill_halo(lev, "p")
                    for small in options:
                        set_small(small)
                        for sweeps in (3, 40):
                            runs = [timed(lambda: mg.relax(lev, sweeps)) for _ in range(a.warmup + a.reps)][a.warmup:]
                            us = [1e3 * r[0] for r in runs]
                            row = {"class": name, "level": list(want), "mode": method, "small_any_nz": small, "sweeps": sweeps, "launches": runs[0][1],
                                   "us_min": round(min(us), 2), "us_median": round(float(np.median(us)), 2), "us_max": round(max(us), 2)}
                            doc["classes"].append(row)
                            print(json.dumps(row), flush=True)
                    set_small(0)
        if "solves" in a.what:
            nx, ny = a.plane
            for case in a.cases:
                nz, hold = (int(v) for v in case.split(":"))
                u, v, w = resting_column_state(nx, ny, nz)
                for method in a.methods:
                    init((nx, ny, nz), hold, method)
                    nhydro.compute_rhs(u, v, w)
                    for small in options:
                        set_small(small)
                        runs = [timed(lambda: mg.solve_p(1e-10, a.maxit)) for _ in range(a.warmup + a.reps)][a.warmup:]
                        ms = [r[0] for r in runs]
                        it = max(runs[0][2][0], 1)
                        row = {"size": [nx, ny, nz], "hold_odd_nz": hold, "relax_method": method, "small_any_nz": small, "iterations": runs[0][2][0],
                               "final_residual": float(runs[0][2][1][-1]), "levels_nz": [mg.grid(l).nz for l in range(1, mg.nlevs() + 1)],
                               "ms_per_iteration": round(float(np.median(ms)) / it, 4), "ms_per_iteration_min": round(min(ms) / it, 4),
                               "ms_per_iteration_max": round(max(ms) / it, 4), "launches_per_iteration": round(runs[0][1] / it, 1)}
                        doc["solves"].append(row)
                        print(json.dumps(row), flush=True)
                    set_small(0)
    finally:
        mg.nhydro_clean()
        nhydro.set_option("hold_odd_nz", 0); nhydro.set_option("rb_seq", 1); nhydro.set_option("rb_exact", 0)
        set_small(0)
    if a.merge:
        with open(a.merge) as f:
            par = json.load(f)
        doc["parent"] = {"classes": par["classes"], "solves": par["solves"]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
