#!/usr/bin/env python3
"""What the view entries cost and save: the resident time step on the model's own padded arrays against the densely packed
arrays, at 512x512x64 and 512x1024x128, float64 and float32, four colours.  Every figure is the median of --reps (20) calls after a warm-up,
taken with device events around a call that waits for the device.  Each library is loaded in a process of its own (a child of this script,
one at a time; a child that fails ends the run).

  (a) the dense entries on the PARENT commit's library (two processes: their difference is the run-to-run spread a row is judged by) and on
      this one:  rhs_correct = nhydro_solve_device with solver_maxiter = 0 (compute_rhs + correct_uvw),  solve = nhydro_solve_device with
      two iterations (solver_prec = 1e-30, so that every call does the same work)
  (b) the view entries of this library on a state padded as CROCO pads a GLOBAL_2D_ARRAY (three ghost cells per side in i and j, the row pitch
      made odd), against its dense entries
  (c) what a model has to do without them: three gathers (.contiguous()), the dense call, three copy_ back, as one span
  zeta: nhydro_update_zeta_view on a pitched i-fastest array against transpose-gather + nhydro_update_zeta_device

  python3 scripts/state_view_time.py --parent-lib PATH/libmgx.so [--also LABEL=PATH/libmgx.so ...] [--out profiles/state_view_time.json]
The parent's library: `git worktree add DIR HEAD~1 && make -C DIR/mgroms_amd/csrc` (or any build of the commit before this feature)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((512, 512, 64), (512, 1024, 128))
GHOST = 3
VIEW_SYMBOLS = ("mgx_state_strides_check", "mgx_solve_device_view", "mgx_check_nondivergence_device_view", "mgx_update_zeta_device_view")


def child(a):
    from mgroms_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    have = ctypes.CDLL(_lib.LIB_PATH)
    views = all(hasattr(have, s) for s in VIEW_SYMBOLS)
    if not views:   # the parent's library: the table without the entries it does not have
        for s in VIEW_SYMBOLS:
            _lib._SIGS.pop(s, None)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import seamount_geometry
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        t = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return {"median": float(np.median(t)), "min": min(t), "max": max(t)}

    def padded(shape, dtype):
        """the model's array around a logical (nk, nj, ni): three ghost cells per side in j and i, an odd pitch"""
        nk, nj, ni = shape
        pitch = ni + 2 * GHOST
        pitch += 1 - pitch % 2
        return torch.zeros((nk, nj + 2 * GHOST, pitch), dtype=dtype, device="cuda")

    out = {"library": "given with --lib" if a.lib else "mgroms_amd/libmgx.so of this tree", "has_view_entries": views, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for nx, ny, nz in SHAPES:
        key = "%dx%dx%d" % (nx, ny, nz)
        rec = out["shapes"][key] = {}
        shapes = ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2))
        rng = np.random.default_rng(1)
        src = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in shapes]
        for mode, par in (("rhs_correct", dict(solver_prec=1e-10, solver_maxiter=0)), ("solve", dict(solver_prec=1e-30, solver_maxiter=2))):
            mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method="FC", **par))
            mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
            if mode == "rhs_correct":
                nhydro.set_option("warm_start", 1)   # no cold-start clearing of p either: the two model kernels and their transposes
            for dname, dtype in (("float64", torch.float64), ("float32", torch.float32)):
                r = rec.setdefault(mode, {}).setdefault(dname, {})
                dense = [t.to(dtype) for t in src]
                r["dense"] = timed(lambda: nhydro.nhydro_solve_device(*dense))
                if views:
                    store = [padded(s, dtype) for s in shapes]
                    # u(1:nx+1, 0:ny+1), v(0:nx+1, 1:ny+1), w(0:nx+1, 0:ny+1) inside arrays that start at i, j = -2
                    vw = [store[0][:, 2:2 + ny + 2, 3:3 + nx + 1], store[1][:, 3:3 + ny + 1, 2:2 + nx + 2], store[2][:, 2:2 + ny + 2, 2:2 + nx + 2]]
                    for v, t in zip(vw, src):
                        v.copy_(t)
                    assert all(tuple(v.shape) == s and v.stride(2) == 1 and v.stride(1) % 2 == 1 for v, s in zip(vw, shapes))
                    r["view"] = timed(lambda: nhydro.nhydro_solve_view(*vw))

                    def gather_call_scatter():
                        g = [v.contiguous() for v in vw]
                        nhydro.nhydro_solve_device(*g)
                        for v, t in zip(vw, g):
                            v.copy_(t)
                    r["gather_dense_scatter"] = timed(gather_call_scatter)
                    esz = dense[0].element_size()
                    r["state_bytes"] = int(sum(t.numel() for t in dense) * esz)
                    del store, vw
                del dense
            if mode == "solve" and views:   # the refresh, on the hierarchy that is there
                z = torch.from_numpy(seamount_geometry(nx, ny, 1, 1, 0)[2]).cuda()   # (nx+2, ny+2), j fastest: the dense entry's layout
                zs = padded((1, ny, nx), torch.float64)[0]   # the model's zeta(-2:nx+3, -2:ny+3), pitch nx + 7
                zv = zs[2:2 + ny + 2, 2:2 + nx + 2]          # zeta(0:nx+1, 0:ny+1) of it
                zv.copy_(z.T)
                rec["zeta"] = {"dense": timed(lambda: nhydro.nhydro_update_zeta_device(z)),
                               "view": timed(lambda: nhydro.nhydro_update_zeta_view(zv)),
                               "transpose_gather_dense": timed(lambda: nhydro.nhydro_update_zeta_device(zv.T.contiguous()))}
            nhydro.set_option("warm_start", 0)
            mg.nhydro_clean()
        print(key, json.dumps(rec), flush=True)
    with open(a.child_out, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libmgx.so built from the parent commit")
    ap.add_argument("--also", action="append", default=[], help="LABEL=PATH: one more library to time the dense entries of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_view_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--lib")
    ap.add_argument("--child-out")
    a = ap.parse_args()
    if a.child_out:
        return child(a)
    runs = [("this", None)] + ([("parent_1", a.parent_lib), ("parent_2", a.parent_lib)] if a.parent_lib else [])
    runs += [tuple(x.split("=", 1)) for x in a.also]
    res = {"unit": "ms per call, device events around a call that waits for the device; median, min, max of %d after 3 warm-up calls" % a.reps,
           "relax_method": "FC", "runs": {}}
    tmp = a.out + ".part"
    for label, lib in runs:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child-out", tmp, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        print("----", label, lib or "(the tree's library)", flush=True)
        r = subprocess.run(cmd)
        if r.returncode != 0:
            sys.exit("%s: the child ended with status %d; nothing more is started" % (label, r.returncode))
        with open(tmp) as f:
            res["runs"][label] = json.load(f)
        os.remove(tmp)
    summarise(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def summarise(res):
    """the rows DESIGN.md 6.3 quotes: (a) this library's dense entries against the parent's two processes, (b) view against dense, (c) view
    against gather + dense + scatter"""
    runs = res["runs"]
    s = res["summary"] = {}
    for key, rec in runs["this"]["shapes"].items():
        for mode in ("rhs_correct", "solve"):
            for dname, r in rec[mode].items():
                row = s.setdefault(key, {}).setdefault(mode, {}).setdefault(dname, {})
                if "parent_1" in runs:
                    p = [runs[q]["shapes"][key][mode][dname]["dense"]["median"] for q in ("parent_1", "parent_2")]
                    lo, hi = min(p), max(p)
                    row["dense_parent"] = p
                    row["dense_this"] = r["dense"]["median"]
                    row["dense_this_over_parent_mean"] = r["dense"]["median"] / (0.5 * (lo + hi))
                    row["dense_not_slower_than_parent_within_its_spread"] = bool(r["dense"]["median"] <= hi + (hi - lo))   # the spread: the parent's two processes
                    for label in runs:
                        if label not in ("this", "parent_1", "parent_2"):
                            row["dense_" + label] = runs[label]["shapes"][key][mode][dname]["dense"]["median"]
                if "view" in r:
                    row["view_over_dense"] = r["view"]["median"] / r["dense"]["median"]
                    row["view_over_gather_dense_scatter"] = r["view"]["median"] / r["gather_dense_scatter"]["median"]
                    row["second_copy_of_the_state_avoided_bytes"] = r["state_bytes"]
                    row["copy_traffic_avoided_bytes_per_step"] = 4 * r["state_bytes"]   # three gathers and three scatters, each read once and written once
        if "zeta" in rec:
            z = rec["zeta"]
            s[key]["zeta_view_over_transpose_gather_dense"] = z["view"]["median"] / z["transpose_gather_dense"]["median"]
    print(json.dumps(s, indent=1))


if __name__ == "__main__":
    main()
