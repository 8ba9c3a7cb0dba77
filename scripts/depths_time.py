#!/usr/bin/env python3
"""What the matrices from the caller's own depths cost, at 512x512x64 and 512x1024x128.  Every figure is the median of
--reps (20) calls after a warm-up, taken with device events around a call that waits for the device.  Each library is loaded in a process
of its own (a child of this script, one at a time; a child that fails ends the run).

  refresh     nhydro_update_depths_device from the library's dense layout and from the model's i-fastest padded arrays (two ghost cells per
              side, an odd pitch), against nhydro_update_zeta_device of the PARENT commit's library (and of this one)
  set_up      nhydro_matrices of this library against the parent's, with the launches and halo fills mgx_counters reports for one call (the
              feature unused: they must be equal), and nhydro_matrices_depths_device beside them
  iteration   one solve_p iteration (solver_prec = 1e-30), four colours and the red-black default, after nhydro_matrices and after a depth
              set-up on the SAME depths: what losing the sigma generation costs (at nz >= 32 the colour pass reads the stored coefficients)

  python3 scripts/depths_time.py --parent-lib PATH/libmgx.so [--out profiles/depths_time.json]
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
GHOST = 2
DEPTH_SYMBOLS = ("mgx_depth_strides_check", "mgx_matrices_depths", "mgx_matrices_depths_device", "mgx_update_depths_device", "mgx_depths_launch")


def child(a):
    from mgroms_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    have = ctypes.CDLL(_lib.LIB_PATH)
    depths = all(hasattr(have, s) for s in DEPTH_SYMBOLS)
    if not depths:   # the parent's library: the table without the entries it does not have
        for s in DEPTH_SYMBOLS:
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

    def counted(fn):
        c0 = nhydro.counters()
        fn()
        c1 = nhydro.counters()
        return {k: c1[k] - c0[k] for k in ("launches", "halo_fills")}

    out = {"library": "given with --lib" if a.lib else "mgroms_amd/libmgx.so of this tree", "has_depth_entries": depths, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for nx, ny, nz in SHAPES:
        key = "%dx%dx%d" % (nx, ny, nz)
        rec = out["shapes"][key] = {}
        geo = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in seamount_geometry(nx, ny, 1, 1, 0)]
        dx, dy, zeta, h = geo
        rng = np.random.default_rng(1)
        b = rng.standard_normal((nx + 2, ny + 2, nz))
        for method in ("FC", "RB"):
            r = rec[method] = {}
            mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, solver_prec=1e-30))
            sigma = lambda: nhydro.nhydro_matrices_device(dx, dy, zeta, h, None, 4e3, 0.0, 0.0)
            sigma()
            r["matrices"] = dict(timed(sigma), **counted(sigma))
            r["update_zeta"] = dict(timed(lambda: nhydro.nhydro_update_zeta_device(zeta)), **counted(lambda: nhydro.nhydro_update_zeta_device(zeta)))
            g = mg.grid(1)
            g.set("b", b)
            r["iteration_after_matrices"] = timed(lambda: mg.solve_p(1e-30, 1))
            if depths:
                zr, zw = torch.from_numpy(g.zr).cuda(), torch.from_numpy(g.zw).cuda()
                pitch = nx + 2 * GHOST
                pitch += 1 - pitch % 2
                ZR = torch.zeros((nz, ny + 2 * GHOST, pitch), dtype=torch.float64, device="cuda")
                ZW = torch.zeros((nz + 1, ny + 2 * GHOST, pitch), dtype=torch.float64, device="cuda")
                vr, vw = ZR[:, GHOST:GHOST + ny, GHOST:GHOST + nx], ZW[:, GHOST:GHOST + ny, GHOST:GHOST + nx]
                vr.copy_(zr[2:-2, 2:-2].permute(2, 1, 0)); vw.copy_(zw[2:-2, 2:-2].permute(2, 1, 0))
                dense = lambda: nhydro.nhydro_matrices_depths_device(dx, dy, zr, zw)
                dense()
                r["matrices_depths"] = dict(timed(dense), **counted(dense))
                r["update_depths_dense"] = dict(timed(lambda: nhydro.nhydro_update_depths_device(zr, zw)), **counted(lambda: nhydro.nhydro_update_depths_device(zr, zw)))
                r["update_depths_strided"] = dict(timed(lambda: nhydro.nhydro_update_depths_device(vr, vw)), **counted(lambda: nhydro.nhydro_update_depths_device(vr, vw)))
                r["depth_bytes_in"] = int((zr[2:-2, 2:-2].numel() + zw[2:-2, 2:-2].numel()) * 8)
                g.set("b", b)
                r["iteration_after_depths"] = timed(lambda: mg.solve_p(1e-30, 1))
                del zr, zw, ZR, ZW, vr, vw
            mg.nhydro_clean()
        print(key, json.dumps(rec), flush=True)
    with open(a.child_out, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libmgx.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depths_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--lib")
    ap.add_argument("--child-out")
    a = ap.parse_args()
    if a.child_out:
        return child(a)
    runs = [("this", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    res = {"unit": "ms per call, device events around a call that waits for the device; median, min, max of %d after 3 warm-up calls" % a.reps, "runs": {}}
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
    """the rows DESIGN.md 6.4 quotes"""
    runs = res["runs"]
    s = res["summary"] = {}
    for key, rec in runs["this"]["shapes"].items():
        for method, r in rec.items():
            row = s.setdefault(key, {}).setdefault(method, {})
            med = lambda name: r[name]["median"]
            row["update_depths_dense_ms"], row["update_depths_strided_ms"], row["update_zeta_this_ms"] = med("update_depths_dense"), med("update_depths_strided"), med("update_zeta")
            row["matrices_this_ms"], row["matrices_depths_ms"] = med("matrices"), med("matrices_depths")
            row["iteration_after_matrices_ms"], row["iteration_after_depths_ms"] = med("iteration_after_matrices"), med("iteration_after_depths")
            row["iteration_depths_over_matrices"] = med("iteration_after_depths") / med("iteration_after_matrices")
            if "parent" in runs:
                p = runs["parent"]["shapes"][key][method]
                row["update_zeta_parent_ms"], row["matrices_parent_ms"] = p["update_zeta"]["median"], p["matrices"]["median"]
                row["iteration_after_matrices_parent_ms"] = p["iteration_after_matrices"]["median"]
                row["update_depths_dense_over_parent_update_zeta"] = med("update_depths_dense") / p["update_zeta"]["median"]
                row["update_depths_strided_over_parent_update_zeta"] = med("update_depths_strided") / p["update_zeta"]["median"]
                row["matrices_counters_equal_parent"] = all(r["matrices"][k] == p["matrices"][k] and r["update_zeta"][k] == p["update_zeta"][k] for k in ("launches", "halo_fills"))
    print(json.dumps(s, indent=1))


if __name__ == "__main__":
    main()
