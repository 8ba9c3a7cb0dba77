#!/usr/bin/env python3
"""What option "periodic" costs today (include/mgx.h), with device events on the solver's stream, median of --reps:
  per relax_method (FC, RB) and per periodic = 0, 1, 3
    solve_p_iteration   (solve_p(1e-30, 3) - solve_p(1e-30, 1)) / 2, "warm_start" on: what one more iteration costs, and its launches
    level1_sweep        relax(1, 1), and its launches
    level1_halo_fill    fill_halo(1, "p") under "async": k_halo_wrap with periodic != 0 (one launch), k_halo_phys with 0
A periodic hierarchy loses the launches that need a closed level (the persistent and one-workgroup relax, the restriction chain, the
direct coarsest solve) and gains a halo fill behind every colour pass: the launch counts beside the times say which of the two it pays for.
  python3 scripts/profile_periodic.py 512 512 64 --out profiles/periodic_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import seamount_geometry  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n0 = nhydro.counters()["launches"]
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), nhydro.counters()["launches"] - n0


def stats(rows):
    a = np.array([r[0] for r in rows])
    return {"ms": {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "all": [round(float(x), 4) for x in a]},
            "launches": sorted({int(r[1]) for r in rows})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dims", type=int, nargs=3)
    ap.add_argument("--methods", nargs="+", default=["FC", "RB"])
    ap.add_argument("--periodic", type=int, nargs="+", default=[0, 1, 3])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nx, ny, nz = a.dims
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    doc = {"dims": [nx, ny, nz], "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "transport": {}, "methods": {}}
    dx, dy, zeta, h = seamount_geometry(nx, ny, 1, 1, 0)   # (the halo entries of a periodic direction are ignored)
    rng = np.random.default_rng(3)
    ub, vb, wb = rng.standard_normal((nz, ny, nx)), rng.standard_normal((nz, ny, nx)), rng.standard_normal((nz + 1, ny, nx))
    u = np.ascontiguousarray(np.pad(np.concatenate([ub, ub[:, :, :1]], axis=2), [(0, 0), (1, 1), (0, 0)], mode="wrap"))
    v = np.ascontiguousarray(np.pad(np.concatenate([vb, vb[:, :1, :]], axis=1), [(0, 0), (0, 0), (1, 1)], mode="wrap"))
    w = np.ascontiguousarray(np.pad(wb, [(0, 0), (1, 1), (1, 1)], mode="wrap"))
    try:
        for method in a.methods:
            doc["methods"][method] = {}
            for per in a.periodic:
                mg.nhydro_clean()
                nhydro.set_option("periodic", per)
                mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method))
                mg.nhydro_matrices(dx, dy, zeta, h, None, 4e3, 0.0, 0.0)
                from mgroms_amd._lib import lib
                doc["transport"][str(per)] = lib().mgx_transport().decode()
                nhydro.compute_rhs(u, v, w)
                nhydro.set_option("warm_start", 1)
                rows = {"solve_p_1": [], "solve_p_3": [], "level1_sweep": [], "level1_halo_fill": []}
                for q in range(a.warmup + a.reps):
                    r = {"solve_p_1": timed(lambda: mg.solve_p(1e-30, 1)), "solve_p_3": timed(lambda: mg.solve_p(1e-30, 3)),
                         "level1_sweep": timed(lambda: mg.relax(1, 1))}
                    nhydro.set_option("async", 1)
                    try:
                        t, n = timed(lambda: [mg.fill_halo(1, "p") for _ in range(10)])
                    finally:
                        nhydro.set_option("async", 0)
                    nhydro.synchronize()
                    r["level1_halo_fill"] = (t / 10, n // 10)
                    if q >= a.warmup:
                        for k in rows:
                            rows[k].append(r[k])
                nhydro.set_option("warm_start", 0)
                res = {k: stats(v_) for k, v_ in rows.items()}
                it = [(r3[0] - r1[0]) / 2 for r1, r3 in zip(rows["solve_p_1"], rows["solve_p_3"])]
                res["solve_p_iteration"] = {"ms": {"median": float(np.median(it)), "min": float(min(it)), "max": float(max(it))},
                                            "launches": sorted({(r3[1] - r1[1]) // 2 for r1, r3 in zip(rows["solve_p_1"], rows["solve_p_3"])})}
                doc["methods"][method]["periodic_%d" % per] = res
                for k in ("solve_p_iteration", "level1_sweep", "level1_halo_fill"):
                    print(f"{method} periodic = {per} {k}: median {res[k]['ms']['median']:.4f} ms, launches {res[k]['launches']}")
    finally:
        mg.nhydro_clean()
        nhydro.set_option("periodic", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
