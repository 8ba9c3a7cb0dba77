#!/usr/bin/env python3
"""Times the set-up half of a time step with device events on the solver's stream, per relax_method:
  (a) nhydro_matrices from host arrays                      -- also runs on a tree without the device entry points (--mode host)
  (b) nhydro_matrices_device from tensors
  (c) nhydro_update_zeta_device, with option "async" = 0 and 1
  (d) a resident step: nhydro_update_zeta_device + nhydro_solve_device, with warm_start = 0 and 1 (u, v, w restored before every step)
(a), (b), (c) alternate inside one repetition loop, so they see the same machine.  Every figure is kept per repetition: `ev_ms` the device
span between two events around the call, `host_ms` the wall clock until the call returned.  One JSON document on stdout or to --out.
  python3 scripts/profile_device_timestep.py 512 512 64 --methods FC RB --reps 20 --warmup 3 --out profiles/device_timestep.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import seamount_geometry  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host


def stats(rows):
    out = {}
    for key, idx in (("ev_ms", 0), ("host_ms", 1)):
        a = np.array([r[idx] for r in rows])
        out[key] = {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "all": [round(float(x), 4) for x in a]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dims", type=int, nargs=3)
    ap.add_argument("--mode", choices=("host", "all"), default="all")
    ap.add_argument("--methods", nargs="+", default=["FC", "RB"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    nx, ny, nz = a.dims
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    doc = {"label": a.label, "dims": [nx, ny, nz], "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "methods": {}}
    dx, dy, _, h = seamount_geometry(nx, ny, 1, 1, 0)
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    zetas = [0.8 * np.sin(2 * np.pi * i / nx + ph) * np.cos(2 * np.pi * j / ny - ph) for ph in (0.0, 0.01)]
    for method in a.methods:
        mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method))
        res = {}
        calls = {"a_matrices_host": lambda q: mg.nhydro_matrices(dx, dy, zetas[q % 2], h, None, 4e3, 0.0, 0.0)}
        if a.mode == "all":
            tdx, tdy, th = (torch.from_numpy(x).cuda() for x in (dx, dy, h))
            tz = [torch.from_numpy(z).cuda() for z in zetas]
            calls["b_matrices_device"] = lambda q: mg.nhydro_matrices_device(tdx, tdy, tz[q % 2], th, None, 4e3, 0.0, 0.0)
            calls["c_update_zeta_device"] = lambda q: mg.nhydro_update_zeta_device(tz[q % 2])

            def c_async(q):
                nhydro.set_option("async", 1)
                try:
                    mg.nhydro_update_zeta_device(tz[q % 2])
                finally:
                    nhydro.set_option("async", 0)
            calls["c_update_zeta_device_async"] = c_async
        rows = {k: [] for k in calls}
        for q in range(a.warmup + a.reps):
            for k, fn in calls.items():
                r = timed(lambda: fn(q))
                nhydro.synchronize()
                if q >= a.warmup:
                    rows[k].append(r)
        for k in calls:
            res[k] = stats(rows[k])
        if a.mode == "all":
            rng = np.random.default_rng(3)
            uvw0 = [torch.from_numpy(rng.standard_normal(s)).cuda() for s in ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2))]
            uvw = [t.clone() for t in uvw0]
            for ws in (0, 1):
                nhydro.set_option("warm_start", ws)
                rws = []
                for q in range(a.warmup + a.reps):
                    for t, t0 in zip(uvw, uvw0):
                        t.copy_(t0)

                    def step():
                        mg.nhydro_update_zeta_device(tz[q % 2])
                        nhydro.nhydro_solve_device(*uvw)
                    r = timed(step)
                    if q >= a.warmup:
                        rws.append(r)
                res["d_resident_step_warm_start_%d" % ws] = stats(rws)
            nhydro.set_option("warm_start", 0)
            res["zeta_refreshes"] = nhydro.get_option("zeta_refreshes")
            res["zeta_chain_launches"] = nhydro.get_option("zeta_chain_launches")
        doc["methods"][method] = res
        mg.nhydro_clean()
    txt = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    for method, res in doc["methods"].items():
        for k, v in res.items():
            if isinstance(v, dict):
                print(f"{a.label} {method} {k}: ev median {v['ev_ms']['median']:.3f} ms [{v['ev_ms']['min']:.3f} .. {v['ev_ms']['max']:.3f}], host median {v['host_ms']['median']:.3f} ms")


if __name__ == "__main__":
    main()
