#!/usr/bin/env python3
"""What the wrap across ranks costs (include/mgx.h: option "periodic" on a process grid): a 2 x 1 grid of blocks whose
two ranks SHARE ONE GPU (gloo with host staging for the hooks, hipIpc pushes for the cycle's halos) -- a rehearsal: nothing here crosses
two physical devices, and nobody has measured what the wrap costs over xGMI.

Per configuration -- the closed grid with the library of another tree (--parent-root: a checkout of the parent commit with its library
built), the closed grid with this tree, periodic = 1 with this tree -- and per transport (pushes, hooks): the wall time of Vcycle(1) between
two barriers, median of --reps, and the launches of one level-1 fill_halo("p").  The configurations are run as fresh pairs of processes,
alternated --rounds times, so that a drift of the card shows up in every configuration alike.

  python3 scripts/profile_periodic_grid.py 256 512 64 --parent-root ../parent --out profiles/periodic_grid_time.json"""
import argparse
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def rank_main(a):
    sys.path.insert(0, a.root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE="2", OMP_NUM_THREADS="1")
    import time
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=a.rank, world_size=2)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    from mgroms_amd.testcases import resting_column_state, seamount_geometry
    nx, ny, nz = a.dims
    nhydro.set_verbose(0)
    if a.periodic:
        nhydro.set_option("periodic", a.periodic)
    comm = Comm(device="cuda", p2p=True)
    mg.nhydro_init(nx, ny, nz, 2, 1, a.rank, nhydro.default_params(relax_method="FC"), comm=comm)
    assert comm.p2p_active, comm.p2p_error
    dx, dy, zeta, h = seamount_geometry(nx, ny, 2, 1, a.rank)   # (the halo entries on a periodic side are ignored)
    mg.nhydro_matrices(dx, dy, zeta, h, None, 4e3, 0.0, 0.0)
    nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
    out = {"transport": comm.transport()}
    for name, on in (("pushes", True), ("hooks", False)):
        comm.set_p2p(on)
        ms = []
        for q in range(a.warmup + a.reps):
            torch.cuda.synchronize(); dist.barrier()
            t0 = time.perf_counter()
            mg.Vcycle(1)
            torch.cuda.synchronize(); dist.barrier()
            if q >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        c0 = nhydro.counters()
        mg.fill_halo(1, "p")
        c1 = nhydro.counters()
        out[name] = {"vcycle_ms": {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [round(x, 3) for x in ms]},
                     "level1_halo_fill": {k: c1[k] - c0[k] for k in ("launches", "exchanges", "p2p_exchanges")}}
    comm.set_p2p(True)
    mg.nhydro_clean()
    dist.barrier()
    dist.destroy_process_group()
    if a.rank == 0:
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dims", type=int, nargs=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--periodic", type=int, default=0)
    ap.add_argument("--port", type=int, default=0)
    a = ap.parse_args()
    if a.rank >= 0:
        return rank_main(a)
    configs = ([("closed, parent", a.parent_root, 0)] if a.parent_root else []) + [("closed", ROOT, 0), ("periodic_1", ROOT, 1)]
    doc = {"what": "shared-GPU rehearsal: both ranks of the 2 x 1 grid on ONE device, hooks host-staged over gloo; nothing crossed two physical devices",
           "block": a.dims, "grid": [2, 1], "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "configs": {c[0]: [] for c in configs}}
    for rnd in range(a.rounds):
        for label, root, per in configs:
            s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
            cmd = [sys.executable, os.path.abspath(__file__)] + [str(d) for d in a.dims] + ["--root", os.path.abspath(root), "--periodic", str(per), "--port", str(port),
                                                                                             "--reps", str(a.reps), "--warmup", str(a.warmup)]
            procs = [subprocess.Popen(cmd + ["--rank", str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
            outs = []
            for p in procs:
                try:
                    outs.append(p.communicate(timeout=240)[0])
                except subprocess.TimeoutExpired:
                    for q in procs:
                        q.kill()
                    raise
            if any(p.returncode for p in procs):
                raise SystemExit("%s failed:\n%s" % (label, "\n".join(o[-2000:] for o in outs)))
            res = json.loads([l for l in outs[0].splitlines() if l.startswith("RESULT ")][-1][7:])
            doc["configs"][label].append(res)
            print(rnd, label, {k: (res[k]["vcycle_ms"]["median"], res[k]["level1_halo_fill"]) for k in ("pushes", "hooks")}, flush=True)
    import numpy as np
    doc["summary"] = {label: {k: float(np.median([r[k]["vcycle_ms"]["median"] for r in rows])) for k in ("pushes", "hooks")} for label, rows in doc["configs"].items()}
    print(json.dumps(doc["summary"], indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
