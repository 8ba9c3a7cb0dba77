"""Option "krylov" on a 2x2 process grid: the four ranks as THREADS of this process (the machinery of tests/_gpu_thread_ranks.py: one
libmgx.so instance, HIP stream and ThreadComm per rank), four colours, cold start.  Prints one JSON line: rank 0's iteration count,
history, restarts and the all-reduce calls the solve made (tests/test_gpu_krylov.py compares them with the one-rank solve).

usage: _gpu_krylov_ranks.py nx ny nz m tol maxite      (nx, ny, nz: one rank's block)"""
import json
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NPX = NPY = 2


def rank_main(rank, tw, cfg, results):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import check, lib
    from mgroms_amd.parallel import ThreadComm
    from mgroms_amd.testcases import seamount_geometry
    nx, ny, nz, m, tol, maxite = cfg
    try:
        torch.cuda.set_device(0)
        torch.cuda.set_stream(torch.cuda.Stream())
        L = lib()
        inst = L.mgx_instance_create()
        check(L.mgx_instance_select(inst))
        nhydro.set_verbose(0)
        comm = ThreadComm(tw, rank, p2p=True)
        mg.nhydro_init(nx, ny, nz, NPX, NPY, rank, nhydro.default_params(relax_method="FC", solver_prec=tol), comm=comm)
        mg.nhydro_matrices(*seamount_geometry(nx, ny, NPX, NPY, rank), None, 4e3, 0.0, 0.0)
        u = np.zeros((nz, ny + 2, nx + 1)); v = np.zeros((nz, ny + 1, nx + 2)); w = -np.ones((nz + 1, ny + 2, nx + 2)); w[0] = 0
        nhydro.compute_rhs(u, v, w)
        nhydro.set_option("krylov", m)
        tw.barrier.wait(60)
        a0 = nhydro.counters()["allreduces"]
        n, hist = mg.solve_p(tol, maxite)
        a1 = nhydro.counters()["allreduces"]
        restarts = nhydro.get_option("krylov_restarts")
        tw.barrier.wait(120)
        mg.nhydro_clean()
        check(L.mgx_instance_select(0))
        check(L.mgx_instance_destroy(inst))
        results[rank] = dict(ok=True, n=n, hist=[float(h) for h in hist], restarts=restarts, allreduces=a1 - a0)
    except BaseException:
        results[rank] = dict(ok=False, error=traceback.format_exc())
        try:
            tw.barrier.abort()
        except Exception:
            pass


def main():
    nx, ny, nz, m = (int(a) for a in sys.argv[1:5])
    tol, maxite = float(sys.argv[5]), int(sys.argv[6])
    world = NPX * NPY
    os.environ["OMP_NUM_THREADS"] = "8"
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(8, 3 * world)))  # one hardware queue per rank and stream: see tests/_gpu_thread_ranks.py
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("MGX_TEST_WATCHDOG", "100")), exit=True)
    import torch
    torch.cuda.set_device(0)
    from mgroms_amd.parallel import ThreadWorld
    tw = ThreadWorld(world)
    results = [None] * world
    th = [threading.Thread(target=rank_main, args=(r, tw, (nx, ny, nz, m, tol, maxite), results), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(90)
    bad = [r for r in range(world) if results[r] is None or not results[r]["ok"]]
    for r in bad:
        print(f"rank {r}: " + (results[r]["error"] if results[r] else "did not finish"), file=sys.stderr)
    if not bad:
        same = all(results[r]["hist"] == results[0]["hist"] and results[r]["n"] == results[0]["n"] for r in range(world))
        print(json.dumps(dict(results[0], same_on_all_ranks=same)))
    sys.stdout.flush()
    os._exit(1 if bad else 0)


if __name__ == "__main__":
    main()
