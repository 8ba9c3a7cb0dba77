"""Option "krylov_precision" = 32 on a 2x2 process grid: the four ranks as THREADS of this process (the machinery of
tests/_gpu_thread_ranks.py: one libmgx.so instance, HIP stream and ThreadComm per rank).  Every rank sets "krylov" = 4 and
"krylov_precision" = 32 and calls solve_p, which must refuse.  Prints one JSON line: the four error texts.

usage: _gpu_krylov_mixed_ranks.py"""
import json
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NPX = NPY = 2
NX, NY, NZ = 32, 32, 8


def rank_main(rank, tw, results):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import MgxError, check, lib
    from mgroms_amd.parallel import ThreadComm
    from mgroms_amd.testcases import seamount_geometry
    try:
        torch.cuda.set_device(0)
        torch.cuda.set_stream(torch.cuda.Stream())
        L = lib()
        inst = L.mgx_instance_create()
        check(L.mgx_instance_select(inst))
        nhydro.set_verbose(0)
        comm = ThreadComm(tw, rank, p2p=True)
        mg.nhydro_init(NX, NY, NZ, NPX, NPY, rank, nhydro.default_params(relax_method="FC", solver_prec=1e-8), comm=comm)
        mg.nhydro_matrices(*seamount_geometry(NX, NY, NPX, NPY, rank), None, 4e3, 0.0, 0.0)
        u = np.zeros((NZ, NY + 2, NX + 1)); v = np.zeros((NZ, NY + 1, NX + 2)); w = -np.ones((NZ + 1, NY + 2, NX + 2)); w[0] = 0
        nhydro.compute_rhs(u, v, w)
        nhydro.set_option("krylov", 4)
        nhydro.set_option("krylov_precision", 32)
        tw.barrier.wait(60)
        try:
            mg.solve_p(1e-8, 10)
            text = "NOT REFUSED"
        except MgxError as e:
            text = str(e)
        tw.barrier.wait(60)
        mg.nhydro_clean()
        check(L.mgx_instance_select(0))
        check(L.mgx_instance_destroy(inst))
        results[rank] = dict(ok=True, error=text)
    except BaseException:
        results[rank] = dict(ok=False, error=traceback.format_exc())
        try:
            tw.barrier.abort()
        except Exception:
            pass


def main():
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
    th = [threading.Thread(target=rank_main, args=(r, tw, results), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(90)
    bad = [r for r in range(world) if results[r] is None or not results[r]["ok"]]
    for r in bad:
        print(f"rank {r}: " + (results[r]["error"] if results[r] else "did not finish"), file=sys.stderr)
    if not bad:
        print(json.dumps([results[r]["error"] for r in range(world)]))
    sys.stdout.flush()
    os._exit(1 if bad else 0)


if __name__ == "__main__":
    main()
