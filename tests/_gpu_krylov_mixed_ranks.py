"""Option "krylov_precision" = 32 on a 2x2 process grid: the four ranks as THREADS of this process (the machinery of
tests/_gpu_thread_ranks.py: one libmgx.so instance, HIP stream and ThreadComm per rank).  Every rank sets "krylov" = 4 and
"krylov_precision" = 32 and calls solve_p, which must refuse.  Prints one JSON line: the four error texts.

usage: _gpu_krylov_mixed_ranks.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import prepare_thread_rank_process, run_threads, thread_rank   # (tests/ is the script's directory: already on sys.path)
NPX = NPY = 2
NX, NY, NZ = 32, 32, 8


def rank_main(rank, tw):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import MgxError
    from mgroms_amd.testcases import resting_column_state, seamount_geometry
    with thread_rank(tw, rank, p2p=True) as comm:
        mg.nhydro_init(NX, NY, NZ, NPX, NPY, rank, nhydro.default_params(relax_method="FC", solver_prec=1e-8), comm=comm)
        mg.nhydro_matrices(*seamount_geometry(NX, NY, NPX, NPY, rank), None, 4e3, 0.0, 0.0)
        nhydro.compute_rhs(*resting_column_state(NX, NY, NZ))
        nhydro.set_option("krylov", 4)
        nhydro.set_option("krylov_precision", 32)
        tw.barrier.wait(60)
        try:
            mg.solve_p(1e-8, 10)
            text = "NOT REFUSED"
        except MgxError as e:
            text = str(e)
    return text


def main():
    prepare_thread_rank_process(NPX * NPY)
    run_threads(NPX * NPY, rank_main, finish=lambda texts: print(json.dumps(texts)))


if __name__ == "__main__":
    main()
