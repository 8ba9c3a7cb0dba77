"""Option "krylov" on a 2x2 process grid: the four ranks as THREADS of this process (the machinery of tests/_gpu_thread_ranks.py: one
libmgx.so instance, HIP stream and ThreadComm per rank), four colours, cold start.  Prints one JSON line: rank 0's iteration count,
history, restarts and the all-reduce calls the solve made (tests/test_gpu_krylov.py compares them with the one-rank solve).

usage: _gpu_krylov_ranks.py nx ny nz m tol maxite      (nx, ny, nz: one rank's block)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import prepare_thread_rank_process, run_threads, thread_rank   # (tests/ is the script's directory: already on sys.path)
NPX = NPY = 2


def rank_main(rank, tw, cfg):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import resting_column_state, seamount_geometry
    nx, ny, nz, m, tol, maxite = cfg
    with thread_rank(tw, rank, p2p=True) as comm:
        mg.nhydro_init(nx, ny, nz, NPX, NPY, rank, nhydro.default_params(relax_method="FC", solver_prec=tol), comm=comm)
        mg.nhydro_matrices(*seamount_geometry(nx, ny, NPX, NPY, rank), None, 4e3, 0.0, 0.0)
        nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
        nhydro.set_option("krylov", m)
        tw.barrier.wait(60)
        a0 = nhydro.counters()["allreduces"]
        n, hist = mg.solve_p(tol, maxite)
        a1 = nhydro.counters()["allreduces"]
        restarts = nhydro.get_option("krylov_restarts")
    return dict(ok=True, n=n, hist=[float(h) for h in hist], restarts=restarts, allreduces=a1 - a0)


def main():
    nx, ny, nz, m = (int(a) for a in sys.argv[1:5])
    tol, maxite = float(sys.argv[5]), int(sys.argv[6])
    prepare_thread_rank_process(NPX * NPY)

    def finish(results):
        same = all(r["hist"] == results[0]["hist"] and r["n"] == results[0]["n"] for r in results)
        print(json.dumps(dict(results[0], same_on_all_ranks=same)))
    run_threads(NPX * NPY, lambda rank, tw: rank_main(rank, tw, (nx, ny, nz, m, tol, maxite)), finish)


if __name__ == "__main__":
    main()
