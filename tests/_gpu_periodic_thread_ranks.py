"""All ranks of a periodic multi-rank GPU solve as THREADS of this one process (tests/test_gpu_periodic_grid.py), each on its own libmgx.so
instance, HIP stream and mgroms_amd.parallel.ThreadComm, as tests/_gpu_thread_ranks.py runs the closed grids.  The yardstick is the
one-rank periodic solve of the global problem (tests/test_gpu_periodic.py pins it), computed on instance 0 before the threads start:
every rank's level-1 p, halos included, is its block of that p indexed with wrap, bit for bit, through the pointer-connected pushes.

usage: _gpu_periodic_thread_ranks.py npx npy nx ny nz nsmall periodic"""
import os
import sys
import threading
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def rank_main(rank, tw, cfg, f, geo, uvw, ref, results):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import check, lib
    from mgroms_amd.parallel import ThreadComm
    npx, npy, nx, ny, nz, nsmall, per = cfg
    try:
        torch.cuda.set_device(0)
        torch.cuda.set_stream(torch.cuda.Stream())
        L = lib()
        inst = L.mgx_instance_create()
        check(L.mgx_instance_select(inst))
        nhydro.set_verbose(0)
        nhydro.set_option("periodic", per)   # per instance
        comm = ThreadComm(tw, rank, p2p=True)
        par = nhydro.default_params(relax_method="FC", solver_prec=1e-30, nsmall=nsmall, ns_coarsest=6)
        mg.nhydro_init(nx, ny, nz, npx, npy, rank, par, comm=comm)
        assert comm.p2p_active, comm.p2p_error
        table = nhydro.level_table_periodic(nx, ny, nz, npx, npy, rank, nsmall, per)
        for lev in range(1, mg.nlevs() + 1):
            assert mg.grid(lev).neighb == table[lev - 1]["neighb"], (rank, lev)
        qi, qj = (rank % npx) * nx, (rank // npx) * ny
        a = {n: f[n][qi:qi + nx + 2, qj:qj + ny + 2].copy() for n in ("dx", "dy", "zeta", "h")}
        mg.nhydro_matrices(a["dx"], a["dy"], a["zeta"], a["h"], None, geo["hc"], geo["theta_b"], geo["theta_s"])
        U, V, W = uvw
        nhydro.compute_rhs(U[:, qj:qj + ny + 2, qi:qi + nx + 1].copy(), V[:, qj:qj + ny + 1, qi:qi + nx + 2].copy(), W[:, qj:qj + ny + 2, qi:qi + nx + 2].copy())
        c0 = nhydro.counters()
        n, hist = mg.solve_p(1e-30, 3)
        c = nhydro.counters()
        assert c["p2p_exchanges"] > c0["p2p_exchanges"]
        NX, NY = npx * nx, npy * ny
        ii = np.arange(qi - 1, qi + nx + 1)
        jj = np.arange(qj - 1, qj + ny + 1)
        ii = ii % NX if per & 1 else ii
        jj = jj % NY if per & 2 else jj
        want = ref["p"][np.ix_(ii + 1, jj + 1)]
        assert n == ref["n"] and np.array_equal(mg.grid(1).p, want), rank
        assert np.all(np.abs(hist - ref["hist"]) <= 1e-12 * np.abs(ref["hist"])), (hist, ref["hist"])
        tw.barrier.wait(120)
        mg.nhydro_clean()
        check(L.mgx_instance_select(0))
        check(L.mgx_instance_destroy(inst))
        results[rank] = f"rank {rank} ok p2p_exchanges={c['p2p_exchanges']}"
    except BaseException:
        results[rank] = "rank %d FAILED:\n%s" % (rank, traceback.format_exc())
        try:
            tw.barrier.abort()
        except Exception:
            pass


def main():
    npx, npy, nx, ny, nz, nsmall, per = (int(a) for a in sys.argv[1:8])
    world = npx * npy
    os.environ["OMP_NUM_THREADS"] = "8"
    # one hardware queue per rank and stream, set before HIP initialises (tests/_gpu_thread_ranks.py has the reason)
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(8, 3 * world)))
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("MGX_TEST_WATCHDOG", "100")), exit=True)  # a stuck collective: all stacks, then exit
    import torch
    torch.cuda.set_device(0)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import ThreadWorld
    from test_gpu_periodic import full2d, geometry, velocities_from, velocity_bases
    NX, NY = npx * nx, npy * ny
    geo = geometry(NX, NY, per)
    f = full2d(geo, per)
    uvw = velocities_from(velocity_bases(NX, NY, nz, per, 5), per)
    nhydro.set_verbose(0)
    nhydro.set_option("periodic", per)
    mg.nhydro_init(NX, NY, nz, 1, 1, 0, nhydro.default_params(relax_method="FC", solver_prec=1e-30, nsmall=nsmall, ns_coarsest=6))
    mg.nhydro_matrices(f["dx"], f["dy"], f["zeta"], f["h"], None, geo["hc"], geo["theta_b"], geo["theta_s"])
    nhydro.compute_rhs(*uvw)
    ref = {}
    ref["n"], ref["hist"] = mg.solve_p(1e-30, 3)
    ref["p"] = mg.grid(1).p
    mg.nhydro_clean()
    nhydro.set_option("periodic", 0)
    tw = ThreadWorld(world)
    results = [None] * world
    cfg = (npx, npy, nx, ny, nz, nsmall, per)
    th = [threading.Thread(target=rank_main, args=(r, tw, cfg, f, geo, uvw, ref, results), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(90)
    bad = [r for r in range(world) if results[r] is None or "ok" not in results[r].split("\n")[0]]
    for r in range(world):
        print(results[r] if results[r] is not None else f"rank {r} did not finish")
    sys.stdout.flush()
    os._exit(1 if bad else 0)  # daemon threads may still sit in a collective after a failure


if __name__ == "__main__":
    main()
