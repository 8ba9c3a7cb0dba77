"""All ranks of a periodic multi-rank GPU solve as THREADS of this one process (tests/test_gpu_periodic_grid.py), each on its own libmgx.so
instance, HIP stream and mgroms_amd.parallel.ThreadComm, as tests/_gpu_thread_ranks.py runs the closed grids.  The yardstick is the
one-rank periodic solve of the global problem (tests/test_gpu_periodic.py pins it), computed on instance 0 before the threads start:
every rank's level-1 p, halos included, is its block of that p indexed with wrap, bit for bit, through the pointer-connected pushes.

usage: _gpu_periodic_thread_ranks.py npx npy nx ny nz nsmall periodic"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ranks import prepare_thread_rank_process, run_threads, thread_rank


def rank_main(rank, tw, cfg, f, geo, uvw, ref):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    npx, npy, nx, ny, nz, nsmall, per = cfg
    with thread_rank(tw, rank, p2p=True) as comm:
        nhydro.set_option("periodic", per)   # per instance
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
    return f"p2p_exchanges={c['p2p_exchanges']}"


def main():
    npx, npy, nx, ny, nz, nsmall, per = (int(a) for a in sys.argv[1:8])
    prepare_thread_rank_process(npx * npy)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
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
    cfg = (npx, npy, nx, ny, nz, nsmall, per)
    run_threads(npx * npy, lambda rank, tw: rank_main(rank, tw, cfg, f, geo, uvw, ref))


if __name__ == "__main__":
    main()
