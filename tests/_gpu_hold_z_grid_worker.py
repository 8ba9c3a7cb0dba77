"""One rank of a multi-rank GPU solve with option "hold_z_levels" (tests/test_gpu_hold_z.py), in the pattern of _gpu_hold_grid_worker.py.  All ranks share cuda:0 and talk over gloo
with host staging, as in tests/_gpu_periodic_grid_worker.py.

The yardstick is the ONE-RANK held solve of the global problem, which tests/test_gpu_hold_z.py pins: four colours do not depend on
the decomposition, so every rank's b and p, on every level, are bit for bit its block of the one-rank arrays (the block located from
mgx_level_info; a gathered level holds the whole group's block).  Each worker solves the global problem on one rank first, then cleans and
initialises its rank of the grid.  The solve runs through the default transport (the pushes), then again through the exchange hooks.

usage: _gpu_hold_z_grid_worker.py rank world npx npy port nx ny nz nsmall m"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ranks import gloo_rank

TOL_HIST = 1e-12   # p is bit-identical: only the order of the norm's reduction differs (the bound of tests/_gpu_rank_worker.py)


def main():
    rank, world, npx, npy, port, nx, ny, nz, nsmall, m = (int(a) for a in sys.argv[1:11])
    with gloo_rank(rank, world, port):
        rank_main(rank, npx, npy, nx, ny, nz, nsmall, m)
    print(f"rank {rank} ok")


def rank_main(rank, npx, npy, nx, ny, nz, nsmall, m):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    from mgroms_amd.testcases import resting_column_state, seamount_geometry

    nhydro.set_verbose(0)
    NX, NY = npx * nx, npy * ny
    pi, pj = rank % npx, rank // npx
    par = dict(relax_method="FC", solver_prec=1e-30, nsmall=nsmall)

    def rhs(lx, ly):
        nhydro.compute_rhs(*resting_column_state(lx, ly, nz))

    # ---- the yardstick: the global problem on one rank ------------------------------------------------------------------------------
    mg.nhydro_clean()
    nhydro.set_option("hold_z_levels", m)
    mg.nhydro_init(NX, NY, nz, 1, 1, 0, nhydro.default_params(**par))
    mg.nhydro_matrices(*seamount_geometry(NX, NY, 1, 1, 0), None, 4e3, 0.0, 0.0)
    rhs(NX, NY)
    ref = {"nlevs": mg.nlevs(), "b": mg.grid(1).b}
    ref["n"], ref["hist"] = mg.solve_p(1e-30, 3)
    ref["nz"] = [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)]
    ref["p"] = {lev: mg.grid(lev).p for lev in range(1, mg.nlevs() + 1)}
    assert ref["nz"][:m + 1] == [nz] * (m + 1), ref["nz"]   # the first m pairs are held, level 1 -> 2 included
    assert nhydro.get_option("hold_z_fused") > 0              # and their down legs ran as one kernel
    mg.nhydro_clean()

    # ---- this rank of the grid -----------------------------------------------------------------------------------------------------------
    nhydro.set_option("hold_z_levels", m)
    comm = Comm(device="cuda", p2p=True)
    mg.nhydro_init(nx, ny, nz, npx, npy, rank, nhydro.default_params(**par), comm=comm)
    assert comm.p2p_active, comm.p2p_error
    table = nhydro.level_table(nx, ny, nz, npx, npy, rank, nsmall, hold_z_levels=m)
    assert mg.nlevs() == len(table) == ref["nlevs"]
    for lev in range(1, mg.nlevs() + 1):
        gl = mg.grid(lev)
        t = table[lev - 1]
        assert (gl.nx, gl.ny, gl.nz, gl.gather, gl.neighb) == (t["nx"], t["ny"], t["nz"], t["gather"], t["neighb"]), (rank, lev)
        assert gl.nz == ref["nz"][lev - 1]
    assert any(t["gather"] for t in table)
    mg.nhydro_matrices(*seamount_geometry(nx, ny, npx, npy, rank), None, 4e3, 0.0, 0.0)

    def block(lev):
        """(i0, j0): where this rank's block of the level lies in the one-rank level, from mgx_level_info"""
        gl = mg.grid(lev)
        bi = pi // gl.incx if gl.npx > 1 else 0
        bj = pj // gl.incy if gl.npy > 1 else 0
        assert gl.nx * gl.npx == NX >> (lev - 1) and gl.ny * gl.npy == NY >> (lev - 1), (lev, gl.nx, gl.npx)
        return bi * gl.nx, bj * gl.ny

    def same(got, A, lev, what, halo):
        gl = mg.grid(lev)
        i0, j0 = block(lev)
        want = A[i0:i0 + gl.nx + 2, j0:j0 + gl.ny + 2]
        if not halo:
            got, want = got[1:-1, 1:-1], want[1:-1, 1:-1]
        bad = got != want
        assert not bad.any(), (rank, lev, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())

    def check(tag):
        rhs(nx, ny)
        same(mg.grid(1).b, ref["b"], 1, "b " + tag, False)
        n, hist = mg.solve_p(1e-30, 3)
        assert n == ref["n"] == 3, (n, ref["n"])
        assert np.all(np.abs(hist - ref["hist"]) <= TOL_HIST * np.abs(ref["hist"])), (hist, ref["hist"])
        same(mg.grid(1).p, ref["p"][1], 1, "p " + tag, True)     # the halo on a rank seam is the neighbour's interior, on a wall the mirror
        for lev in range(2, mg.nlevs() + 1):
            same(mg.grid(lev).p, ref["p"][lev], lev, "p " + tag, False)
        return nhydro.counters()

    f0 = nhydro.get_option("hold_z_fused")
    c0 = nhydro.counters()
    c1 = check("pushes")
    assert c1["p2p_exchanges"] > c0["p2p_exchanges"]
    comm.set_p2p(False)
    c2 = check("hooks")
    assert c2["p2p_exchanges"] == c1["p2p_exchanges"] and c2["exchanges"] > c1["exchanges"]
    comm.set_p2p(True)
    assert nhydro.get_option("hold_z_fused") > f0   # the down leg of the held pair onto an open coarse level is the fused kernel's too

    mg.nhydro_clean()
    nhydro.set_option("hold_z_levels", 0)


if __name__ == "__main__":
    main()
