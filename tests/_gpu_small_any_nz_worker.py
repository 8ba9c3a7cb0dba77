"""One rank of a multi-rank GPU solve with option "small_any_nz" (tests/test_gpu_small_any_nz.py).  All ranks share cuda:0 and talk over
gloo, as in tests/_gpu_hold_grid_worker.py.

2 x 2 ranks of 16 x 16 x 12: level 2 is 8 x 8 x 6 with neighbours -- not a closed level, declined -- and level 3 is 4 x 4 x 3 per rank,
gathered to the closed 8 x 8 x 3 level every rank holds whole, which the option serves.  The yardstick is the same rank's run with option
0: four colours, three iterations, p and b of every level bit for bit.

usage: _gpu_small_any_nz_worker.py rank world npx npy port nx ny nz nsmall"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ranks import gloo_rank


def main():
    rank, world, npx, npy, port, nx, ny, nz, nsmall = (int(a) for a in sys.argv[1:10])
    with gloo_rank(rank, world, port):
        rank_main(rank, npx, npy, nx, ny, nz, nsmall)
    print(f"rank {rank} ok")


def rank_main(rank, npx, npy, nx, ny, nz, nsmall):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    from mgroms_amd.testcases import resting_column_state, seamount_geometry

    nhydro.set_verbose(0)
    par = dict(relax_method="FC", solver_prec=1e-30, nsmall=nsmall)
    runs = []
    for small in (0, 1):
        mg.nhydro_clean()
        nhydro.set_option("small_any_nz", small)
        comm = Comm(device="cuda", p2p=True)
        mg.nhydro_init(nx, ny, nz, npx, npy, rank, nhydro.default_params(**par), comm=comm)
        assert comm.p2p_active, comm.p2p_error
        levels = [mg.grid(lev) for lev in range(1, mg.nlevs() + 1)]
        dims = [(g.nx, g.ny, g.nz, bool(g.gather)) for g in levels]
        assert dims == [(16, 16, 12, False), (8, 8, 6, False), (8, 8, 3, True)], (rank, dims)
        assert any(n >= 0 for n in levels[1].neighb) and all(n < 0 for n in levels[2].neighb), (rank, levels[1].neighb, levels[2].neighb)
        mg.nhydro_matrices(*seamount_geometry(nx, ny, npx, npy, rank), None, 4e3, 0.0, 0.0)
        nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
        c0, l0 = nhydro.get_option("small_any_nz_calls"), nhydro.counters()["launches"]
        n, hist = mg.solve_p(1e-30, 3)
        runs.append(dict(n=n, hist=hist, calls=nhydro.get_option("small_any_nz_calls") - c0, launches=nhydro.counters()["launches"] - l0,
                         p=[g.get("p") for g in levels], b=[g.get("b") for g in levels]))
    mg.nhydro_clean()
    nhydro.set_option("small_any_nz", 0)
    r0, r1 = runs
    assert r0["n"] == r1["n"] == 3
    assert r0["calls"] == 0 and r1["calls"] > 0 and r1["launches"] < r0["launches"], (rank, r0["calls"], r1["calls"], r0["launches"], r1["launches"])
    assert np.all(np.abs(r1["hist"] - r0["hist"]) <= 1e-12 * np.abs(r0["hist"])), (r1["hist"], r0["hist"])
    for lev in range(3):
        for name in ("p", "b"):
            bad = r1[name][lev] != r0[name][lev]
            assert not bad.any(), (rank, lev + 1, name, int(bad.sum()))
    print(f"rank {rank}: {r1['calls']} served calls, launches {r0['launches']} -> {r1['launches']}")


if __name__ == "__main__":
    main()
