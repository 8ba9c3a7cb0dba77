"""The set-up half of a device-resident time step on a process grid (tests/test_gpu_device_timestep.py): the ranks run as THREADS of
this one process, as in tests/_gpu_thread_ranks.py -- each with its own libmgx.so instance, HIP stream and ThreadComm hooks.  Every
rank calls nhydro_matrices_device with one zeta and nhydro_update_zeta_device with another; zeta, zw and cA of every level (gathered
ones included) must then equal the oracle's emulated ranks built with the second zeta, and the one-launch 2-D path must not have been
taken (levels with neighbours or a gather keep one coarsening, one all-gather and one halo fill per level).

A rank that fails aborts the barrier the others wait on and starts nothing more on the GPU; the threads are joined with a bound and a
watchdog ends the process if a collective is stuck.  The test runs this file under `timeout`.

usage: _gpu_device_timestep_ranks.py npx npy nx ny nz nsmall"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import prepare_thread_rank_process, run_threads, thread_rank   # (tests/ is the script's directory: already on sys.path)


def rank_zeta(nx, ny, npx, npy, rank, ph, seed):
    """a moving free surface, smooth in the GLOBAL indices plus noise of this rank's own (the halos are the library's to fill)"""
    pi, pj = rank % npx, rank // npx
    i = np.arange(nx + 2, dtype=np.float64)[:, None] + pi * nx
    j = np.arange(ny + 2, dtype=np.float64)[None, :] + pj * ny
    rng = np.random.default_rng(seed + rank)
    return 0.8 * np.sin(2 * np.pi * i / (npx * nx) + ph) * np.cos(2 * np.pi * j / (npy * ny) - ph) + 0.05 * rng.standard_normal((nx + 2, ny + 2))


def rank_main(rank, tw, cfg, o):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from oracle.mgoracle import seamount_geometry
    npx, npy, nx, ny, nz, nsmall = cfg
    with thread_rank(tw, rank, p2p=False) as comm:
        mg.nhydro_init(nx, ny, nz, npx, npy, rank, nhydro.default_params(relax_method="FC", nsmall=nsmall), comm=comm)
        dx, dy, _, h = seamount_geometry(nx, ny, npx, npy, rank)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        mg.nhydro_matrices_device(dev(dx), dev(dy), dev(rank_zeta(nx, ny, npx, npy, rank, 0.0, 100)), dev(h), None, 4e3, 0.0, 0.0)
        mg.nhydro_update_zeta_device(dev(rank_zeta(nx, ny, npx, npy, rank, 1.3, 200)))
        assert nhydro.get_option("zeta_refreshes") == 1
        assert nhydro.get_option("zeta_chain_launches") == 0
        assert mg.nlevs() == o.nlevs
        gathered = [l for l in range(1, o.nlevs + 1) if o.level_info(l, rank)["gather"]]
        for lev in range(1, o.nlevs + 1):
            g = mg.grid(lev)
            for name in ("zeta", "zw", "cA"):
                a, b = g.get(name), o.field(name, lev, rank)
                assert np.array_equal(a, b), (rank, lev, name, np.argwhere(a != b)[:4].tolist())
    return f"gathered_levels={gathered}"


def main():
    npx, npy, nx, ny, nz, nsmall = (int(a) for a in sys.argv[1:7])
    world = npx * npy
    prepare_thread_rank_process(world)
    from oracle.mgoracle import Oracle, seamount_geometry
    o = Oracle(nx, ny, nz, npx, npy, relax_method="FC", nsmall=nsmall)
    for r in range(world):
        dx, dy, _, h = seamount_geometry(nx, ny, npx, npy, r)
        for name, a in (("dx", dx), ("dy", dy), ("zeta", rank_zeta(nx, ny, npx, npy, r, 1.3, 200)), ("h", h)):
            o.field(name, 1, r)[...] = a
    o.matrices(4e3, 0.0, 0.0)
    run_threads(world, lambda rank, tw: rank_main(rank, tw, (npx, npy, nx, ny, nz, nsmall), o))


if __name__ == "__main__":
    main()
