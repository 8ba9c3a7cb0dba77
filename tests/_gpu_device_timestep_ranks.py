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
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rank_zeta(nx, ny, npx, npy, rank, ph, seed):
    """a moving free surface, smooth in the GLOBAL indices plus noise of this rank's own (the halos are the library's to fill)"""
    pi, pj = rank % npx, rank // npx
    i = np.arange(nx + 2, dtype=np.float64)[:, None] + pi * nx
    j = np.arange(ny + 2, dtype=np.float64)[None, :] + pj * ny
    rng = np.random.default_rng(seed + rank)
    return 0.8 * np.sin(2 * np.pi * i / (npx * nx) + ph) * np.cos(2 * np.pi * j / (npy * ny) - ph) + 0.05 * rng.standard_normal((nx + 2, ny + 2))


def rank_main(rank, tw, cfg, o, results):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import check, lib
    from mgroms_amd.parallel import ThreadComm
    from oracle.mgoracle import seamount_geometry
    npx, npy, nx, ny, nz, nsmall = cfg
    try:
        torch.cuda.set_device(0)
        torch.cuda.set_stream(torch.cuda.Stream())
        L = lib()
        inst = L.mgx_instance_create()
        check(L.mgx_instance_select(inst))
        nhydro.set_verbose(0)
        comm = ThreadComm(tw, rank, p2p=False)
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
        tw.barrier.wait(60)
        mg.nhydro_clean()
        check(L.mgx_instance_select(0))
        check(L.mgx_instance_destroy(inst))
        results[rank] = f"rank {rank} ok gathered_levels={gathered}"
    except BaseException:
        results[rank] = "rank %d FAILED:\n%s" % (rank, traceback.format_exc())
        try:
            tw.barrier.abort()
        except Exception:
            pass


def main():
    npx, npy, nx, ny, nz, nsmall = (int(a) for a in sys.argv[1:7])
    world = npx * npy
    os.environ["OMP_NUM_THREADS"] = "8"
    # one hardware queue per rank at least, set before HIP initialises (tests/_gpu_thread_ranks.py says why)
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(8, 3 * world)))
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("MGX_TEST_WATCHDOG", "100")), exit=True)
    import torch
    torch.cuda.set_device(0)
    from mgroms_amd.parallel import ThreadWorld
    from oracle.mgoracle import Oracle, seamount_geometry
    o = Oracle(nx, ny, nz, npx, npy, relax_method="FC", nsmall=nsmall)
    for r in range(world):
        dx, dy, _, h = seamount_geometry(nx, ny, npx, npy, r)
        for name, a in (("dx", dx), ("dy", dy), ("zeta", rank_zeta(nx, ny, npx, npy, r, 1.3, 200)), ("h", h)):
            o.field(name, 1, r)[...] = a
    o.matrices(4e3, 0.0, 0.0)
    tw = ThreadWorld(world)
    results = [None] * world
    th = [threading.Thread(target=rank_main, args=(r, tw, (npx, npy, nx, ny, nz, nsmall), o, results), daemon=True) for r in range(world)]
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
