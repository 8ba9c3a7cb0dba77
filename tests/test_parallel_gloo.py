"""world_size 2 and 4 gloo runs (CPU) of the multi-GPU transport layer: halo exchange, all-reduce and the colour-group
all-gather through the C callbacks of mgroms_amd.parallel.Comm, checked against the oracle's emulated MPI."""
import os

import pytest

from _ranks import free_port, run_process_ranks

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2), (2, 2)])
def test_transport_gloo(npx, npy):
    import __graft_entry__ as g
    g.build()
    world = npx * npy
    run_process_ranks(os.path.join(HERE, "_gloo_worker.py"), world, (world, npx, npy, free_port()), timeout=180)
