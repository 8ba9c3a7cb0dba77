"""One rank of the float state on a process grid (tests/test_gpu_model_f32_ranks.py): nhydro_solve on this rank's float32 block of one global
u, v, w, against the oracle's emulated ranks on the promoted field -- b array_equal, u, v, w np.float32 of the oracle's block bit for bit.
The flux faces that neighbours exchange in compute_rhs are fp64 whatever the state is."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import gloo_rank   # (tests/ is the script's directory: already on sys.path)
from _problem import _geometry, load_uvw, oracle_twin, problem


def main():
    rank, world, npx, npy, port, nx, ny, nz = (int(a) for a in sys.argv[1:9])
    with gloo_rank(rank, world, port):
        line = rank_main(rank, npx, npy, nx, ny, nz)
    print(f"rank {rank} ok {line}")


def rank_main(rank, npx, npy, nx, ny, nz):
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    nhydro.set_verbose(0)
    pr = problem((npx * nx, npy * ny, nz), relax_method="FC", solver_prec=1e-9, solver_maxiter=3, nsmall=8, ns_coarsest=6)
    mg.nhydro_init(nx, ny, nz, npx, npy, rank, nhydro.default_params(**pr.par), comm=Comm(device="cuda", p2p=True))
    mg.nhydro_matrices(*_geometry(pr.geom, nx, ny, npx, npy, rank), None, *pr.sigma)
    # one global float field, cut per rank: the copies of a shared face and of the halo rows agree
    g = np.random.default_rng(999)
    glob = tuple(g.standard_normal(s).astype(np.float32)
                 for s in ((nz, npy * ny + 2, npx * nx + 1), (nz, npy * ny + 1, npx * nx + 2), (nz + 1, npy * ny + 2, npx * nx + 2)))
    qj, qi = (rank // npx) * ny, (rank % npx) * nx
    mine = tuple(np.ascontiguousarray(a[:, qj:qj + ny + ey, qi:qi + nx + ex]) for a, ex, ey in zip(glob, (1, 2, 2), (2, 1, 2)))
    before = tuple(a.copy() for a in mine)
    mg.nhydro_solve(*mine)
    o = oracle_twin(pr, npx, npy)
    load_uvw(o, tuple(a.astype(np.float64) for a in glob))
    n, _, _ = o.nhydro_solve()
    assert n >= 1, n
    assert np.array_equal(mg.grid(1).b, o.field("b", 1, rank)), rank
    assert np.array_equal(mg.grid(1).p, o.field("p", 1, rank)), rank
    for name, a, a0 in zip("uvw", mine, before):
        want = o.field(name, 1, rank).astype(np.float32)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), want.view(np.uint32)), (rank, name, int((a.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.any(a.view(np.uint32) != a0.view(np.uint32)), (rank, name)
    mg.nhydro_clean()
    return "nite=%d" % n


if __name__ == "__main__":
    main()
