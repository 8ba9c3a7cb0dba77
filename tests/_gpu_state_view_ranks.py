"""One rank of the view entries on a process grid (tests/test_gpu_state_view.py): this rank's block of one global u, v, w, once as
contiguous tensors through nhydro_check_nondivergence_device / nhydro_solve_device and once as views of padded, sentinel-filled storage
through the view entries -- b, p and u, v, w bit for bit the same, the padding untouched, for float64 and float32.  Both calls are
collective, and every rank makes them in the same order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import gloo_rank   # (tests/ is the script's directory: already on sys.path)
from _problem import _geometry, problem
from _state_view import bits, padded, padding_untouched


def main():
    rank, world, npx, npy, port, nx, ny, nz = (int(a) for a in sys.argv[1:9])
    with gloo_rank(rank, world, port):
        line = rank_main(rank, npx, npy, nx, ny, nz)
    print(f"rank {rank} ok {line}")


def rank_main(rank, npx, npy, nx, ny, nz):
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    nhydro.set_verbose(0)
    pr = problem((npx * nx, npy * ny, nz), relax_method="FC", solver_prec=1e-9, solver_maxiter=3, nsmall=8, ns_coarsest=6)
    mg.nhydro_init(nx, ny, nz, npx, npy, rank, nhydro.default_params(**pr.par), comm=Comm(device="cuda", p2p=True))
    mg.nhydro_matrices(*_geometry(pr.geom, nx, ny, npx, npy, rank), None, *pr.sigma)
    # one global field, cut per rank: the copies of a shared face and of the halo rows agree
    g = np.random.default_rng(777)
    glob = tuple(g.uniform(-1, 1, s) for s in ((nz, npy * ny + 2, npx * nx + 1), (nz, npy * ny + 1, npx * nx + 2), (nz + 1, npy * ny + 2, npx * nx + 2)))
    qj, qi = (rank // npx) * ny, (rank % npx) * nx
    done = []
    for dtype in (np.float64, np.float32):
        mine = tuple(np.ascontiguousarray(a[:, qj:qj + ny + ey, qi:qi + nx + ex].astype(dtype)) for a, ex, ey in zip(glob, (1, 2, 2), (2, 1, 2)))
        dense = [torch.from_numpy(a).cuda() for a in mine]
        stores, views = zip(*(padded(torch, a) for a in mine))
        nhydro.nhydro_check_nondivergence_device(*dense)
        b0 = mg.grid(1).b
        nhydro.nhydro_check_nondivergence_view(*views)
        assert np.array_equal(mg.grid(1).b, b0) and np.any(b0 != 0), (rank, dtype)
        nhydro.nhydro_solve_device(*dense)
        b0, p0 = mg.grid(1).b, mg.grid(1).p
        nhydro.nhydro_solve_view(*views)
        assert np.array_equal(mg.grid(1).b, b0) and np.array_equal(mg.grid(1).p, p0) and np.any(p0 != 0), (rank, dtype)
        for name, a, d, st, v in zip("uvw", mine, dense, stores, views):
            assert torch.equal(bits(torch, v), bits(torch, d)), (rank, dtype, name, int((bits(torch, v) != bits(torch, d)).sum()))
            assert not torch.equal(bits(torch, d), bits(torch, torch.from_numpy(a).cuda())), (rank, dtype, name, "the solve corrected nothing")
            assert padding_untouched(torch, st, v) == (True, 0), (rank, dtype, name)
        done.append(np.dtype(dtype).name)
    mg.nhydro_clean()
    return "views=" + ",".join(done)


if __name__ == "__main__":
    main()
