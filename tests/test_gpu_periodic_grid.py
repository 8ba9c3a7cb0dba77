"""Option "periodic" on a process grid (include/mgx.h; DESIGN.md sections 1 and 5): the wrap across ranks.

One process per rank on the shared card, at most four, gloo with host staging (tests/_gpu_periodic_grid_worker.py).  The CPU oracle has
closed walls only; the yardstick is the one-rank periodic solve, which tests/test_gpu_periodic.py pins and which four colours reproduce
bit for bit on every decomposition: each worker solves the global problem on one rank first, then its rank of the grid, and compares
h, zr, cA on every level (halos included wherever a halo cell has a one-rank counterpart: the worker's docstring names the three kinds
that have none; the block located from mgx_level_info), b, p after three iterations (bit for bit, halos included) and the residual
history (1e-12 relative).

Measured on the MI355X: red-black in the sequential order against the plane loop <= 7.7e-16 of max|p| on every level (bound 1e-12); GS on
the grid 16 iterations, 2.9e-11 and 5.7e-11 of max|p| from the one-rank four-colour solution per rank, d0 = 1.6e-10 (bound 16 d0); the
operator identity through the model calls per rank <= 6.1e-16 (bound 3.5e-14)."""
import os
import subprocess
import sys

import pytest

from _ranks import free_port, run_process_ranks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


CASES = [
    # npx, npy, block, nsmall, periodic, method, options of the worker
    (2, 1, (32, 32, 8), 8, 1, "FC", "hooks+refuse"),   # E and W are one peer; the gathered level has only itself as neighbour; pushes, then hooks
    (1, 2, (16, 32, 8), 8, 1, "FC", "count"),           # mixed level: self in i, a rank in j; S, SW, SE are one peer; ragged block; one launch per fill
    (2, 2, (32, 32, 16), 8, 3, "FC", "hooks"),          # three peers, all four corners the diagonal rank; pushes, then hooks
    (2, 2, (32, 32, 16), 32, 1, "FC", ""),              # every coarse level gathered; closed and periodic corners on a grid
    (4, 1, (16, 32, 8), 16, 1, "FC", ""),               # distinct E and W peers on level 1; gathers 4 -> 2 -> 1: a gathered level with two ranks
    (2, 1, (64, 128, 64), 8, 1, "FC", "uvw"),           # the bench's matrix-free level-1 kernels with both i sides open; nhydro_solve, the seam face
    (2, 2, (16, 16, 8), 8, 3, "FC", "bmask"),           # an island across a rank seam and the wrap seam: rmask, cA, p
    (2, 1, (32, 32, 16), 8, 1, "RB", "rbseq"),          # red-black in the sequential order against rb_exact on the same grid, every level
    (2, 1, (32, 32, 16), 8, 1, "GS", "gs"),             # GS to 1e-11 on the grid within 16 x d0 of the one-rank FC solution
    (2, 2, (32, 32, 16), 8, 3, "FC", "shift"),          # a roll by one block moves the outputs one rank east; the operator identity per rank
]


def _id(c):
    return "%dx%d-%dx%dx%d-nsmall%d-per%d-%s%s" % (c[0], c[1], *c[2], c[3], c[4], c[5], "-" + c[6] if c[6] else "")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_periodic_grid(case):
    npx, npy, (nx, ny, nz), nsmall, per, method, opt = case
    world = npx * npy
    run_process_ranks(os.path.join(HERE, "_gpu_periodic_grid_worker.py"), world, (world, npx, npy, free_port(), nx, ny, nz, nsmall, per, method, opt))


def test_periodic_4x2_ranks_in_one_process():
    """4 x 2 ranks of 16 x 16 x 16, nsmall = 8, periodic = 3, as threads of one process (tests/_gpu_periodic_thread_ranks.py): every
    rank's level-1 p against the one-rank solve, through the pointer-connected pushes"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_periodic_thread_ranks.py"), "4", "2", "16", "16", "16", "8", "3"],
                         capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-3000:]
    for r in range(8):
        assert f"rank {r} ok" in out.stdout
