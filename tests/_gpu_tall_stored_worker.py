"""Worker of test_two_wave_blocks_and_streaming_same_words_as_generic_column: MGX_NO_TALL is read once per process, so the generic
column runs in a process of its own.  Masked seamount (bmask, island mask), four colours, one relax(1, 1) from the state of
big_state; prints a digest of p with its halo, the stored tall passes counted and the launches of the call."""
import hashlib
import os
import sys

import numpy as np


def big_state(nx, ny, nz):
    """p and b of the large case: uniform numbers of a fixed seed (cheap to draw at 42 M cells)"""
    r = np.random.default_rng(80)
    shape = (nx + 2, ny + 2, nz)
    return r.random(shape) - 0.5, r.random(shape) - 0.5


def main(nx, ny, nz):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from _problem import gpu_problem
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    gpu_problem(mg, (nx, ny, nz), bmask=True, relax_method="FC", cmatrix="real", solver_prec=1e-10)
    p, b = big_state(nx, ny, nz)
    g = mg.grid(1)
    g.set("p", p); g.set("b", b); mg.fill_halo(1, "p")
    c0 = nhydro.counters()["launches"]
    mg.relax(1, 1)
    print("LAUNCHES", nhydro.counters()["launches"] - c0)
    print("PASSES", nhydro.get_option("tall_stored_passes"))
    print("DIGEST", hashlib.sha256(g.get("p").tobytes()).hexdigest())
    mg.nhydro_clean()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
