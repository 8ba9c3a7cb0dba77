"""nhydro_matrices and a solve in a process of its own (tests/test_gpu_depths.py): "fresh" never sees depths; "after" first sets up and
solves on old-S depths in the same hierarchy.  Prints one line, RESULT <digest of p> <growth of every counter over nhydro_matrices,
compute_rhs and solve_p>, which must not depend on the mode.

usage: _gpu_depths_after_worker.py fresh|after"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    mode = sys.argv[1]
    assert mode in ("fresh", "after")
    import torch
    torch.cuda.set_device(0)
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from _depths import dense, old_s_depths
    from _operator_identity import case_inputs
    from _problem import uvw

    dims = nx, ny, nz = 64, 32, 64     # level 1 generates slots 4 / 7 from the sigma fields: they must be back
    inp = case_inputs(nx, ny, "seamount", stretched=True, curvilinear=True)
    state = uvw(dims, seed=17)
    nhydro.set_verbose(0)
    mg.nhydro_init(*dims, 1, 1, 0, nhydro.default_params(relax_method="FC", solver_prec=1e-10))
    if mode == "after":
        zr, zw = old_s_depths(inp["h"][1:-1, 1:-1], np.zeros((nx, ny)), nz)
        mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw))
        nhydro.compute_rhs(*state)
        mg.solve_p(1e-10, 3)
    c0 = nhydro.counters()
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], None, inp["hc"], inp["theta_b"], inp["theta_s"])
    nhydro.compute_rhs(*state)
    n, hist = mg.solve_p(1e-10, 4)
    c1 = nhydro.counters()
    p = mg.grid(1).p
    assert np.abs(p).max() > 0
    grown = {k: c1[k] - c0[k] for k in sorted(c0)}
    print("RESULT", hashlib.sha256(p.tobytes()).hexdigest(), n, hist.tobytes().hex(), grown)
    mg.nhydro_clean()


if __name__ == "__main__":
    main()
