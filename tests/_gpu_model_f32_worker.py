"""Worker of test_forced_run_lengths (tests/test_gpu_model_f32.py): MGX_MODEL_KR (the model kernels' run length) is read once per process, so
every run length is a process of its own.  On a float32 state: compute_rhs, then correct_uvw with a random p (nhydro_solve with warm_start
and solver_maxiter = 0), once through the host entries and once through the device entries; writes b and the corrected u, v, w of each,
p, and the u it started from, as .npy files into the directory argv[4]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from _problem import gpu_problem  # noqa: E402

nx, ny, nz = (int(a) for a in sys.argv[1:4])
out = sys.argv[4]
torch.cuda.set_device(0)
nhydro.set_verbose(0)
gpu_problem(mg, (nx, ny, nz), geom="seamount", relax_method="FC", solver_prec=1e-10, solver_maxiter=0)
rng = np.random.default_rng(23)  # the draws of _state32(..., seed=23) in the test
u0, v0, w0 = (rng.standard_normal(s).astype(np.float32) for s in ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2)))
np.save(os.path.join(out, "u0.npy"), u0)
g1 = mg.grid(1)
g1.set("p", np.random.default_rng(29).standard_normal(g1._shape("p")))
mg.fill_halo(1, "p")
p = g1.p
np.save(os.path.join(out, "p.npy"), p)
nhydro.set_option("warm_start", 1)
for entry in ("host", "device"):
    if entry == "host":
        u, v, w = u0.copy(), v0.copy(), w0.copy()
        mg.nhydro_solve(u, v, w)
    else:
        d = [torch.from_numpy(a).cuda() for a in (u0, v0, w0)]
        nhydro.nhydro_solve_device(*d)
        u, v, w = (t.cpu().numpy() for t in d)
    assert np.array_equal(g1.p, p)  # no iteration ran
    for name, a in (("b", g1.b), ("u", u), ("v", v), ("w", w)):
        np.save(os.path.join(out, "%s_%s.npy" % (name, entry)), a)
mg.nhydro_clean()
print("ok")
