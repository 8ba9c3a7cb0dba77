"""One plain solve_p in a fresh process, after option "krylov" was set to 4 and back to 0 (touch = 1) or never touched (touch = 0):
prints the history and p as hex, for tests/test_gpu_krylov.py to compare bit for bit.  touch = 2: one solve with "krylov" = 4 under
"tictoc" = 1 and the timer table it leaves (the table is process state that outlives nhydro_clean, so it is filled in a process of its own).
usage: _gpu_krylov_off_worker.py METHOD TOUCH"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

torch.cuda.set_device(0)
import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from _problem import gpu_problem, rhs, uvw  # noqa: E402

meth, touch = sys.argv[1], int(sys.argv[2])
nx, ny, nz = 64, 64, 16
nhydro.set_verbose(0)
gpu_problem(mg, (nx, ny, nz), relax_method=meth, solver_prec=1e-10)
rhs(mg, None, uvw((nx, ny, nz)))
if touch == 2:
    import tempfile
    nhydro.set_option("tictoc", 1)
    nhydro.set_option("krylov", 4)
    n, hist = mg.solve_p(1e-10, 50)
    path = os.path.join(tempfile.mkdtemp(), "tictoc.txt")
    nhydro.print_tictoc(path)
    print(json.dumps(dict(n=n, tictoc=open(path).read())))
    mg.nhydro_clean()
    sys.exit(0)
if touch:
    nhydro.set_option("krylov", 4)
    mg.solve_p(1e-10, 50)
    nhydro.set_option("krylov", 0)
n, hist = mg.solve_p(1e-10, 50)
print(json.dumps(dict(n=n, hist=[float(h).hex() for h in hist], p=hashlib.sha256(np.ascontiguousarray(mg.grid(1).p).tobytes()).hexdigest())))
mg.nhydro_clean()
