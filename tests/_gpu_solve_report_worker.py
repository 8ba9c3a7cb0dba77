"""What a verbose solve_p leaves behind, for tests/test_gpu_solve_report.py: the seamount at 16 x 16 x 8, four colours, one rank, tol = 1e-30 and
maxite = 3, solved twice by each driver (MODE: plain, mixed = "cycle_precision" 32, krylov = "krylov" 2), each driver in a fresh working
directory.  The drivers print through C's printf, so every solve's lines are framed by marker lines, C's buffers flushed around them.
usage: _gpu_solve_report_worker.py   (one JSON line per solve between `@@ begin MODE K` and `@@ end MODE K`)"""
import ctypes
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

torch.cuda.set_device(0)
import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from _problem import gpu_problem, rhs, uvw  # noqa: E402

libc = ctypes.CDLL(None)


def mark(text):
    libc.fflush(None)
    print(text, flush=True)


nx, ny, nz = 16, 16, 8
nhydro.set_verbose(1)
gpu_problem(mg, (nx, ny, nz), relax_method="FC", solver_prec=1e-10)
rhs(mg, None, uvw((nx, ny, nz)))
for mode, opts in (("plain", {}), ("mixed", {"cycle_precision": 32}), ("krylov", {"krylov": 2})):
    for k, val in opts.items():
        nhydro.set_option(k, val)
    os.chdir(tempfile.mkdtemp())
    for k in (1, 2):
        mark(f"@@ begin {mode} {k}")
        before = nhydro.counters()["launches"]
        n, hist = mg.solve_p(1e-30, 3)
        launches = nhydro.counters()["launches"] - before
        mark("@@ json " + json.dumps(dict(n=n, hist=[float(h).hex() for h in hist], launches=launches, fort100=open("fort.100").read())))
        mark(f"@@ end {mode} {k}")
    for k in opts:
        nhydro.set_option(k, {"cycle_precision": 64, "krylov": 0}[k])
mg.nhydro_clean()
