#!/usr/bin/env python3
"""Time level-1 smoother sweeps and residuals only (HIP events): python3 scripts/sweep_time.py [nx ny nz method reps [mask]]
mask: bmask = .true. with the island mask of mgroms_amd.testcases -- the colour pass then runs on stored coefficients"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import island_mask, resting_column_state, seamount_geometry  # noqa: E402

nx, ny, nz = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (512, 512, 64)
method = sys.argv[4] if len(sys.argv) > 4 else "FC"
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 30
mask = len(sys.argv) > 6 and sys.argv[6] == "mask"
torch.cuda.set_device(0)
nhydro.set_verbose(0)
mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method=method, bmask=1) if mask else nhydro.default_params(relax_method=method))
mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), island_mask(nx, ny) if mask else None, 4e3, 0.0, 0.0)
nhydro.compute_rhs(*resting_column_state(nx, ny, nz))
mg.Vcycle(1)
nhydro.time_relax(1, 5)
s = [nhydro.time_relax(1, reps) for _ in range(3)]
r = [nhydro.time_residual(1, reps) for _ in range(3)]
cells = nx * ny * nz
print(f"{method} {nx}x{ny}x{nz}{' bmask' if mask else ''}: sweep {min(s):.4f} ms ({88*cells/min(s)/1e6/8000*100:.1f}% of 8 TB/s), residual {min(r):.4f} ms ({88*cells/min(r)/1e6/8000*100:.1f}%)")
mg.nhydro_clean()
