"""Worker of tests/test_gpu_resrest_zw.py: the switches of the fused residual + restriction are read from the environment once per
process, so every path runs in a process of its own.  Arguments: the case, the file the arrays go to (np.savez).  Written per stage:
every level's b and p after two V-cycles, then the history of two solve_p iterations and level 1's p after them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from mgroms_amd.testcases import island_mask, seamount_geometry  # noqa: E402

CASES = {  # dims, option "periodic", what else
    "nz2": ((8, 8, 2), 0, ""), "nz4": ((8, 8, 4), 0, ""), "ragged": ((24, 72, 12), 0, ""), "empty_wave": ((12, 8, 6), 0, ""),
    "periodic": ((32, 16, 8), 3, ""), "moving": ((16, 16, 8), 0, "moving"), "bmask": ((16, 16, 8), 0, "bmask"),
    "user_matrix": ((16, 16, 8), 0, "user_matrix"),
}
case, dest = sys.argv[1], sys.argv[2]
(nx, ny, nz), per, what = CASES[case]
torch.cuda.set_device(0)
nhydro.set_verbose(0)
nhydro.set_option("periodic", per)
mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method="FC", bmask=1 if what == "bmask" else 0))
rng = np.random.default_rng(11)
dx, dy, zeta, h = seamount_geometry(nx, ny, 1, 1, 0)


def halo(a):  # (nx, ny) interior -> (nx+2, ny+2): the wrapped interior along a periodic direction, the edge value on a closed side
    for ax, bit in ((0, 1), (1, 2)):
        w = [(0, 0), (0, 0)]; w[ax] = (1, 1)
        a = np.pad(a, w, mode="wrap" if per & bit else "edge")
    return a


# nothing constant along a direction, no symmetry: every column its own depth and surface
h = halo(h[1:-1, 1:-1] * (1.0 + 0.02 * (2.0 * rng.random((nx, ny)) - 1.0)))
surfaces = [halo(0.3 * rng.standard_normal((nx, ny))) for _ in range(2)]
sigma = (250.0, 0.4, 6.0)  # a stretched coordinate: on a uniform one zw is linear in k and a depth taken from the wrong row goes unseen
rmask = island_mask(nx, ny) if what == "bmask" else None
out = {}


def stage(tag, zeta):
    mg.nhydro_matrices(dx, dy, zeta, h, rmask, *sigma)
    g = mg.grid(1)
    if what == "user_matrix":  # slots 4 and 7 that no depth formula gives
        cA = g.get("cA"); cA[..., 3] *= 1.5; cA[..., 6] *= 1.25
        g.set("cA", cA)
    r = np.random.default_rng(12)
    g.set("p", r.standard_normal(g._shape("p"))); g.set("b", r.standard_normal(g._shape("b"))); mg.fill_halo(1, "p")
    for _ in range(2):
        mg.Vcycle(1)
    for lev in range(1, mg.nlevs() + 1):
        out[f"{tag}_b{lev}"] = mg.grid(lev).b; out[f"{tag}_p{lev}"] = mg.grid(lev).p
    n, hist = mg.solve_p(1e-30, 2)
    out[f"{tag}_hist"] = np.asarray(hist); out[f"{tag}_p_solved"] = mg.grid(1).p


stage("first", surfaces[0])
if what == "moving":  # the free surface moved: the generated depths must follow the refreshed 2-D fields
    stage("second", surfaces[1])
np.savez(dest, **out)
mg.nhydro_clean()
print("DONE", len(out))
