"""numpy yardsticks of option "hold_odd_nz" (tests/test_gpu_hold_odd_nz.py, tests/_gpu_hold_grid_worker.py).

The transfers of a held pair (two levels of equal nz) are the reference's 2-D operators applied to every row: fine2coarse_2D with a 2-D x,
coarse2fine_2D_linear and coarse2fine_2D_nearest of mg_intergrids.f90, written here term by term in the reference's order (numpy neither
reorders nor fuses), so the GPU kernels are compared bit for bit.  Arrays are the library's host layout: index [i][j][k], halo included.

The reference has no hierarchy with a held pair, so a held LEVEL is pinned on an Oracle of that level's size: its level 1 is built from the
library's own dx, dy, zeta, h of the level (level_oracle), and its matrix, relax and residual are the reference's for such a grid."""
import numpy as np


def mirror(a):
    """the closed halo of a solver field: homogeneous Neumann images, corners included (mg_mpi_exchange.f90:509-597)"""
    a[:, 0] = a[:, 1]; a[:, -1] = a[:, -2]
    a[0] = a[1]; a[-1] = a[-2]
    return a


def restrict_held(x):
    """y(k,j2,i2) = x(k,j,i) + x(k,j,i+1) + x(k,j+1,i) + x(k,j+1,i+1), left to right; interior of the result, halo zero"""
    nx, ny = x.shape[0] - 2, x.shape[1] - 2
    y = np.zeros((nx // 2 + 2, ny // 2 + 2, x.shape[2]))
    y[1:-1, 1:-1] = ((x[1:nx + 1:2, 1:ny + 1:2] + x[2:nx + 2:2, 1:ny + 1:2]) + x[1:nx + 1:2, 2:ny + 2:2]) + x[2:nx + 2:2, 2:ny + 2:2]
    return y


def prolong_held(xc, linear=True):
    """the interior of the fine correction from the coarse array WITH its halo; halo of the result zero"""
    nxc, nyc = xc.shape[0] - 2, xc.shape[1] - 2
    nx, ny = 2 * nxc, 2 * nyc
    xf = np.zeros((nx + 2, ny + 2, xc.shape[2]))

    def at(dj, di):   # xc(k, j2 + dj, i2 + di)
        return xc[1 + di:1 + di + nxc, 1 + dj:1 + dj + nyc]
    if linear:
        a, b, c = 9.0 / 16.0, 3.0 / 16.0, 1.0 / 16.0
        xf[1:nx + 1:2, 1:ny + 1:2] = ((a * at(0, 0) + c * at(-1, -1)) + b * at(-1, 0)) + b * at(0, -1)   # (j  , i  )
        xf[1:nx + 1:2, 2:ny + 2:2] = ((a * at(0, 0) + c * at(+1, -1)) + b * at(+1, 0)) + b * at(0, -1)   # (j+1, i  )
        xf[2:nx + 2:2, 1:ny + 1:2] = ((a * at(0, 0) + c * at(-1, +1)) + b * at(-1, 0)) + b * at(0, +1)   # (j  , i+1)
        xf[2:nx + 2:2, 2:ny + 2:2] = ((a * at(0, 0) + c * at(+1, +1)) + b * at(+1, 0)) + b * at(0, +1)   # (j+1, i+1)
    else:
        for oi in (1, 2):
            for oj in (1, 2):
                xf[oi:nx + oi:2, oj:ny + oj:2] = at(0, 0)
    return xf


def held_levels(mg):
    """the fine levels of the held pairs of the live hierarchy, finest first"""
    nz = [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)]
    return [lev for lev in range(1, len(nz)) if nz[lev - 1] == nz[lev]]


def level_oracle(mg, lev, hc, theta_b=0.0, theta_s=0.0, **par):
    """an Oracle of level lev's size whose level 1 carries the library's dx, dy, zeta, h of that level (bmask: its mask too)"""
    from oracle.mgoracle import Oracle
    g = mg.grid(lev)
    o = Oracle(g.nx, g.ny, g.nz, 1, 1, **par)
    for name in ("dx", "dy", "zeta", "h"):
        o.field(name)[...] = g.get(name)
    if par.get("bmask"):
        o.field("rmask")[...] = g.get("rmask")
    o.matrices(hc, theta_b, theta_s)
    return o


def composite_vcycle(os_, lev1, ns_pre, ns_post, ns_coarsest, linear=True):
    """Vcycle(lev1) of mg_solvers.f90:129-151 on closed held levels lev1 .. lev1 + len(os_) - 1: relax and residual by each level's own
    Oracle (level 1 of os_[q]), the transfers by the numpy operators above.  Starts from the p and b the first Oracle holds."""
    n = len(os_)
    for q in range(n - 1):
        os_[q].relax(1, ns_pre)
        os_[q].residual(1)
        os_[q + 1].field("b")[...] = mirror(restrict_held(os_[q].field("r")))
        os_[q + 1].field("p")[...] = 0.0
    os_[n - 1].relax(1, ns_coarsest)
    for q in range(n - 2, -1, -1):
        r = mirror(prolong_held(os_[q + 1].field("p"), linear))
        p = os_[q].field("p")
        p[...] = p + r
        os_[q].relax(1, ns_post)
