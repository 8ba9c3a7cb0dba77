"""Vertical sizes that are not powers of two (nz = 24, 40, 48, 80, 96 and their coarse levels 20, 12, 10, 6, 5, 3), which
ROMS / CROCO users choose for their physics: the reference halves any even nz (mg_grids.f90:503-541), and so does this
library.  Every path a solve takes at these sizes -- the level-1 colour pass, the default red-black order, Gauss-Seidel, the
transfers, the odd coarsest levels, a gathered multi-rank run and the Fortran driver -- against the CPU oracle.

Tolerances as in test_gpu_parity.py: four-colour and Gauss-Seidel fields bit for bit, histories 1e-12 relative (norms are
reduced in another order), the default red-black order 1e-12 of max|p| per relax call (rb_exact: bit for bit)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import gpu_problem, hist_close, oracle_twin, random_level, rhs, uvw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
mg = gpu_module(rb_exact=0)


def _setup(mg, nx, ny, nz, bmask=False, **par):
    """the seamount problem on the GPU and on the oracle (bmask: the island mask on both)"""
    return oracle_twin(gpu_problem(mg, (nx, ny, nz), bmask=bmask, **dict(dict(relax_method="FC", solver_prec=1e-10), **par)))


# ---- four colours ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 24), (64, 32, 48), (32, 32, 40), (64, 64, 96), (32, 32, 6)])
def test_fc_solve_bitwise(mg, dims):
    """three V-cycles of solve_p: p and b of every level bit for bit, the residual of every level (recomputed on both sides)
    bit for bit, the history to 1e-12; then nhydro_solve's u, v, w bit for bit"""
    nx, ny, nz = dims
    o = _setup(mg, nx, ny, nz)
    assert mg.nlevs() == o.nlevs
    rhs(mg, o, uvw(dims))
    n, hist = mg.solve_p(1e-30, 3)
    no, ho, _ = o.solve_p(1e-30, 3)
    assert n == no == 3 and hist_close(hist, ho, rtol=1e-12, atol=1e-13, same_length=True), (hist, ho)
    for lev in range(1, o.nlevs + 1):
        g = mg.grid(lev)
        for name in ("p", "b"):
            a, c = g.get(name), o.field(name, lev)
            assert np.array_equal(a, c), (lev, name, np.abs(a - c).max())
        mg.compute_residual(lev); o.residual(lev)
        a, c = g.get("r")[1:-1, 1:-1], o.field("r", lev)[1:-1, 1:-1]
        assert np.array_equal(a, c), (lev, "r", np.abs(a - c).max())
    # the whole nhydro_solve from a rough state
    o = _setup(mg, nx, ny, nz, solver_maxiter=8)
    u, v, w = uvw(dims, seed=17)
    o.field("u")[...] = u; o.field("v")[...] = v; o.field("w")[...] = w
    mg.nhydro_solve(u, v, w)
    o.nhydro_solve()
    assert np.array_equal(mg.grid(1).p, o.field("p"))
    assert np.array_equal(u, o.field("u")) and np.array_equal(v, o.field("v")) and np.array_equal(w, o.field("w"))


@pytest.mark.parametrize("nz", [48, 96])
def test_fc_relax_bench_scale(mg, nz):
    """one level-1 four-colour relax at the bench's plane size (512 x 512), bit for bit"""
    o = _setup(mg, 512, 512, nz)
    g = random_level(mg, o, 1, np.random.default_rng(nz))
    mg.relax(1, 1); o.relax(1, 1)
    assert np.array_equal(g.get("p"), o.field("p"))


# ---- the reference default: red-black, cmatrix='real', sequential order -------------------------------------------
@pytest.mark.parametrize("dims,bmask", [((64, 64, 48), False), ((32, 32, 24), False), ((32, 32, 48), True), ((32, 32, 128), True)])
def test_rb_default_relax_every_level(mg, dims, bmask):
    """relax(lev, 1) of the default red-black order on every level from a random state, within 1e-12 of the oracle's sequential
    loop.  With bmask the colour pass runs on stored coefficients, i.e. not the matrix-free kernel: at nz = 48 and nz = 128 the
    windowed walk must then restore the physical images of the rows below its row cut."""
    nx, ny, nz = dims
    o = _setup(mg, nx, ny, nz, bmask=bmask, relax_method="RB")
    assert mg.nhydro.get_option("rb_seq") == 1 and mg.nhydro.get_option("rb_exact") == 0
    rng = np.random.default_rng(41)
    for lev in range(1, o.nlevs + 1):
        g = random_level(mg, o, lev, rng)
        mg.relax(lev, 1); o.relax(lev, 1)
        a, c = g.get("p"), o.field("p", lev)
        assert np.abs(a - c).max() <= 1e-12 * np.abs(c).max(), (lev, np.abs(a - c).max() / np.abs(c).max())


def test_rb_exact_tall_bmask(mg):
    """the reference's order bit for bit (rb_exact) at nz = 128 with bmask, every level"""
    mg.nhydro.set_option("rb_exact", 1)
    try:
        o = _setup(mg, 32, 32, 128, bmask=True, relax_method="RB")
        rng = np.random.default_rng(43)
        for lev in range(1, o.nlevs + 1):
            g = random_level(mg, o, lev, rng)
            mg.relax(lev, 1); o.relax(lev, 1)
            assert np.array_equal(g.get("p"), o.field("p", lev)), lev
    finally:
        mg.nhydro.set_option("rb_exact", 0)


# ---- Gauss-Seidel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 24), (16, 16, 48), (16, 16, 128)])
def test_gauss_seidel_any_nz(mg, dims):
    """relax_method='GS' at sizes without a register-resident instance: relax on every level, then a three-iteration solve_p,
    bit for bit"""
    nx, ny, nz = dims
    o = _setup(mg, nx, ny, nz, relax_method="GS")
    rng = np.random.default_rng(7)
    for lev in range(1, o.nlevs + 1):
        g = random_level(mg, o, lev, rng)
        mg.relax(lev, 2); o.relax(lev, 2)
        assert np.array_equal(g.get("p"), o.field("p", lev)), lev
    o = _setup(mg, nx, ny, nz, relax_method="GS")
    rhs(mg, o, uvw(dims))
    n, hist = mg.solve_p(1e-30, 3)
    no, ho, _ = o.solve_p(1e-30, 3)
    assert n == no == 3 and hist_close(hist, ho, rtol=1e-12, atol=1e-13, same_length=True), (hist, ho)
    assert np.array_equal(mg.grid(1).p, o.field("p"))


# ---- kernel selection ----------------------------------------------------------------------------------------------------
def _relax_launches(mg, nx, ny, nz, method):
    gpu_problem(mg, (nx, ny, nz), relax_method=method)
    mg.relax(1, 2)
    c0 = mg.nhydro.counters()
    mg.relax(1, 2)
    c1 = mg.nhydro.counters()
    return c1["launches"] - c0["launches"], c1["halo_fills"] - c0["halo_fills"]


@pytest.mark.parametrize("method,nz,nz2", [("FC", 48, 64), ("RB", 48, 64), ("FC", 96, 128)])
def test_level1_takes_the_register_kernel(mg, method, nz, nz2):
    """the level-1 colour pass at nz = 48 / 96 stores its own physical mirrors (and for red-black the walk's d0), as the nz = 64
    / 128 kernels do: relax(1, 2) issues the same launches.  (Red-black is not compared at 96 against 128: the nz = 128 pass
    leaves no d0, so its count legitimately differs.)"""
    assert _relax_launches(mg, 512, 512, nz, method) == _relax_launches(mg, 512, 512, nz2, method)


# ---- multi-rank, Fortran -------------------------------------------------------------------------------------------------
def test_thread_ranks_2x2_gather_nz24():
    """2x2 ranks of 32 x 32 x 24 (64 x 64 x 24 in all), coarse levels gathered: every rank's fields bit for bit against the
    oracle's emulated ranks (tests/_gpu_thread_ranks.py)"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_thread_ranks.py"), "2", "2", "32", "32", "24", "8"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-3000:]
    for r in range(4):
        assert f"rank {r} ok" in out.stdout


def test_fortran_driver_default_namelist_nz48(mg, tmp_path):
    """fortran/testseamount_gpu 64 64 48 with the default namelist (red-black, the reference default): every printed residual
    agrees with the oracle's history to the printed digits (E10.3), sum(p**2) to 1e-10"""
    exe = os.path.join(os.path.dirname(HERE), "fortran", "testseamount_gpu")
    if not os.path.exists(exe):
        pytest.skip("flang not available when build() ran")
    mg.nhydro_clean()
    (tmp_path / "nh_namelist").write_text("&nhparam\n/\n")
    out = subprocess.run([exe, "64", "64", "48"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    its = re.findall(r"ite = *(\d+): res = *([0-9.E+-]+) / conv", out.stdout)
    from oracle.mgoracle import make_seamount
    o = make_seamount(64, 64, 48)
    n, h, _ = o.nhydro_solve()
    assert len(its) == n > 0
    for (k, r) in its:
        assert abs(float(r) - h[int(k)]) <= 5.1e-3 * h[int(k)]
    sp2 = float(re.search(r"sum_p2 = *([0-9.E+-]+)", out.stdout).group(1))
    assert np.isclose(sp2, (o.field("p")[1:-1, 1:-1, :] ** 2).sum(), rtol=1e-10)
