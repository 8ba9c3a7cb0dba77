"""Every consumer of dx, dy on a metric that varies in i and in j, against the CPU oracle.

The generators' dx, dy are constant over the plane, and the two metrics the other files vary are separable (dx(i), dy(j)).  On such a
metric a 2-D factor fetched one column off, a face average with the wrong partner, a swapped pair in the coarsening of dx, dy or the
cell's metric where the face's is meant leave every bit unchanged.  Here dx, dy are the generators' times
testcases.curvilinear_metric -- dx(i,j), dy(i,j) within 25 % of the uniform value, not symmetric, not separable, fx no shifted copy of
fy -- as a curvilinear ROMS / CROCO grid has them, and each operation that reads dx or dy is compared with the oracle on it: the
set-up of every level, the four-colour pass matrix-free and on stored slots (one shape per kernel family of mgx_choice.h), red-black,
the residual, the fused residual + restriction and the closing residual of solve_p, compute_rhs, correct_uvw, Krylov pass 1, the
device-resident refresh and the held levels.  (The fp32 operators: tests/test_gpu_mixed_precision.py; the dx, dy halos between ranks:
the `curv` rows of tests/test_gpu_multirank.py; the wrap: tests/test_gpu_periodic.py.)

The oracle itself is tied on this metric without the GPU: its matrix, divergence and gradient keep the operator identity on the
curvilinear cases of tests/_operator_identity.py to 3.4e-16 ... 1.4e-15, and four colours are decomposition independent bit for bit
(tests/test_oracle.py).

Tolerances are those the project already states for the same operation on the seamount (tests/test_gpu_parity.py): four colours, the
residual, the set-up and the model coupling bit for bit; norms 1e-13 relative; histories against the oracle 1e-12; the red-black
default 1e-12 of max|p| per relax call; the stretched coordinate 1e-12 (device cosh / exp)."""
import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, hist_close, load_uvw, on_gpu, oracle_twin, problem, random_level, rhs, uvw

pytestmark = pytest.mark.gpu
HC = 4e3
mg = gpu_module(rb_exact=0, rb_seq=1, krylov=0, hold_odd_nz=0)

_restore_options = restore_options("rb_exact", "rb_seq", "krylov")


def _mf(monkeypatch, stored):
    """MGX_NO_MF is read by every nhydro_init: the stored slots instead of the in-kernel coefficients"""
    if stored:
        monkeypatch.setenv("MGX_NO_MF", "1")
    else:
        monkeypatch.delenv("MGX_NO_MF", raising=False)


def _setup(mg, dims, geom="seamount", **par):
    """the curvilinear problem on the GPU and its oracle twin"""
    pr = gpu_problem(mg, dims, geom=geom, metric="curvilinear", **dict(dict(relax_method="FC", solver_prec=1e-10), **par))
    assert pr.metric == "curvilinear"
    dx, dy = pr.fields[:2]
    for a in (dx, dy):      # what was handed over varies along every row and every column
        assert np.ptp(a, axis=0).min() > 0 and np.ptp(a, axis=1).min() > 0
    return pr, oracle_twin(pr)


def _same(a, c, what):
    assert a.shape == c.shape and np.array_equal(a, c), (what, float(np.abs(a - c).max()), np.argwhere(a != c)[:4].tolist())


# ---- set-up ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,geom,bmask", [((32, 16, 8), "seamount", False), ((64, 32, 16), "seamount", False),
                                             ((48, 96, 16), "rndtopo", False), ((32, 64, 16), "seamount", True)],
                         ids=["32x16x8", "64x32x16", "48x96x16-rndtopo", "32x64x16-bmask"])
def test_setup_every_level_bitwise(mg, dims, geom, bmask, monkeypatch):
    """dx, dy, h, zr, zw, cw, cA (bmask: rmask too) of every level, halo included: the coarsening of the metric (nx /= ny: a transposed
    pair would show) and every coefficient built from it"""
    _mf(monkeypatch, False)
    pr, o = _setup(mg, dims, geom, bmask=bmask)
    assert mg.nlevs() == o.nlevs
    for lev in range(1, o.nlevs + 1):
        g, li = mg.grid(lev), o.level_info(lev)
        assert (g.nx, g.ny, g.nz) == (li["nx"], li["ny"], li["nz"])
        for name in ("dx", "dy", "h", "zr", "zw", "cw", "cA") + (("rmask",) if bmask else ()):
            _same(g.get(name), o.field(name, lev), (lev, name))
        if min(g.nx, g.ny) >= 4:   # the coarsened metric still varies in both directions
            assert np.ptp(g.get("dx")[1:-1, 1:-1], axis=0).min() > 0 and np.ptp(g.get("dx")[1:-1, 1:-1], axis=1).min() > 0
    o.close()


# ---- four colours ----------------------------------------------------------------------------------------------------------------
# one shape per kernel family that mgx_choice.h distinguishes
FC_SHAPES = [
    ((32, 16, 8), False),     # register-resident
    ((64, 32, 16), False),    # register-resident
    ((64, 32, 64), False),    # register-resident, nz = 64
    ((32, 32, 24), False),    # generic coarse levels of 12, 6, 3 rows
    ((32, 32, 96), False),    # tall, matrix-free
    ((16, 32, 128), False),   # tall, matrix-free
    ((32, 32, 96), True),     # bmask: tall on stored slots
]


@pytest.mark.parametrize("stored", [False, True], ids=["matrix-free", "stored"])
@pytest.mark.parametrize("dims,bmask", FC_SHAPES, ids=["%dx%dx%d%s" % (d + ("-bmask" if b else "",)) for d, b in FC_SHAPES])
def test_relax_fc_every_level_bitwise(mg, dims, bmask, stored, monkeypatch):
    """two four-colour sweeps from a random p, b on every level, the whole array with its halo: with the coefficients rebuilt in
    registers from the 2-D factors (MF_PROLOGUE, OWN_SLOPES) and with MGX_NO_MF = 1 on the stored slots -- each against the oracle, not
    only against the other"""
    _mf(monkeypatch, stored)
    pr, o = _setup(mg, dims, bmask=bmask)
    rng = np.random.default_rng(2)
    t0 = mg.nhydro.get_option("tall_stored_passes")
    for lev in range(1, o.nlevs + 1):
        g = random_level(mg, o, lev, rng)
        mg.relax(lev, 2); o.relax(lev, 2)
        _same(g.get("p"), o.field("p", lev), (lev, "p"))
    tall = mg.nhydro.get_option("tall_stored_passes") - t0
    if dims[2] >= 96:   # the tall-column pass on stored coefficients ran exactly where the matrix-free form may not
        assert (tall > 0) == (stored or bmask), (tall, stored, bmask)
    o.close()


# ---- red-black -------------------------------------------------------------------------------------------------------------------
def _rho_from_oracle(o, lev):
    """the contraction bound of the windowed walk from the oracle's coefficients: g1 = (T^-1 e1)(1) by tridiag's recurrences
    (mg_relax.f90:308-334), times cA(5|8, 1, j, i) -- as tests/test_gpu_parity.py::test_rb_sequential_order_windowed_walk forms it"""
    cA = o.field("cA", lev)[1:-1, 1:-1]
    d, dd = cA[..., 0], cA[..., 1]
    n = d.shape[-1]
    bet = 1.0 / d[..., 0]; x = np.zeros_like(d); gam = np.zeros_like(d); x[..., 0] = bet
    for k in range(1, n):
        gam[..., k] = dd[..., k] * bet
        bet = 1.0 / (d[..., k] - dd[..., k] * gam[..., k])
        x[..., k] = (0 - dd[..., k] * x[..., k - 1]) * bet
    for k in range(n - 2, -1, -1):
        x[..., k] -= gam[..., k + 1] * x[..., k + 1]
    return (np.abs(x[..., 0] * cA[..., 0, 4]) + np.abs(x[..., 0] * cA[..., 0, 7])).max()


@pytest.mark.parametrize("dims", [(32, 64, 16), (16, 32, 128)], ids=lambda d: "%dx%dx%d" % d)
def test_relax_rb_default_every_level(mg, dims, monkeypatch):
    """the red-black default (the reference's sequential order at speed, rb_seq) on every level, two relax calls from a random state:
    each within 1e-12 of max|p| of the oracle's sequential loop, the project's bound for this mode.  The windowed walk ran (two colours
    per call, but for the one-workgroup levels), and its rho is the bound rebuilt from THIS matrix."""
    _mf(monkeypatch, False)
    pr, o = _setup(mg, dims, relax_method="RB")
    assert mg.nhydro.get_option("rb_seq") == 1 and mg.nhydro.get_option("rb_exact") == 0 and mg.nhydro.get_option("rbseq_window") == 1
    rng = np.random.default_rng(41)
    for lev in range(1, o.nlevs + 1):
        rho, m = mg.nhydro.rbseq_window_info(lev)
        rho_o = _rho_from_oracle(o, lev)
        assert abs(rho - rho_o) <= 1e-12 * rho_o, (lev, rho, rho_o)
        g = random_level(mg, o, lev, rng)
        for call in range(2):
            n0 = mg.nhydro.get_option("rbseq_window_colours")
            mg.relax(lev, 1); o.relax(lev, 1)
            windows = mg.nhydro.get_option("rbseq_window_colours") - n0
            a, c = g.get("p"), o.field("p", lev)
            err = np.abs(a - c).max() / np.abs(c).max()
            print(f"{dims} level {lev} call {call}: {windows} window colours, {err:.3e} of max|p| from the sequential loop")
            assert err <= 1e-12, (lev, call, err)
            assert windows == 2 or (lev >= 2 and windows == 0 and g.nx * g.ny * g.nz <= 8192), (lev, windows, g.nx, g.ny, g.nz)
            assert lev > 1 or windows == 2
    o.close()


def test_relax_rb_exact_every_level_bitwise(mg, monkeypatch):
    """rb_exact: the reference's sequential order, one relax call of two sweeps per level, bit for bit"""
    _mf(monkeypatch, False)
    mg.nhydro.set_option("rb_exact", 1)
    pr, o = _setup(mg, (32, 32, 8), relax_method="RB")
    rng = np.random.default_rng(5)
    for lev in range(1, o.nlevs + 1):
        g = random_level(mg, o, lev, rng)
        mg.relax(lev, 2); o.relax(lev, 2)
        _same(g.get("p"), o.field("p", lev), (lev, "p"))
    o.close()


# ---- residual, norm, transfers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored", [False, True], ids=["matrix-free", "stored"])
def test_residual_and_norm(mg, stored, monkeypatch):
    """r bit for bit and its norm within 1e-13 on levels 1 and 2, from a random p, b; at 64 x 32 x 16 (level 1 matrix-free unless
    MGX_NO_MF) and at 32 x 16 x 8"""
    _mf(monkeypatch, stored)
    for dims in ((64, 32, 16), (32, 16, 8)):
        pr, o = _setup(mg, dims)
        rng = np.random.default_rng(1)
        for lev in (1, 2):
            g = random_level(mg, o, lev, rng)
            _same(g.get("p"), o.field("p", lev), (lev, "p with its halo"))
            res, reso = mg.compute_residual(lev), o.residual(lev)
            _same(g.get("r"), o.field("r", lev), (lev, "r"))
            assert abs(res - reso) <= 1e-13 * reso, (lev, res, reso)
        o.close()


@pytest.mark.parametrize("stored", [False, True], ids=["matrix-free", "stored"])
def test_solve_three_iterations_bitwise(mg, stored, monkeypatch):
    """three solve_p iterations with four colours at 64 x 32 x 64 from seeded random u, v, w: the fused residual + restriction of the
    down legs (matrix-free: slots 4 and 7 rebuilt in registers), the transfers of every level and the closing residual.  p of every
    level and r bit for bit, the history within 1e-12"""
    _mf(monkeypatch, stored)
    dims = (64, 32, 64)
    pr, o = _setup(mg, dims)
    rhs(mg, o, uvw(dims, seed=13))
    _same(mg.grid(1).b, o.field("b"), "b")
    n, hist = mg.solve_p(1e-30, 3)
    no, ho, _ = o.solve_p(1e-30, 3)
    assert n == no == 3 and hist_close(hist, ho, rtol=1e-12, atol=0.0, same_length=True), (hist, ho)
    assert hist[3] < hist[0]
    for lev in range(1, o.nlevs + 1):
        _same(mg.grid(lev).p, o.field("p", lev), (lev, "p"))
    res, reso = mg.compute_residual(1), o.residual(1)     # the level-1 residual kernel of nz = 64 on the solve's p
    _same(mg.grid(1).r, o.field("r"), "r")
    assert abs(res - reso) <= 1e-13 * reso, (res, reso)
    o.close()


# ---- the model coupling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,bmask", [((32, 16, 8), False), ((48, 32, 8), True)], ids=["32x16x8", "48x32x8-bmask"])
def test_compute_rhs_and_correct_uvw_bitwise(mg, dims, bmask, monkeypatch):
    """seeded random u, v, w: b after compute_rhs (the face's metric in the fluxes and the cross terms), then p, u, v, w after
    nhydro_solve (correct_uvw's gradient over the face's metric), bit for bit"""
    _mf(monkeypatch, False)
    pr, o = _setup(mg, dims, bmask=bmask, solver_prec=1e-9, solver_maxiter=3)
    u, v, w = uvw(dims, seed=5)
    load_uvw(o, (u, v, w))
    mg.nhydro.compute_rhs(u, v, w, pr.rmask)
    o.compute_rhs()
    _same(mg.grid(1).b, o.field("b"), "b")
    assert np.abs(mg.grid(1).b).max() > 0
    mg.nhydro_solve(u, v, w, pr.rmask)
    o.nhydro_solve()
    _same(mg.grid(1).p, o.field("p"), "p")
    for name, a in (("u", u), ("v", v), ("w", w)):
        _same(a, o.field(name), name)
    o.close()


def test_stretched_sigma_with_a_free_surface(mg, monkeypatch):
    """theta_s = 6, theta_b = 0.4, hc = 250 and zeta /= 0 on the curvilinear metric at 32 x 32 x 16: zr, zw, cA of every level within
    1e-12, the bound of tests/test_gpu_parity.py::test_stretched_sigma_coordinates (the device's cosh / exp differ from the host's in
    the last bit); the histories of a solve within that test's bound"""
    _mf(monkeypatch, False)
    dims = nx, ny, nz = 32, 32, 16
    ii, jj = np.meshgrid(np.arange(nx + 2), np.arange(ny + 2), indexing="ij")
    zeta = 0.4 * np.cos(0.25 * ii) * np.sin(0.15 * jj)
    pr, o = _setup(mg, dims, zeta=zeta, sigma=(250.0, 0.4, 6.0), solver_prec=1e-9)
    for lev in range(1, o.nlevs + 1):
        for name in ("dx", "dy"):
            _same(mg.grid(lev).get(name), o.field(name, lev), (lev, name))
        for name in ("zr", "zw", "cA"):
            a, b = mg.grid(lev).get(name), o.field(name, lev)
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max()), (lev, name)
    rhs(mg, o, uvw(dims))
    n, hist = mg.solve_p(1e-9, 50)
    no, ho, _ = o.solve_p(1e-9, 50)
    assert n == no and np.all(np.abs(hist - ho) <= 1e-13 + 1e-10 * np.abs(ho)), (hist, ho)
    o.close()


# ---- Krylov --------------------------------------------------------------------------------------------------------------------
def test_krylov_follows_the_reference_gcr(mg, monkeypatch):
    """krylov = 4 at 64 x 32 x 16 with four colours to 1e-10 (pass 1 applies the level-1 operator matrix-free): the same count as the
    numpy GCR over the oracle and the history within 10 x eps_ref, the bounds of tests/test_gpu_krylov.py"""
    from tests._krylov_ref import eps_ref, history_noise
    _mf(monkeypatch, False)
    dims = (64, 32, 16)
    pr = problem(dims, metric="curvilinear", relax_method="FC", solver_prec=1e-10, solver_maxiter=50)

    def oracle():
        o = oracle_twin(pr)
        rhs(None, o, uvw(dims))
        return o
    e, nref, href = eps_ref(oracle, 4, 1e-10)
    on_gpu(mg, pr)
    rhs(mg, None, uvw(dims))
    mg.nhydro.set_option("krylov", 4)
    n, hist = mg.solve_p(1e-10, 50)
    d = history_noise(hist, href, 1e-10)
    print(f"\n64x32x16 FC m=4 curvilinear: GPU {n} it, reference {nref} it, eps_ref {e:.3e}, history difference {d:.3e} = {d / e:.2f} x eps_ref")
    assert n == nref, (n, nref)
    assert d <= 10 * e, (d, e)
    assert mg.nhydro.get_option("krylov_restarts") == 0


# ---- the device-resident step ------------------------------------------------------------------------------------------------
def _zeta(nx, ny, ph, seed):
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    return 0.8 * np.sin(2 * np.pi * i / nx + ph) * np.cos(2 * np.pi * j / ny - ph) + 0.05 * np.random.default_rng(seed).standard_normal((nx + 2, ny + 2))


@pytest.mark.parametrize("dims", [(32, 16, 8), (64, 32, 64)], ids=lambda d: "%dx%dx%d" % d)
def test_device_matrices_and_zeta_refresh_bitwise(mg, dims, monkeypatch):
    """nhydro_matrices_device from tensors, and nhydro_update_zeta_device to another free surface, leave on every level exactly what
    nhydro_matrices from numpy leaves with that free surface -- which is the oracle's (theta = 0: no transcendental function)"""
    import torch
    _mf(monkeypatch, False)
    nx, ny, _ = dims
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    za, zc = _zeta(nx, ny, 0.0, 31), _zeta(nx, ny, 2.9, 33)
    names = ("dx", "dy", "zeta", "h", "zr", "zw", "cw", "cA")
    pr = gpu_problem(mg, dims, metric="curvilinear", zeta=zc, sigma=(HC, 0.0, 0.0), relax_method="FC", solver_prec=1e-12)
    o = oracle_twin(pr)
    host = {(lev, n): mg.grid(lev).get(n) for lev in range(1, mg.nlevs() + 1) for n in names}
    for (lev, n), a in host.items():
        if n != "zeta":
            _same(a, o.field(n, lev), ("nhydro_matrices", lev, n))
    dx, dy, _, h = pr.fields
    par = mg.nhydro.default_params(**pr.par)
    for what, first in (("matrices_device", zc), ("update_zeta_device", za)):
        mg.nhydro_clean()
        mg.nhydro_init(*dims, 1, 1, 0, par)
        mg.nhydro_matrices_device(dev(dx), dev(dy), dev(first), dev(h), None, HC, 0.0, 0.0)
        if first is za:
            assert not np.array_equal(mg.grid(1).get("cA"), host[(1, "cA")])
            mg.nhydro_update_zeta_device(dev(zc))
            assert mg.nhydro.get_option("zeta_refreshes") == 1
        for (lev, n), a in host.items():
            _same(mg.grid(lev).get(n), a, (what, lev, n))
    o.close()


# ---- held levels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nzs", [((32, 32, 40), [40, 20, 10, 5]), ((64, 64, 40), [40, 20, 10, 5, 5])], ids=["32x32x40", "64x64x40"])
def test_hold_odd_nz_relax_every_level_bitwise(mg, dims, nzs, monkeypatch):
    """hold_odd_nz = 1 with nz = 40: one four-colour relax call on every level, bit for bit.  At 32 x 32 x 40 the hierarchy ends at
    4 x 4 x 5, the level on which nz turns odd, so the option changes nothing there; 64 x 64 x 40 has one level more, the held pair
    (8 x 8 x 5, 4 x 4 x 5), whose colour passes are the generic ones.  The reference has no such hierarchy, so each level is held to an
    Oracle of its size fed with the level's own dx, dy, zeta, h (tests/_hold_ref.py), as tests/test_gpu_hold_odd_nz.py does; down to
    the first level of odd nz the hierarchy is the default one, and there dx, dy are the oracle twin's coarsening too."""
    from _hold_ref import held_levels, level_oracle
    _mf(monkeypatch, False)
    pr = gpu_problem(mg, dims, metric="curvilinear", sigma=(HC, 0.0, 0.0), init_options=dict(hold_odd_nz=1), relax_method="FC", solver_prec=1e-10)
    try:
        held = held_levels(mg)
        assert [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)] == nzs and held == ([4] if len(nzs) == 5 else [])
        twin = oracle_twin(pr)
        for lev in range(1, 5):
            for name in ("dx", "dy"):
                _same(mg.grid(lev).get(name), twin.field(name, lev), (lev, name))
        twin.close()
        rng = np.random.default_rng(9)
        for lev in range(1, mg.nlevs() + 1):
            o = level_oracle(mg, lev, HC, relax_method="FC")
            g = mg.grid(lev)
            _same(g.get("cA")[1:-1, 1:-1], o.field("cA")[1:-1, 1:-1], (lev, "cA"))
            p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
            g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
            o.field("p")[...] = p; o.field("b")[...] = b; o.fill_halo(1, "p")
            mg.relax(lev, 1); o.relax(1, 1)
            _same(g.get("p"), o.field("p"), (lev, "p"))
            o.close()
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("hold_odd_nz", 0)
