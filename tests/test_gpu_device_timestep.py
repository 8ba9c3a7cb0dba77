"""The set-up half of a device-resident time step: nhydro_matrices_device, nhydro_update_zeta_device (the per-step call of a model with
a moving free surface) and nhydro_check_nondivergence_device, on torch tensors.

Contract: everything is bit for bit what nhydro_matrices from host arrays leaves, so every comparison is np.array_equal -- both sides
run the same kernels in the same order.  theta_s = theta_b = 0 throughout: setup_zr_zw then has no transcendental function and the CPU
oracle is bitwise too, with zeta /= 0 (tests/test_gpu_model_coupling.py::test_two_time_steps_with_a_moving_free_surface).

The reference of a shape -- every field of every level after nhydro_matrices(dx, dy, zeta_c, h) from numpy -- is built once per module
and shared (`_host_reference`)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import oracle_twin, problem, rhs, uvw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# (nx, ny, nz), bmask
SHAPES = [
    ((32, 32, 8), 0),
    ((96, 64, 24), 0),    # an odd coarsest nz (24, 12, 6, 3); three tiles of the one-launch zeta path in i, two in j
    ((62, 6, 24), 0),     # a one-level hierarchy: only level-1 halos to write, tile tails in both directions
    ((16, 32, 128), 0),   # a tall column
    ((32, 32, 8), 1),     # bmask = 1 with a random 0/1 rmask
]
IDS = ["%dx%dx%d%s" % (s + ("-bmask" if b else "",)) for s, b in SHAPES]
GEO = ("dx", "dy", "h")
FIELDS = ("dx", "dy", "zeta", "h", "zr", "zw", "cw", "cA")
HC = 4e3


mg = gpu_module()


def _zeta(nx, ny, which):
    """three states of a moving free surface: the sine + noise form of test_two_time_steps_with_a_moving_free_surface"""
    ph, seed = {"a": (0.0, 31), "b": (1.3, 32), "c": (2.9, 33)}[which]
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    rng = np.random.default_rng(seed)
    return 0.8 * np.sin(2 * np.pi * i / nx + ph) * np.cos(2 * np.pi * j / ny - ph) + 0.05 * rng.standard_normal((nx + 2, ny + 2))


def _geometry(dims, bmask):
    from mgroms_amd.testcases import seamount_geometry
    nx, ny, _ = dims
    dx, dy, _, h = seamount_geometry(nx, ny, 1, 1, 0)
    rmask = None
    if bmask:
        rmask = (np.random.default_rng(7).random((nx + 2, ny + 2)) < 0.85).astype(np.float64)
    return dx, dy, h, rmask


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _init(mg, dims, bmask=0, **par):
    kw = dict(relax_method="FC", solver_prec=1e-12, bmask=1 if bmask else 0)
    kw.update(par)
    mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(**kw))


def _matrices_host(mg, dims, bmask, which):
    dx, dy, h, rmask = _geometry(dims, bmask)
    mg.nhydro_matrices(dx, dy, _zeta(dims[0], dims[1], which), h, rmask, HC, 0.0, 0.0)


def _matrices_device(mg, dims, bmask, which):
    dx, dy, h, rmask = _geometry(dims, bmask)
    mg.nhydro_matrices_device(_dev(dx), _dev(dy), _dev(_zeta(dims[0], dims[1], which)), _dev(h), _dev(rmask), HC, 0.0, 0.0)


def _update(mg, dims, which):
    mg.nhydro_update_zeta_device(_dev(_zeta(dims[0], dims[1], which)))


def _read_all(mg, bmask):
    names = FIELDS + (("rmask",) if bmask else ())
    return {(lev, n): mg.grid(lev).get(n) for lev in range(1, mg.nlevs() + 1) for n in names}


def _assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for key in want:
        a, b = got[key], want[key]
        assert np.array_equal(a, b), (what, key, np.argwhere(a != b)[:4].tolist())


_REF = {}


def _host_reference(mg, dims, bmask):
    """every field of every level after nhydro_matrices(dx, dy, zeta_c, h[, rmask]) from numpy, on a fresh instance; built once"""
    key = (dims, bmask)
    if key not in _REF:
        mg.nhydro_clean()
        _init(mg, dims, bmask)
        _matrices_host(mg, dims, bmask, "c")
        ref = _read_all(mg, bmask)
        for a in ref.values():
            a.setflags(write=False)
        _REF[key] = ref
        mg.nhydro_clean()
    return _REF[key]


def _uvw(dims, seed=37):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s) for s in ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2)))


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,bmask", SHAPES, ids=IDS)
def test_matrices_device_equals_matrices(mg, dims, bmask):
    """nhydro_matrices from numpy, every field of every level read; nhydro_clean, init again, nhydro_matrices_device from tensors of the
    same data: equal.  zw, cw, cA of level 1 also equal the oracle's."""
    ref = _host_reference(mg, dims, bmask)
    _init(mg, dims, bmask)
    _matrices_device(mg, dims, bmask, "c")
    _assert_same(_read_all(mg, bmask), ref, "matrices_device")
    o = oracle_twin(problem(dims, bmask=bool(bmask), rmask=_geometry(dims, bmask)[3], zeta=_zeta(dims[0], dims[1], "c"), sigma=(HC, 0.0, 0.0),
                            relax_method="FC"))
    for name in ("zw", "cw", "cA"):
        assert np.array_equal(ref[(1, name)], o.field(name)), name


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,bmask", SHAPES, ids=IDS)
def test_refresh_equals_rebuild(mg, dims, bmask):
    """matrices_device(zeta_a), update(zeta_b), update(zeta_c) -- three states catch anything stale that two would hide -- against a fresh
    instance built with nhydro_matrices(zeta_c).  dx, dy, h of every level unchanged by the refreshes.  Every shape here is a single-rank
    closed hierarchy: the one-launch 2-D path may decline none of them, so both counters read 2."""
    ref = _host_reference(mg, dims, bmask)
    _init(mg, dims, bmask)
    _matrices_device(mg, dims, bmask, "a")
    geo0 = {(lev, n): mg.grid(lev).get(n) for lev in range(1, mg.nlevs() + 1) for n in GEO}
    assert mg.nhydro.get_option("zeta_refreshes") == 0
    _update(mg, dims, "b")
    _update(mg, dims, "c")
    got = _read_all(mg, bmask)
    _assert_same(got, ref, "refresh")
    for key, a in geo0.items():
        assert np.array_equal(got[key], a), key
    assert mg.nhydro.get_option("zeta_refreshes") == 2
    assert mg.nhydro.get_option("zeta_chain_launches") == 2


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_two_resident_time_steps_against_the_oracle(mg):
    """The moving-free-surface test with nothing on the host: per step nhydro_update_zeta_device, then nhydro_solve_device (FC, two
    iterations) on tensors; b, p and u, v, w (copied back) equal the oracle's after each step.  Then the device divergence check."""
    import torch
    from oracle.mgoracle import Oracle
    dims = nx, ny, nz = 96, 64, 24
    kw = dict(relax_method="FC", solver_prec=1e-12, solver_maxiter=2)
    _init(mg, dims, 0, **kw)
    o = Oracle(nx, ny, nz, 1, 1, **kw)
    dx, dy, h, _ = _geometry(dims, 0)
    for name, a in (("dx", dx), ("dy", dy), ("h", h)):
        o.field(name)[...] = a
    _matrices_device(mg, dims, 0, "a")
    u, v, w = _uvw(dims)
    o.field("u")[...] = u; o.field("v")[...] = v; o.field("w")[...] = w
    du, dv, dw = (torch.from_numpy(a).cuda() for a in (u, v, w))
    for step, which in enumerate(("b", "c")):
        _update(mg, dims, which)
        o.field("zeta")[...] = _zeta(nx, ny, which)
        o.matrices(HC, 0.0, 0.0)
        mg.nhydro.nhydro_solve_device(du, dv, dw)
        n, _, _ = o.nhydro_solve()
        assert n == 2
        assert np.array_equal(mg.grid(1).b, o.field("b")), step
        assert np.array_equal(mg.grid(1).p, o.field("p")), step
        for name, d in (("u", du), ("v", dv), ("w", dw)):
            assert np.array_equal(d.cpu().numpy(), o.field(name)), (step, name)
    kept = [d.clone() for d in (du, dv, dw)]
    mg.nhydro_check_nondivergence_device(du, dv, dw)
    o.check_nondivergence()
    assert np.array_equal(mg.grid(1).b, o.field("b"))
    for d, k in zip((du, dv, dw), kept):
        assert torch.equal(d, k)   # only read


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def _rb_state(mg, dims):
    win = [(mg.nhydro.rbseq_window_info(lev), mg.nhydro.rbseq_window_rows(lev)) for lev in range(1, mg.nlevs() + 1)]
    rhs(mg, None, uvw(dims))
    n, hist = mg.solve_p(1e-30, 3)
    return win, n, hist, mg.grid(1).p


@pytest.mark.parametrize("dims", [(64, 32, 16), (16, 32, 128)], ids=["64x32x16", "16x32x128"])
def test_red_black_default_after_a_refresh(mg, dims):
    """relax_method = 'RB' in the sequential order (the default): rho, the planes of warm-up and the rows of the windowed walk of every
    level, a 3-iteration solve_p history and p after a refresh equal those of the fresh rebuild."""
    _init(mg, dims, 0, relax_method="RB")
    _matrices_device(mg, dims, 0, "a")
    _update(mg, dims, "b")
    got = _rb_state(mg, dims)
    _init(mg, dims, 0, relax_method="RB")
    _matrices_host(mg, dims, 0, "b")
    want = _rb_state(mg, dims)
    assert got[0] == want[0], (got[0], want[0])
    assert any(rho >= 0 for (rho, _), _ in want[0])   # the levels do have their figures
    assert got[1] == want[1] == 3
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[3], want[3])


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{"coarsest_direct": 2}, {"cycle_precision": 32}, {"krylov": 2, "krylov_precision": 32}],
                         ids=["coarsest_direct", "cycle_precision32", "krylov_precision32"])
def test_dependent_state_is_invalidated(mg, options):
    """The direct coarsest operator and the fp32 copies are built from the coefficients: solve (they now exist), refresh with another
    zeta, solve again -- history and p must be a fresh instance's with the new zeta."""
    dims = (32, 32, 8)
    defaults = {"coarsest_direct": 1, "cycle_precision": 64, "krylov": 0, "krylov_precision": 64}

    def solve():
        rhs(mg, None, uvw(dims))
        n, hist = mg.solve_p(1e-30, 3)
        return n, hist, mg.grid(1).p
    try:
        for k, val in options.items():
            mg.nhydro.set_option(k, val)
        _init(mg, dims, 0)
        _matrices_device(mg, dims, 0, "a")
        solve()
        _update(mg, dims, "b")
        got = solve()
        _init(mg, dims, 0)
        _matrices_host(mg, dims, 0, "b")
        want = solve()
        if "coarsest_direct" in options:
            assert mg.nhydro.get_option("coarsest_direct_solves") > 0
        if "cycle_precision" in options:
            assert mg.nhydro.get_option("mixed_iterations") > 0
        if "krylov" in options:
            assert mg.nhydro.get_option("krylov_mixed_iterations") > 0
    finally:
        for k in options:
            mg.nhydro.set_option(k, defaults[k])   # these options outlive nhydro_clean
    assert got[0] == want[0] == 3
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[2], want[2])


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_process_grid_keeps_the_per_level_path():
    """2 x 2 thread ranks on one GPU at 32x32x16 per rank, nsmall = 8 (a gather level): tests/_gpu_device_timestep_ranks.py"""
    cmd = ["timeout", "-k", "10", "140", sys.executable, os.path.join(HERE, "_gpu_device_timestep_ranks.py"), "2", "2", "32", "32", "16", "8"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-3000:]
    for r in range(4):
        assert f"rank {r} ok" in out.stdout
    assert "gathered_levels=[4]" in out.stdout, out.stdout


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(mg):
    import torch
    from mgroms_amd._lib import MgxError
    dims = nx, ny, nz = 32, 32, 8
    _init(mg, dims, 0)
    z = _zeta(nx, ny, "a")
    with pytest.raises(MgxError, match="mgx_matrices"):
        mg.nhydro_update_zeta_device(_dev(z))
    _matrices_device(mg, dims, 0, "a")
    bad = {"cpu": torch.from_numpy(z), "float32": _dev(z).float(), "transposed": _dev(np.ascontiguousarray(z.T)).t(),
           "shape": _dev(z[:-1])}
    assert not bad["transposed"].is_contiguous() and tuple(bad["transposed"].shape) == (nx + 2, ny + 2)
    dx, dy, h, _ = (_dev(a) for a in _geometry(dims, 0))
    u, v, w = (_dev(a) for a in _uvw(dims))
    for what, t in bad.items():
        with pytest.raises(ValueError):
            mg.nhydro_update_zeta_device(t)
        with pytest.raises(ValueError):
            mg.nhydro_matrices_device(dx, dy, t, h)
        with pytest.raises(ValueError):
            mg.nhydro_check_nondivergence_device(u, v, w, rmask=t)
    with pytest.raises(ValueError):
        mg.nhydro_check_nondivergence_device(u.cpu(), v, w)
    assert mg.nhydro.get_option("zeta_refreshes") == 0
    _init(mg, dims, 1)
    with pytest.raises(MgxError, match=r"bmask=\.true\. needs rmask in mgx_matrices \(nhydro\.f90:52-55\)"):
        mg.nhydro_matrices_device(dx, dy, _dev(z), h, None)


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_async_refresh_gives_the_same_fields(mg):
    """option "async" = 1, four colours: the refresh only enqueues; after synchronize() the fields are those of async = 0"""
    dims, bmask = SHAPES[1]
    ref = _host_reference(mg, dims, bmask)
    _init(mg, dims, bmask)
    _matrices_device(mg, dims, bmask, "a")
    zc = _dev(_zeta(dims[0], dims[1], "c"))   # kept alive until the stream has read it
    mg.nhydro.set_option("async", 1)
    try:
        mg.nhydro_update_zeta_device(zc)
        mg.nhydro.synchronize()
    finally:
        mg.nhydro.set_option("async", 0)   # outlives nhydro_clean
    _assert_same(_read_all(mg, bmask), ref, "async refresh")
    assert mg.nhydro.get_option("zeta_chain_launches") == 1
