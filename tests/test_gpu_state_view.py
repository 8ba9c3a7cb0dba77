"""The resident time step on the model's own padded arrays: nhydro_solve_view, nhydro_check_nondivergence_view and
nhydro_update_zeta_view (include/mgx.h: the *_view entries) against the dense device entries they are twins of.

Contract: the addresses differ, nothing else.  So every comparison is bit for bit -- u, v, w as integers, b, p, the residual history and the
iteration count equal -- and every element of the padded storage outside the views keeps the bits of the NaN sentinel it was filled with
(tests/_state_view.py: ghost widths 3/2 in i, 2/3 in j, 1/0 in k, an odd row pitch).  Seamount, state uniform in (-1, 1) without a zero.

Shapes, the smallest that reach every addressing path: 12x8x8 (nx != ny, inside one block; two levels -- 12x10x8 is no shape of this library:
mgx_init refuses its second level, 6x5x4, as odd), 40x6x4 (i crosses a block boundary at 32 and
the 64-lane row of the model kernels holds nx + 2 = 42 of them; ny + 1 and ny + 2 rows differ) and 8x8x16, where the runs of the flux
kernels and of correct_uvw split in two along blockIdx.z (the layout function below, the arithmetic of choose_model_run)."""
import os

import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem
from _ranks import free_port, run_process_ranks
from _state_view import bits, padded, padding_untouched, state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
mg = gpu_module()
_restore_options = restore_options("async")

SHAPES = [(12, 8, 8), (40, 6, 4), (8, 8, 16)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
DTYPES = [np.float64, np.float32]
PAR = dict(relax_method="FC", solver_prec=1e-9, solver_maxiter=4)


def _runs(ni, nj, klast):
    """row counts of the runs the flux kernels and correct_uvw launch over rows 1..klast (choose_model_run, mgx_choice_transfer.h, without
    MGX_MODEL_KR: the text of tests/test_gpu_model_coupling.py::_runs)"""
    waves = -(-ni // 64) * nj
    nrun = min(max(-(-16384 // waves), 1), -(-klast // 8))
    kr = -(-klast // nrun)
    nb = -(-klast // kr)
    return [kr] * (nb - 1) + [klast - kr * (nb - 1)]


def test_the_shape_list_reaches_every_addressing_path():
    nx, ny, nz = SHAPES[2]
    assert _runs(nx + 1, ny, nz) == [8, 8] and _runs(nx, ny + 1, nz) == [8, 8] and _runs(nx + 2, ny + 2, nz) == [8, 8]   # uf, vf, correct_uvw
    assert len(_runs(nx, ny, nz + 1)) >= 2                                                                              # wf
    for nx, ny, nz in SHAPES[:2]:
        assert len(_runs(nx + 2, ny + 2, nz)) == 1
    assert SHAPES[0][0] != SHAPES[0][1] and SHAPES[0][0] + 2 <= 32 and SHAPES[1][0] > 32


def _solve(mg, fn, uvw, rmask, tmp_path):
    """fn(u, v, w, rmask) with the history of THIS call from fort.100 (written when verbose, 17 significant digits: exact); returns
    (p, b, history, iterations, launches and the other counters the call added)"""
    f = tmp_path / "fort.100"
    if f.exists():
        f.unlink()
    c0 = mg.nhydro.counters()
    mg.nhydro.set_verbose(1)
    try:
        fn(*uvw, rmask)
    finally:
        mg.nhydro.set_verbose(0)
    c1 = mg.nhydro.counters()
    rows = [ln.split() for ln in f.read_text().splitlines()]
    return mg.grid(1).p, mg.grid(1).b, np.array([float(r[0]) for r in rows]), len(rows) - 1, {k: c1[k] - c0[k] for k in c0}


def _compare(mg, s, rmask, tmp_path, what, solved=True):
    """the dense device entries on contiguous clones against the view entries on padded storage: the divergence check, then the solve"""
    import torch
    dense = [torch.from_numpy(a).cuda() for a in s]
    stores, views = zip(*(padded(torch, a) for a in s))
    rm = None if rmask is None else torch.from_numpy(np.ascontiguousarray(rmask)).cuda()
    # nhydro_check_nondivergence: only reads
    mg.nhydro.nhydro_check_nondivergence_device(*dense, rm)
    b_dense = mg.grid(1).b
    mg.nhydro.nhydro_check_nondivergence_view(*views, rm)
    assert np.array_equal(mg.grid(1).b, b_dense) and np.any(b_dense != 0), what
    for n, a, d, st, v in zip("uvw", s, dense, stores, views):
        assert torch.equal(bits(torch, v), bits(torch, torch.from_numpy(a).cuda())) and torch.equal(bits(torch, d), bits(torch, v)), (what, n, "check wrote")
        assert padding_untouched(torch, st, v) == (True, 0), (what, n, "check")
    # nhydro_solve.  One solve of a scratch copy first: what the first solve after nhydro_matrices builds once (the direct coarsest operator of
    # sequential-order red-black) is then there for both sides, and the counters of the two calls compare
    mg.nhydro.nhydro_solve_device(*[d.clone() for d in dense], rm)
    p0, b0, h0, n0, c0 = _solve(mg, mg.nhydro.nhydro_solve_device, dense, rm, tmp_path)
    p1, b1, h1, n1, c1 = _solve(mg, mg.nhydro.nhydro_solve_view, views, rm, tmp_path)
    print(what, "nite", n0, n1, "hist", h0.tolist(), "counters", c0, c1)
    if solved:
        assert n0 >= 1
    assert n1 == n0 and np.array_equal(h1, h0), (what, n0, n1, h0, h1)
    assert np.array_equal(b1, b0) and np.array_equal(p1, p0), what
    assert c1 == c0, (what, c0, c1)
    for n, a, d, st, v in zip("uvw", s, dense, stores, views):
        assert torch.equal(bits(torch, v), bits(torch, d)), (what, n, int((bits(torch, v) != bits(torch, d)).sum()))
        assert not torch.equal(bits(torch, d), bits(torch, torch.from_numpy(a).cuda())), (what, n, "the solve corrected nothing")
        assert padding_untouched(torch, st, v) == (True, 0), (what, n, "solve")
    return dense, c0


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_view_entries_equal_the_dense_entries(mg, dims, dtype, tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)
    gpu_problem(mg, dims, **PAR)
    s = state(dims, seed=dims[2] + 3, dtype=dtype)
    dense, c_dense = _compare(mg, s, None, tmp_path, (dims, dtype.__name__))
    # a view that happens to be dense: the same bits and the same counters as the dense entry
    again = [torch.from_numpy(a).cuda() for a in s]
    assert all(t.is_contiguous() for t in again)
    _, _, _, _, c_view = _solve(mg, mg.nhydro.nhydro_solve_view, again, None, tmp_path)
    assert c_view == c_dense, (c_view, c_dense)
    for n, d, v in zip("uvw", dense, again):
        assert torch.equal(bits(torch, v), bits(torch, d)), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_bmask_and_a_mask_of_the_call(mg, dtype, tmp_path, monkeypatch):
    """bmask with the island mask in the matrices and another, random mask with the call (dense, as in the dense entries)"""
    monkeypatch.chdir(tmp_path)
    dims = nx, ny, nz = SHAPES[0]
    gpu_problem(mg, dims, bmask=True, **PAR)
    rmask = (np.random.default_rng(5).random((nx + 2, ny + 2)) < 0.8).astype(np.float64)
    assert 0 < rmask.sum() < rmask.size
    _compare(mg, state(dims, seed=21, dtype=dtype), rmask, tmp_path, ("bmask", dtype.__name__))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_red_black(mg, dtype, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    dims = SHAPES[0]
    gpu_problem(mg, dims, **dict(PAR, relax_method="RB"))
    _compare(mg, state(dims, seed=22, dtype=dtype), None, tmp_path, ("RB", dtype.__name__))


def test_views_on_a_2x2_process_grid():
    """2 x 2 ranks of 8x8x4 (tests/_gpu_state_view_ranks.py): every rank's view call against that rank's dense call, float64 and float32"""
    npx, npy, nx, ny, nz = 2, 2, 8, 8, 4
    run_process_ranks(os.path.join(HERE, "_gpu_state_view_ranks.py"), npx * npy, [npx * npy, npx, npy, free_port(), nx, ny, nz])


# ---- zeta ------------------------------------------------------------------------------------------------------------------------------
def _moving_zeta(nx, ny, ph, seed):
    """a free surface in the model's order: (ny + 2, nx + 2), i fastest"""
    i = np.arange(nx + 2, dtype=np.float64)[None, :]
    j = np.arange(ny + 2, dtype=np.float64)[:, None]
    return 0.8 * np.sin(2 * np.pi * i / nx + ph) * np.cos(2 * np.pi * j / ny - ph) + 0.05 * np.random.default_rng(seed).standard_normal((ny + 2, nx + 2))


def _after_refresh(mg, dims, s):
    """what a refresh leaves: cA of every level, zr, zw of level 1 and -- through a compute_rhs of s -- the model-space copies"""
    out = {("cA", lev): mg.grid(lev).get("cA") for lev in range(1, mg.nlevs() + 1)}
    out.update({(n, lev): mg.grid(lev).get(n) for n in ("zeta", "zr", "zw", "cw") for lev in range(1, mg.nlevs() + 1)})
    mg.nhydro.nhydro_check_nondivergence_device(*s)
    out["b"] = mg.grid(1).b
    return out


@pytest.mark.parametrize("async_", [0, 1], ids=["waits", "async"])
@pytest.mark.parametrize("dims", SHAPES[:2], ids=IDS[:2])
def test_zeta_from_a_pitched_i_fastest_array(mg, dims, async_):
    import torch
    nx, ny, nz = dims
    gpu_problem(mg, dims, **PAR)
    s = [torch.from_numpy(a).cuda() for a in state(dims, seed=23, dtype=np.float64)]
    za, zb = _moving_zeta(nx, ny, 0.4, 41), _moving_zeta(nx, ny, 1.7, 42)
    dense = torch.from_numpy(zb).cuda().T.contiguous()
    assert tuple(dense.shape) == (nx + 2, ny + 2)
    store, view = padded(torch, zb[None])
    store, view = store[1], view[0]
    assert tuple(view.shape) == (ny + 2, nx + 2) and view.stride(0) % 2 == 1 and view.stride(0) > nx + 2

    def refresh(fn, z):
        mg.nhydro.nhydro_update_zeta_device(torch.from_numpy(za).cuda().T.contiguous())   # a state in between: nothing of zb is left over
        c0, r0 = mg.nhydro.counters(), mg.nhydro.get_option("zeta_refreshes")
        mg.nhydro.set_option("async", async_)
        try:
            fn(z)
            mg.nhydro.synchronize()
        finally:
            mg.nhydro.set_option("async", 0)
        c1 = mg.nhydro.counters()
        assert mg.nhydro.get_option("zeta_refreshes") == r0 + 1
        return _after_refresh(mg, dims, s), {k: c1[k] - c0[k] for k in c0}

    want, c_dense = refresh(mg.nhydro.nhydro_update_zeta_device, dense)
    got, c_view = refresh(mg.nhydro.nhydro_update_zeta_view, view)
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key], want[key]), (key, np.argwhere(got[key] != want[key])[:4].tolist())
    assert np.array_equal(want[("zeta", 1)][1:-1, 1:-1], zb.T[1:-1, 1:-1])   # (the halo is the library's to fill)
    assert c_view == dict(c_dense, launches=c_dense["launches"] + 1), (c_view, c_dense)   # the transpose, and nothing else
    b = store.view(torch.int64).clone()
    b[2:2 + ny + 2, 3:3 + nx + 2] = 0x7FF80000DEADBEEF
    assert bool((b == 0x7FF80000DEADBEEF).all())   # only read


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(mg):
    import torch
    from mgroms_amd._lib import MgxError
    dims = nx, ny, nz = SHAPES[0]
    mg.nhydro_clean()
    mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(**PAR))
    s64 = state(dims, seed=24, dtype=np.float64)
    views = [padded(torch, a)[1] for a in s64]
    for fn, entry in ((mg.nhydro_solve_view, "mgx_solve_device_view"), (mg.nhydro_check_nondivergence_view, "mgx_check_nondivergence_device_view")):
        with pytest.raises(MgxError, match="mgx_matrices must be called before " + entry):
            fn(*views)
    with pytest.raises(MgxError, match="mgx_update_zeta_device_view: no dx, dy, h to keep"):
        mg.nhydro_update_zeta_view(torch.zeros((ny + 2, nx + 2), dtype=torch.float64, device="cuda"))
    gpu_problem(mg, dims, **PAR)
    before = [v.clone() for v in views]
    for fn in (mg.nhydro_solve_view, mg.nhydro_check_nondivergence_view):
        # a stride along i that is not 1
        wide = torch.zeros((nz, ny + 2, 2 * (nx + 1)), dtype=torch.float64, device="cuda")[:, :, ::2]
        assert tuple(wide.shape) == tuple(views[0].shape) and wide.stride(2) == 2
        with pytest.raises(ValueError, match="stride 1 along i"):
            fn(wide, views[1], views[2])
        with pytest.raises(ValueError, match="stride 1 along i"):
            fn(views[0], views[1], views[2].transpose(1, 2).contiguous().transpose(1, 2))
        # mixed dtypes, a wrong shape, a host tensor
        with pytest.raises(ValueError, match="one dtype"):
            fn(views[0], views[1].float(), views[2])
        with pytest.raises(ValueError, match="shape"):
            fn(views[0][:, :, :-1], views[1], views[2])
        with pytest.raises(ValueError):
            fn(views[0].cpu(), views[1], views[2])
        # overlapping rows: the library's refusal, in its words
        base = torch.zeros(nz * (ny + 2) * (nx + 1), dtype=torch.float64, device="cuda")
        lap = torch.as_strided(base, (nz, ny + 2, nx + 1), (nx * (ny + 2), nx, 1))
        with pytest.raises(MgxError, match=r"u_sj = %d is below the row length of u, %d" % (nx, nx + 1)):
            fn(lap, views[1], views[2])
        lap = torch.as_strided(base, (nz, ny + 2, nx + 1), ((nx + 1) * (ny + 2) - 1, nx + 1, 1))
        with pytest.raises(MgxError, match=r"u_sk = %d is below u_sj x rows" % ((nx + 1) * (ny + 2) - 1)):
            fn(lap, views[1], views[2])
        flat = views[2][:1].expand(nz + 1, ny + 2, nx + 2)   # a level stride of zero
        with pytest.raises(MgxError, match=r"w_sk = 0"):
            fn(views[0], views[1], flat)
    for v, b in zip(views, before):
        assert torch.equal(bits(torch, v), bits(torch, b))   # nothing ran
    # the dense entries keep refusing what is not contiguous
    for fn in (mg.nhydro.nhydro_solve_device, mg.nhydro_check_nondivergence_device):
        with pytest.raises(ValueError, match="contiguous"):
            fn(*views)
    # zeta
    r0 = mg.nhydro.get_option("zeta_refreshes")
    z = torch.zeros((ny + 2, 2 * (nx + 2)), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="stride 1 along i"):
        mg.nhydro_update_zeta_view(z[:, ::2])
    with pytest.raises(ValueError, match="shape"):
        mg.nhydro_update_zeta_view(z[:, :nx + 2].T)
    with pytest.raises(ValueError):
        mg.nhydro_update_zeta_view(z[:, :nx + 2].float())
    with pytest.raises(MgxError, match=r"sj = %d is below the row length of zeta, %d" % (nx + 1, nx + 2)):
        mg.nhydro_update_zeta_view(torch.as_strided(z, (ny + 2, nx + 2), (nx + 1, 1)))
    assert mg.nhydro.get_option("zeta_refreshes") == r0
