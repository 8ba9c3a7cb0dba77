"""The matrices from the caller's own vertical grid on the GPU (include/mgx.h: mgx_matrices_depths*, mgx_update_depths_device).

What is pinned to what:
  1  level 1 IS the caller's grid: the library's own sigma depths handed back give level 1 bit for bit -- zr, zw with their halos, cw, cA,
     the b of compute_rhs and the u, v, w of a solve;
  2  on a flat bottom the coarsening rule of the depths reproduces the whole sigma hierarchy: every level's zr, zw, cA bit for bit, the
     four-colour solve bit for bit, the red-black one within the project's 1e-10;
  3  the kernel is the rule (tests/_depths.py: coarsen_depths) on a grid the library did not make -- ROMS' old S-coordinate on the
     seamount --, on one rank and on 2 x 2 ranks with gathered levels;
  4  the three texts -- matrix, divergence, gradient -- agree on that grid within the project's COUPLING_TOL;
  5  every level's smoother solves its own operator (tests/_smoother_identity.py, its bounds);
  6  the solve converges like the path it replaces;
  7  the strided entry is the dense one with other addresses, and reads nothing but the interior;
  8  the per-step call is a fresh set-up; 9 periodic domains; 10 the refusals, in their words.

Measured on the MI355X (this file's prints): see DESIGN.md 6.4."""
import os
import sys

import numpy as np
import pytest

import _smoother_identity as S
from _depths import assert_monotone, dense, hierarchy, interior, model_arrays, old_s_depths
from _gpu import gpu_module
from _operator_identity import COUPLING_TOL, assert_set_is_meaningful, case_inputs, coupling_defect, water_interior
from _problem import hist_close, uvw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = {"hold_odd_nz": 0, "hold_z_levels": 0, "periodic": 0, "rb_exact": 0, "rb_seq": 1, "async": 0, "warm_start": 0}
mg = gpu_module(**DEFAULTS)


@pytest.fixture(autouse=True)
def _restore_options(mg):
    """after every test: no grid (the options mgx_init reads cannot be set back under a hierarchy built with them), every option at its default"""
    yield
    mg.nhydro_clean()
    for k, v in DEFAULTS.items():
        mg.nhydro.set_option(k, v)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def _init(mg, dims, method="FC", init=None, **par):
    mg.nhydro_clean()
    for k, v in (init or {}).items():
        mg.nhydro.set_option(k, v)
    mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(relax_method=method, **dict(dict(solver_prec=1e-10), **par)))


def _sigma(mg, inp, bmask=False):
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], inp["rmask"] if bmask else None, inp["hc"], inp["theta_b"], inp["theta_s"])


def _levels(mg, names=("zr", "zw", "cA")):
    return [{n: mg.grid(lev).get(n) for n in names} for lev in range(1, mg.nlevs() + 1)]


def _nzs(mg):
    return [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)]


def _same(a, b, what):
    bad = a != b
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same_levels(got, want, what, names=("zr", "zw", "cA")):
    assert len(got) == len(want)
    for lev, (g, w) in enumerate(zip(got, want), 1):
        for n in names:
            _same(g[n], w[n], (what, "level", lev, n))
            assert np.isfinite(g[n]).all(), (what, lev, n)


def _flat(nx, ny):
    """constant h and zeta under a metric that varies in i and j, the stretched sigma set"""
    inp = case_inputs(nx, ny, "seamount", stretched=True, curvilinear=True)
    inp["h"] = np.full((nx + 2, ny + 2), 3000.0)
    inp["zeta"] = np.full((nx + 2, ny + 2), 0.3)
    return inp


def _seamount(nx, ny, mask=False):
    """the seamount under the curvilinear metric and a smooth free surface: dx, dy, rmask and the old-S interiors (zr, zw) over it"""
    inp = case_inputs(nx, ny, "seamount", mask=mask, curvilinear=True)
    return inp, _old_s(inp["h"], nx, ny)


def _zeta(nx, ny, amp=0.4):
    i, j = np.meshgrid(np.arange(nx + 2), np.arange(ny + 2), indexing="ij")
    return amp * np.cos(0.25 * i) * np.sin(0.15 * j)


def _old_s(h, nx, ny, nz=None, amp=0.4):
    def make(nz):
        return old_s_depths(h[1:-1, 1:-1], _zeta(nx, ny, amp)[1:-1, 1:-1], nz)
    return make if nz is None else make(nz)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 16, 8), (64, 32, 64)], ids=["32x16x8", "64x32x64"])
def test_level_1_is_the_callers_grid(mg, dims):
    """nhydro_matrices on the seamount (curvilinear metric, stretched sigma under a rough zeta), its level-1 zr, zw read back and handed to
    nhydro_matrices_depths after a new nhydro_init: zr, zw with their halos (refilled by the library's own rule from the interior alone: the
    halo of what is handed over is NaN here), cw and cA of level 1, and the b of compute_rhs on a random state are bit for bit; so are the
    u, v, w that correct_uvw leaves for a given p.  (The library has no entry for correct_uvw alone: nhydro_solve under "warm_start" = 1 and a
    solver_prec no residual exceeds keeps the p that was set and goes straight from compute_rhs to correct_uvw -- the test checks that it did.
    The coarser levels are NOT those of nhydro_matrices on a seamount, so an iterated p is not compared here.)"""
    nx, ny, nz = dims
    inp = case_inputs(nx, ny, "seamount", stretched=True, curvilinear=True)
    state = uvw(dims, seed=11)
    pset = np.random.default_rng(12).standard_normal((nx + 2, ny + 2, nz))
    out = []
    mg.nhydro.set_option("warm_start", 1)
    try:
        for depths in (False, True):
            _init(mg, dims, solver_prec=1e30)
            if depths:
                zr, zw = out[0]["zr"], out[0]["zw"]
                assert_monotone(interior(zr), interior(zw))
                mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(interior(zr)), dense(interior(zw)))
            else:
                _sigma(mg, inp)
            g = mg.grid(1)
            f = {n: g.get(n) for n in ("zr", "zw", "cw", "cA")}
            mg.nhydro.compute_rhs(*state)
            f["b"] = g.b
            g.set("p", pset); mg.fill_halo(1, "p")
            f["p"] = g.p
            u, v, w = (a.copy() for a in state)
            mg.nhydro_solve(u, v, w)
            _same(g.p, f["p"], "nhydro_solve kept the p that was set")
            f.update(u=u, v=v, w=w)
            out.append(f)
    finally:
        mg.nhydro.set_option("warm_start", 0)
    for n in out[0]:
        _same(out[1][n], out[0][n], (dims, n))
    assert not np.array_equal(out[1]["u"], state[0]) and not np.array_equal(out[1]["w"], state[2])
    # h and zeta stay what they mean: -zw(1) and zw(nz+1), on 0:n+1
    g = mg.grid(1)
    _same(g.h, -out[1]["zw"][1:-1, 1:-1, 0], "h = -zw(1)")
    _same(g.zeta, out[1]["zw"][1:-1, 1:-1, -1], "zeta = zw(nz+1)")


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
FLAT = [((32, 32, 16), {}), ((32, 16, 24), {}), ((64, 32, 64), {}), ((32, 32, 96), {}), ((32, 32, 16), {"hold_z_levels": 1}),
        ((32, 32, 20), {"hold_odd_nz": 1})]


def _flat_pair(mg, dims, init, method, maxit, periodic=0):
    nx, ny, nz = dims
    inp = _flat(nx, ny)
    if periodic:   # a periodic domain needs a periodic metric: the generator's constant dx, dy
        inp = dict(inp, **{k: case_inputs(nx, ny, "seamount")[k] for k in ("dx", "dy")})
    state = uvw(dims, seed=5)
    res = []
    for depths in (False, True):
        _init(mg, dims, method, dict(init, periodic=periodic))
        if depths:
            mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(interior(res[0]["lev"][0]["zr"])), dense(interior(res[0]["lev"][0]["zw"])))
        else:
            _sigma(mg, inp)
        r = {"lev": _levels(mg), "nzs": _nzs(mg)}
        mg.nhydro.compute_rhs(*state)
        r["n"], r["hist"] = mg.solve_p(1e-10, maxit)
        r["p"] = mg.grid(1).p
        res.append(r)
    return res


@pytest.mark.parametrize("dims,init", FLAT, ids=["%dx%dx%d%s" % (d + ("-" + "-".join(i) if i else "",)) for d, i in FLAT])
def test_flat_bottom_equals_the_sigma_hierarchy(mg, dims, init):
    """constant h and zeta, curvilinear dx, dy: every level's zr, zw (interior and halo) and cA are those of nhydro_matrices bit for bit;
    with four colours so are the residual history and p of solve_p(1e-10); with the red-black default the history is within 1e-10.
    32x16x24 ends on an odd nz; 64x32x64 and 32x32x96 are the levels whose colour pass generates from the sigma fields under nhydro_matrices
    and takes the stored coefficients here; the last two hold nz (hold_z_levels on the first pair, hold_odd_nz from nz = 5 on)."""
    sig, dep = _flat_pair(mg, dims, init, "FC", 30)
    assert dep["nzs"] == sig["nzs"]
    _same_levels(dep["lev"], sig["lev"], dims)
    print(dims, init, "FC", sig["n"], sig["hist"][-1], dep["n"], dep["hist"][-1])
    assert dep["n"] == sig["n"] and np.array_equal(dep["hist"], sig["hist"]), (sig["hist"], dep["hist"])
    _same(dep["p"], sig["p"], (dims, "p"))
    assert sig["hist"][-1] < sig["hist"][0] and np.abs(sig["p"]).max() > 0
    sig, dep = _flat_pair(mg, dims, init, "RB", 30)
    print(dims, init, "RB", sig["n"], sig["hist"][-1], dep["n"], dep["hist"][-1])
    _same_levels(dep["lev"], sig["lev"], (dims, "RB"))
    assert hist_close(dep["hist"], sig["hist"], rtol=1e-10, atol=1e-13, same_length=True), (sig["hist"], dep["hist"])


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,init", [((32, 32, 24), {}), ((48, 80, 12), {"hold_z_levels": 2})], ids=["32x32x24", "48x80x12-hold_z_levels-2"])
def test_the_kernel_is_the_rule(mg, dims, init):
    """old-S depths on the seamount: every level's zr, zw interior is coarsen_depths of the level above, bit for bit"""
    nx, ny, nz = dims
    inp, make = _seamount(nx, ny)
    zr, zw = make(nz)
    _init(mg, dims, "FC", init)
    mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw))
    nzs = _nzs(mg)
    if init:
        assert nzs[:3] == [nz] * 3
    want = hierarchy(zr, zw, nzs)
    for lev, (wr, ww) in enumerate(want, 1):
        g = mg.grid(lev)
        _same(interior(g.zr), wr, (dims, lev, "zr"))
        _same(interior(g.zw), ww, (dims, lev, "zw"))
        assert np.isfinite(g.zr).all() and np.isfinite(g.zw).all() and np.isfinite(g.get("cA")).all()


def test_the_kernel_is_the_rule_on_2x2_ranks(mg):
    """32 x 32 x 16 on 2 x 2 ranks of 16 x 16 x 16 with nsmall = 8 (gathered levels): every rank's zr, zw of every level are its block of
    the rule applied to the global depths, and its blocks of cA and of p after solve_p equal the one-rank run bit for bit (four colours)"""
    from _ranks import free_port, run_process_ranks
    mg.nhydro_clean()
    run_process_ranks(os.path.join(HERE, "_gpu_depths_grid_worker.py"), 4, [4, 2, 2, free_port(), 16, 16, 16, 8], timeout=150)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
class _Gpu:
    """coupling_defect's three calls on the library (as tests/test_gpu_operator_identity.py has them)"""

    def __init__(self, mg):
        self.mg = mg

    def solve(self, u, v, w, rmask):
        self.mg.nhydro_solve(u, v, w, rmask)

    def rhs(self, u, v, w, rmask):
        self.mg.nhydro.compute_rhs(u, v, w, rmask)
        return self.mg.grid(1).b[1:-1, 1:-1, :]

    def residual(self):
        self.mg.compute_residual(1)
        return self.mg.grid(1).r[1:-1, 1:-1, :]


@pytest.mark.parametrize("dims,mask", [((32, 16, 8), False), ((64, 32, 64), False), ((32, 32, 8), True)], ids=["32x16x8", "64x32x64", "island-32x32x8"])
def test_the_three_texts_agree_on_a_grid_the_library_did_not_make(mg, dims, mask):
    """coupling_defect (tests/_operator_identity.py) through the model-facing calls with old-S depths: b' = r on the water-interior set
    within COUPLING_TOL, the project's own bound (16 x the oracle's largest measurement).  The identity is a property of the matrix, the
    divergence and the gradient on ONE set of depths, whatever coordinate made them."""
    nx, ny, nz = dims
    inp, make = _seamount(nx, ny, mask)
    zr, zw = make(nz)
    _init(mg, dims, "FC", solver_prec=1e-30, solver_maxiter=2, bmask=1 if mask else 0)
    mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw), inp["rmask"] if mask else None)
    assert_set_is_meaningful(water_interior(inp["rmask"], nx, ny), inp["rmask"])
    f = coupling_defect(_Gpu(mg), nx, ny, nz, inp["rmask"], 1)
    print("coupling defect", dims, mask, f)
    assert np.abs(mg.grid(1).p).max() > 0 and f["Ap_over_b"] > 1e-3, f
    assert f["defect"] <= COUPLING_TOL, (dims, f)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,options", [("FC", {}), ("RB", {}), ("RB", {"rb_exact": 1}), ("GS", {})], ids=["FC", "RB", "RB-rb_exact", "GS"])
def test_every_levels_smoother_solves_its_own_operator(mg, method, options):
    """the checks of tests/_smoother_identity.py on every level of the old-S hierarchy at 32 x 32 x 16, with that file's bounds"""
    dims = (32, 32, 16)
    inp, make = _seamount(32, 32)
    zr, zw = make(16)
    _init(mg, dims, method)
    for k, v in options.items():
        mg.nhydro.set_option(k, v)
    mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw))
    be = S.GpuBackend(mg)
    rb_seq = method == "RB" and not options.get("rb_exact")
    for lev in range(1, mg.nlevs() + 1):
        f = S.run_level(be, lev, method, True, S.SEEDS[0], rb_seq=rb_seq)
        print(method, options, "level", lev, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in f.items() if k != "tol"})
        S.assert_level(f, (method, options, lev))


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", [{}, {"hold_z_levels": 1}], ids=["64x64x16", "64x64x16-hold_z_levels-1"])
def test_it_converges_like_the_path_it_replaces(mg, init):
    """the seamount, four colours, to 1e-10 within solver_maxiter = 50: the library's own sigma depths handed back through the new entry are
    the same problem on level 1 and coarse levels 5e-6 ... 5e-4 of the depth away; the count is at most that of nhydro_matrices plus one (the
    stopping test is a threshold: a perturbed contraction can move the crossing by one iteration).  The old-S grid at the same size must
    reach 1e-10 within the 50; its count is recorded, not bounded."""
    dims = nx, ny, nz = 64, 64, 16
    inp = case_inputs(nx, ny, "seamount")
    state = uvw(dims, seed=7)
    counts = {}
    for what in ("sigma", "sigma depths", "old S"):
        _init(mg, dims, "FC", init, solver_maxiter=50)
        if what == "sigma":
            _sigma(mg, inp)
            g = mg.grid(1)
            lib_zr, lib_zw = interior(g.zr), interior(g.zw)
        elif what == "sigma depths":
            mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(lib_zr), dense(lib_zw))
        else:
            mg.nhydro_matrices_depths(inp["dx"], inp["dy"], *(dense(a) for a in _old_s(inp["h"], nx, ny, nz)))
        mg.nhydro.compute_rhs(*state)
        n, hist = mg.solve_p(1e-10, 50)
        counts[what] = n
        print("iterations to 1e-10,", what, init, n, hist[-1])
        assert hist[-1] <= 1e-10 and n < 50, (what, n, hist)
    assert counts["sigma depths"] <= counts["sigma"] + 1, counts


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 16, 8), (24, 16, 12)], ids=["32x16x8", "24x16x12"])
def test_strides(mg, dims):
    """the depths in i-fastest tensors with 2 and 3 ghost cells per side and a padded pitch, ghost cells and padding NaN: every level's zr,
    zw, cA and the solve are those of the dense entry bit for bit and finite; the caller's arrays come back unchanged, NaN included"""
    import torch
    nx, ny, nz = dims
    inp, make = _seamount(nx, ny)
    zr, zw = make(nz)
    state = uvw(dims, seed=9)
    dx, dy = _dev(inp["dx"]), _dev(inp["dy"])

    def run(set_up):
        _init(mg, dims, "FC")
        set_up()
        mg.nhydro.compute_rhs(*state)
        n, hist = mg.solve_p(1e-10, 10)
        return _levels(mg), hist, mg.grid(1).p

    ref = run(lambda: mg.nhydro_matrices_depths_device(dx, dy, _dev(dense(zr)), _dev(dense(zw))))
    host = run(lambda: mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw)))
    _same_levels(host[0], ref[0], (dims, "host entry"))
    for ghost, pad in ((2, 3), (3, 0)):
        ZR, ZW, sl = model_arrays(zr, zw, ghost, pad)
        tr, tw = _dev(ZR), _dev(ZW)
        got = run(lambda: mg.nhydro_matrices_depths_device(dx, dy, tr[sl], tw[sl]))
        _same_levels(got[0], ref[0], (dims, ghost, pad))
        assert np.array_equal(got[1], ref[1]) and np.isfinite(got[1]).all()
        _same(got[2], ref[2], (dims, ghost, pad, "p"))
        torch.cuda.synchronize()
        assert np.array_equal(tr.cpu().numpy().view(np.int64), ZR.view(np.int64)) and np.array_equal(tw.cpu().numpy().view(np.int64), ZW.view(np.int64))
        # the per-step call through the same strides
        mg.nhydro_update_depths_device(tr[sl], tw[sl])
        _same_levels(_levels(mg), ref[0], (dims, ghost, pad, "update"))


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------
def _window(mg):
    return [mg.nhydro.rbseq_window_info(lev) + (mg.nhydro.rbseq_window_rows(lev),) for lev in range(1, mg.nlevs() + 1)]


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_the_per_step_call_is_a_fresh_set_up(mg, method):
    """nhydro_update_depths_device with the depths of a new zeta: every level's zr, zw, cA, the red-black window figures and a solve (which
    reads the pivots) equal a fresh nhydro_matrices_depths_device bit for bit; "depth_refreshes" counts; under "async" = 1 the call enqueues
    and synchronize() leaves the same fields; nhydro_update_zeta_device is refused afterwards, with the reason."""
    from mgroms_amd._lib import MgxError
    dims = nx, ny, nz = 32, 32, 16
    inp = case_inputs(nx, ny, "seamount", curvilinear=True)
    a = [_dev(dense(x)) for x in _old_s(inp["h"], nx, ny, nz, amp=0.4)]
    b = [_dev(dense(x)) for x in _old_s(inp["h"], nx, ny, nz, amp=-0.7)]
    dx, dy = _dev(inp["dx"]), _dev(inp["dy"])
    state = uvw(dims, seed=13)

    def read():
        mg.nhydro.compute_rhs(*state)
        n, hist = mg.solve_p(1e-10, 8)
        return _levels(mg), _window(mg), hist, mg.grid(1).p

    _init(mg, dims, method)
    mg.nhydro_matrices_depths_device(dx, dy, *b)
    fresh = read()
    _init(mg, dims, method)
    mg.nhydro_matrices_depths_device(dx, dy, *a)
    first = _levels(mg)
    assert mg.nhydro.get_option("depth_refreshes") == 0
    mg.nhydro_update_depths_device(*b)
    assert mg.nhydro.get_option("depth_refreshes") == 1
    got = read()
    assert not np.array_equal(first[0]["zw"], got[0][0]["zw"])
    _same_levels(got[0], fresh[0], (method, "update"))
    assert got[1] == fresh[1], (got[1], fresh[1])
    assert np.array_equal(got[2], fresh[2])
    _same(got[3], fresh[3], (method, "p"))
    mg.nhydro.set_option("async", 1)
    try:
        mg.nhydro_update_depths_device(*a)
        mg.nhydro.synchronize()
    finally:
        mg.nhydro.set_option("async", 0)
    _same_levels(_levels(mg), first, (method, "async"))
    assert mg.nhydro.get_option("depth_refreshes") == 2
    with pytest.raises(MgxError, match="mgx_update_zeta_device: the depths in use are the caller's .*no h and no stretching to apply a new zeta to"):
        mg.nhydro_update_zeta_device(_dev(np.zeros((nx + 2, ny + 2))))
    # the library's own grid again: the refusal is gone and the refresh serves
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], None, 4e3, 0.0, 0.0)
    mg.nhydro_update_zeta_device(_dev(_zeta(nx, ny, 0.1)))


def test_nhydro_matrices_after_depths_is_a_process_that_never_saw_them(mg):
    """two processes side by side: one runs nhydro_matrices and a solve; the other first sets up and solves on old-S depths, then runs the
    same nhydro_matrices and solve in the same hierarchy.  p (its digest) and the growth of every counter of mgx_counters over
    nhydro_matrices + compute_rhs + solve_p are equal: the flag is cleared and the generated fields are back."""
    from _ranks import run_commands
    mg.nhydro_clean()
    worker = os.path.join(HERE, "_gpu_depths_after_worker.py")
    res = run_commands([([sys.executable, worker, mode], None) for mode in ("fresh", "after")], timeout=120)
    lines = []
    for r in res:
        assert r.returncode == 0, r.stdout + r.stderr
        lines.append([l for l in r.stdout.splitlines() if l.startswith("RESULT ")])
        print(r.stdout[-600:])
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------
def test_periodic_flat_bottom_equals_the_sigma_hierarchy(mg):
    """"periodic" = 3 at 32 x 32 x 16: the halos of the depths wrap, and the flat-bottom equality of test 2 holds"""
    sig, dep = _flat_pair(mg, (32, 32, 16), {}, "FC", 30, periodic=3)
    _same_levels(dep["lev"], sig["lev"], "periodic")
    assert dep["n"] == sig["n"] and np.array_equal(dep["hist"], sig["hist"])
    _same(dep["p"], sig["p"], "periodic p")


SHIFTS = [("RB", {"rb_seq": 0, "coarsest_direct": 0}, 8), ("FC", {}, 16)]


@pytest.mark.parametrize("method,options,shift", SHIFTS, ids=["red-black-parallel-8", "four-colours-16"])
def test_periodic_shift(mg, method, options, shift):
    """"periodic" = 3, old-S depths on the seamount under the uniform metric: depths and right-hand side shifted by (shift, shift) columns
    give the shifted p bit for bit, and every level's depths are the shifted depths.

    Which smoother can be asked for which shift.  The hierarchy of 32 x 32 x 16 is 32, 16, 8, 4 columns wide, so a shift by (8, 8) on
    level 1 is a shift by (1, 1) on level 4.  A solve is the same arithmetic per cell after a shift exactly when the shift maps every
    colour of the smoother onto itself on every level, and the sweep within a colour does not depend on the order of its columns:
      * red-black colours are the parity of i + j, which ANY diagonal shift keeps; the parallel colour pass ("rb_seq" = 0: same-colour
        couplings of the bottom row read from a snapshot) has no order within a colour; the coarsest level runs its sweeps
        ("coarsest_direct" = 0: the product with the built operator sums over the cells in storage order).  (8, 8) is asked of it.
      * four colours are the parities of i and of j: (1, 1) on level 4 exchanges (odd, odd), the first colour, with (even, even), the
        last, and the 40 sweeps of the coarsest solve run in another order -- another iterate, equal only to rounding (measured on the
        MI355X: max |p - shifted p| = 4.3e-18 under max |p| = 7.0e-3 after six iterations).  Four colours are shift-invariant for shifts
        that are even on every level, here multiples of 16 (tests/test_gpu_hold_z.py rolls by sixteen for the same reason): (16, 16).
      * the sequential-order red-black default walks the planes i = 1 .. nx in order and is not shift-invariant along i at all."""
    dims = nx, ny, nz = 32, 32, 16
    inp = case_inputs(nx, ny, "seamount")
    zr, zw = _old_s(inp["h"], nx, ny, nz)
    b = np.random.default_rng(21).standard_normal((nx, ny, nz))
    b -= b.mean()
    out = []
    keep = {k: mg.nhydro.get_option(k) for k in options}
    try:
        for sh in (0, shift):
            roll = lambda x, sh=sh: np.roll(x, (sh, sh), axis=(0, 1))
            _init(mg, dims, method, dict(options, periodic=3))
            mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(roll(zr)), dense(roll(zw)))
            g = mg.grid(1)
            full = np.zeros(g._shape("b")); full[1:-1, 1:-1, :] = roll(b)
            g.set("b", full)
            n, hist = mg.solve_p(1e-10, 6)
            out.append((hist, g.p[1:-1, 1:-1, :], [interior(mg.grid(lev).zw) for lev in range(1, mg.nlevs() + 1)], roll))
    finally:
        mg.nhydro_clean()
        for k, v in keep.items():
            mg.nhydro.set_option(k, v)
    hist0, p0, zw0, _ = out[0]
    hist1, p1, zw1, roll = out[1]
    print("periodic shift", method, shift, "histories", hist0, hist1, "max |p - shifted p|", np.abs(p1 - roll(p0)).max(), "of", np.abs(p0).max())
    assert len(zw0) == 4
    for lev, (a0, a1) in enumerate(zip(zw0, zw1), 1):   # the depths of every level are the shifted depths
        _same(a1, np.roll(a0, (shift >> (lev - 1), shift >> (lev - 1)), axis=(0, 1)), ("zw", lev))
    assert hist0[-1] < hist0[0] and np.abs(p0).max() > 0
    _same(p1, roll(p0), ("shifted p", method, shift))


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mg):
    import ctypes
    from mgroms_amd._lib import DepthStrides, MgxError, lib
    L = lib()
    nx, ny, nz = 32, 16, 8
    inp, make = _seamount(nx, ny)
    zr, zw = (dense(a) for a in make(nz))
    mg.nhydro_clean()
    with pytest.raises(MgxError, match="mgx_init has not been called"):
        mg.nhydro_matrices_depths(inp["dx"], inp["dy"], zr, zw)
    _init(mg, (nx, ny, nz))
    with pytest.raises(MgxError, match="mgx_update_depths_device: no dx, dy to keep"):
        mg.nhydro_update_depths_device(_dev(zr), _dev(zw))
    keep = _dev(inp["dx"])
    d = keep.data_ptr()
    assert L.mgx_matrices_depths_device(d, d, None, d, None, None) == 1 and b"mgx_matrices_depths_device: zr or zw is NULL" in L.mgx_last_error()
    assert L.mgx_matrices_depths_device(None, d, d, d, None, None) == 1 and b"mgx_matrices_depths_device: dx or dy is NULL" in L.mgx_last_error()
    bad = DepthStrides(nx - 1, nx * ny, nx, nx * ny)
    assert L.mgx_matrices_depths_device(d, d, d, d, ctypes.byref(bad), None) == 1
    assert b"mgx_matrices_depths_device: zr_sj = 31 is below the row length of zr, 32: rows would overlap" in L.mgx_last_error()
    assert not mg.nhydro.get_option("depth_refreshes")
    with pytest.raises(MgxError, match="no matrix|mgx_matrices must be called"):   # nothing of the refused calls was installed
        mg.solve_p(1e-10, 1)
    # a halving from an odd nz: 64 x 64 x 40 is 40, 20, 10, 5, 2
    _init(mg, (64, 64, 40))
    i64, make = _seamount(64, 64)
    z = [dense(a) for a in make(40)]
    with pytest.raises(MgxError, match=r"the depths of level 4 \(nz = 5\) have no coarsening onto level 5 \(nz = 2\).*hold_odd_nz"):
        mg.nhydro_matrices_depths(i64["dx"], i64["dy"], *z)
    _init(mg, (64, 64, 40), init={"hold_odd_nz": 1})
    mg.nhydro_matrices_depths(i64["dx"], i64["dy"], *z)
    assert _nzs(mg)[3:] == [5] * (mg.nlevs() - 3)
    # bmask without rmask
    _init(mg, (nx, ny, nz), bmask=1)
    with pytest.raises(MgxError, match=r"bmask=.true. needs rmask in mgx_matrices_depths"):
        mg.nhydro_matrices_depths(inp["dx"], inp["dy"], zr, zw)


def test_fp32_cycles_are_served(mg):
    """"cycle_precision" = 32 after a depth set-up: the fp32 copies are conversions of the stored fp64 fields (no fp32 kernel generates from
    the sigma tables), so the mixed solve runs and reaches the tolerance of its fp64 twin"""
    dims = nx, ny, nz = 32, 32, 16
    inp, make = _seamount(nx, ny)
    zr, zw = make(nz)
    _init(mg, dims, "FC")
    mg.nhydro_matrices_depths(inp["dx"], inp["dy"], dense(zr), dense(zw))
    state = uvw(dims, seed=3)
    mg.nhydro.compute_rhs(*state)
    n64, h64 = mg.solve_p(1e-9, 30)
    mg.nhydro.set_option("cycle_precision", 32)
    try:
        mg.nhydro.compute_rhs(*state)
        n32, h32 = mg.solve_p(1e-9, 30)
        assert mg.nhydro.get_option("mixed_iterations") == n32
    finally:
        mg.nhydro.set_option("cycle_precision", 64)
    print("fp64", n64, h64[-1], "fp32 cycles", n32, h32[-1])
    assert h64[-1] <= 1e-9 and n64 < 30 and h32[-1] <= 1e-9 and 0 < n32 < 30
