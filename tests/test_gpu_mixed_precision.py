"""Mixed-precision solve_p (option "cycle_precision" = 32): fp32 F-cycles in correction form under the fp64 refinement loop.

Operators: every fp32 kernel of the cycle, through mgx_mixed_op, against the fp64 operator of the same name on the same input
(levels 1, 2 and the coarsest; |diff|_inf <= 1e-5 of the fp64 result's max: a few fp32 roundings of every term).
Solves: cold start, solver_prec = 1e-12.  The accuracy contract is the fp64 relative residual, so it is checked independently with
the CPU oracle's fp64 residual of the returned p.

Why ||p_mixed - p_fp64||_inf <= 1e-8 max|p_fp64| follows from two solves converged to 1e-12: both solve A p = b, so
p_mixed - p_fp64 = A^-1 (r_fp64 - r_mixed) with ||r_fp64 - r_mixed|| <= 2e-12 ||b||.  The relative difference is therefore at most
cond(A) * 2e-12, and what A^-1 amplifies most are the smoothest modes, which the coarse levels of both cycles resolve alike: the
difference between two converged solutions is a multiple of 2e-12 set by how ill-conditioned the problem is, and 1e-8 leaves a factor
of 5000 for that amplification.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PREC = 1e-12


@pytest.fixture(scope="module")
def mg():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    import mgroms_amd as m
    m.nhydro.set_verbose(0)
    yield m
    m.nhydro.set_option("cycle_precision", 64)
    m.nhydro_clean()


@pytest.fixture(autouse=True)
def _restore_options(mg):
    """the options this file touches survive nhydro_clean: put them back for the tests that run after it"""
    keep = {k: mg.nhydro.get_option(k) for k in ("cycle_precision", "rb_exact", "rb_seq")}
    yield
    for k, v in keep.items():
        mg.nhydro.set_option(k, v)


def _setup(mg, nx, ny, nz, bmask=False, zeta=None, **par):
    """the seamount problem on the GPU and the CPU oracle's copy of its matrix (bmask: the island mask on both)"""
    from oracle.mgoracle import Oracle, seamount_geometry
    from mgroms_amd.testcases import island_mask
    kw = dict(relax_method="FC", solver_prec=PREC, solver_maxiter=50)
    kw.update(par)
    if bmask:
        kw["bmask"] = 1
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, mg.nhydro.default_params(**kw))
    dx, dy, z0, h = seamount_geometry(nx, ny, 1, 1, 0)
    if zeta is not None:
        z0 = zeta
    rmask = island_mask(nx, ny) if bmask else None
    mg.nhydro_matrices(dx, dy, z0, h, rmask, 4e3, 0.0, 0.0)
    okw = {k: kw[k] for k in ("relax_method", "cmatrix", "interp_type") if k in kw}
    if bmask:
        okw["bmask"] = True
    o = Oracle(nx, ny, nz, 1, 1, **okw)
    for name, a in (("dx", dx), ("dy", dy), ("zeta", z0), ("h", h)):
        o.field(name)[...] = a
    if bmask:
        o.field("rmask")[...] = rmask
    o.matrices(4e3, 0.0, 0.0)
    return o


def _uvw(nx, ny, nz):
    u = np.zeros((nz, ny + 2, nx + 1)); v = np.zeros((nz, ny + 1, nx + 2)); w = -np.ones((nz + 1, ny + 2, nx + 2)); w[0] = 0
    return u, v, w


def _rhs(mg, o, nx, ny, nz):
    u, v, w = _uvw(nx, ny, nz)
    mg.nhydro.compute_rhs(u, v, w)
    if o is not None:
        o.field("w")[...] = w
        o.compute_rhs()


def _solve(mg, prec, maxite=50):
    mg.nhydro.set_option("cycle_precision", prec)
    n, hist = mg.solve_p(PREC, maxite)
    return n, hist, mg.grid(1).p


def _oracle_res(o, p):
    """the oracle's fp64 ||b - A p|| / ||b|| of p"""
    bn = np.sqrt(np.sum(o.field("b")[1:-1, 1:-1, :] ** 2))
    o.field("p")[...] = p
    o.fill_halo(1, "p")
    return o.residual(1) / bn


# ---- operators ------------------------------------------------------------------------------------------------------------
def _close(a, ref, what):
    d = np.abs(a - ref).max()
    m = np.abs(ref).max()
    assert m > 0, what
    assert d <= 1e-5 * m, f"{what}: |diff| {d:.3e} > 1e-5 * {m:.3e}"


def _levels(mg):
    n = mg.nlevs()
    return sorted({1, 2, n} & set(range(1, n + 1)))


def _random(mg, lev, names, rng):
    g = mg.grid(lev)
    vals = {}
    for name in names:
        a = rng.standard_normal(g._shape(name))
        g.set(name, a)
        vals[name] = a
    if "p" in names:
        mg.fill_halo(lev, "p")
        vals["p"] = g.p
    return vals


def _restore(mg, lev, vals):
    g = mg.grid(lev)
    for name, a in vals.items():
        g.set(name, a)


@pytest.mark.parametrize("dims", [(64, 64, 16), (128, 128, 48)])
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_match_fp64(mg, dims, method):
    nx, ny, nz = dims
    _setup(mg, nx, ny, nz, relax_method=method)
    mg.nhydro.set_option("rb_seq", 0)   # the fp32 red-black pass is the parallel one
    rng = np.random.default_rng(7)
    nl = mg.nlevs()
    for lev in _levels(mg):
        # relax: one sweep from the same p, b
        vals = _random(mg, lev, ("p", "b"), rng)
        mg.relax(lev, 1)
        ref = mg.grid(lev).p
        _restore(mg, lev, vals)
        mg.nhydro.mixed_op("relax", lev, 1)
        _close(mg.grid(lev).p, ref, f"relax lev {lev}")
        # residual
        _restore(mg, lev, vals)
        mg.compute_residual(lev)
        ref = mg.grid(lev).r
        _restore(mg, lev, vals)
        mg.nhydro.mixed_op("residual", lev)
        _close(mg.grid(lev).r, ref, f"residual lev {lev}")
        # resrest: the V-cycle's down leg = residual, then fine2coarse
        if lev < nl:
            _restore(mg, lev, vals)
            mg.compute_residual(lev)
            mg.fine2coarse(lev)
            ref = mg.grid(lev + 1).b
            _restore(mg, lev, vals)
            mg.nhydro.mixed_op("resrest", lev)
            _close(mg.grid(lev + 1).b, ref, f"residual + restriction lev {lev}")
            assert np.all(mg.grid(lev + 1).p == 0.0)
    # fine2coarse onto levels 2, 3 and the coarsest
    for lev in sorted({1, 2, nl - 1}):
        r = rng.standard_normal(mg.grid(lev)._shape("r"))
        mg.grid(lev).set("r", r)
        mg.fine2coarse(lev)
        ref = mg.grid(lev + 1).b
        mg.grid(lev + 1).set("b", np.zeros_like(ref))
        mg.grid(lev).set("r", r)
        mg.nhydro.mixed_op("fine2coarse", lev)
        _close(mg.grid(lev + 1).b, ref, f"fine2coarse lev {lev}")
        assert np.all(mg.grid(lev + 1).p == 0.0)


@pytest.mark.parametrize("dims", [(64, 64, 16), (128, 128, 48)])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_coarse2fine_matches_fp64(mg, dims, interp):
    nx, ny, nz = dims
    _setup(mg, nx, ny, nz, interp_type=interp)
    rng = np.random.default_rng(11)
    nl = mg.nlevs()
    for lev in sorted({1, 2, nl - 1}):
        fine = _random(mg, lev, ("p",), rng)
        coarse = _random(mg, lev + 1, ("p",), rng)
        mg.coarse2fine(lev)
        ref = mg.grid(lev).p
        _restore(mg, lev, fine)
        _restore(mg, lev + 1, coarse)
        mg.nhydro.mixed_op("coarse2fine", lev)
        _close(mg.grid(lev).p, ref, f"coarse2fine ({interp}) lev {lev}")


# ---- solves ----------------------------------------------------------------------------------------------------------------
# On the seamount at 256x256x32 (dx = 39 m, dz = 125 m) the reference's cycle contracts by only ~0.75 per iteration, and the fp64
# solver does not reach 1e-12 within the namelist's 50 iterations either: those cases get 400.
CASES = [
    dict(dims=(64, 64, 16), relax_method="FC"),
    dict(dims=(64, 64, 16), relax_method="RB"),
    dict(dims=(128, 128, 32), relax_method="FC"),
    dict(dims=(128, 128, 32), relax_method="RB"),
    dict(dims=(256, 256, 32), relax_method="FC", maxite=400),
    dict(dims=(256, 256, 32), relax_method="RB", maxite=400),
    dict(dims=(64, 64, 48), relax_method="FC"),       # nz = 48 -> 24 -> 12 -> 6 -> 3: an odd coarsest nz
    dict(dims=(64, 64, 48), relax_method="RB"),
    dict(dims=(64, 64, 128), relax_method="FC"),
    dict(dims=(64, 64, 16), relax_method="FC", bmask=True),
    dict(dims=(64, 64, 16), relax_method="RB", bmask=True),
    dict(dims=(64, 64, 16), relax_method="FC", cmatrix="simple"),
    dict(dims=(64, 64, 16), relax_method="RB", cmatrix="simple"),
    dict(dims=(64, 64, 16), relax_method="FC", interp_type="nearest"),
]


def _case_id(c):
    return "-".join([("x".join(map(str, c["dims"])))] + [f"{k}={v}" for k, v in c.items() if k != "dims"])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_mixed_solve(mg, case):
    c = dict(case)
    nx, ny, nz = c.pop("dims")
    maxite = c.pop("maxite", 50)
    o = _setup(mg, nx, ny, nz, **c)
    if nz == 48:
        assert mg.grid(mg.nlevs()).nz == 3
    _rhs(mg, o, nx, ny, nz)
    n64, h64, p64 = _solve(mg, 64, maxite)
    assert h64[-1] <= PREC, (n64, h64)
    it0 = mg.nhydro.get_option("mixed_iterations")
    n32, h32, p32 = _solve(mg, 32, maxite)
    assert h32[-1] <= PREC, (n32, h32)
    assert mg.nhydro.get_option("mixed_iterations") - it0 == n32
    assert n32 <= n64 + 2, (n32, n64, h32, h64)
    ro = _oracle_res(o, p32)
    assert abs(ro - h32[-1]) <= 1e-9 * h32[-1], (ro, h32[-1])
    d = np.abs(p32 - p64).max() / np.abs(p64).max()
    assert d <= 1e-8, d


def test_mixed_is_deterministic(mg):
    nx, ny, nz = 128, 128, 32
    _setup(mg, nx, ny, nz, relax_method="RB")
    _rhs(mg, None, nx, ny, nz)
    n1, h1, p1 = _solve(mg, 32)
    n2, h2, p2 = _solve(mg, 32)
    assert n1 == n2
    assert np.array_equal(h1, h2)
    assert np.array_equal(p1, p2)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_fp64_after_mixed_is_unchanged(mg, method):
    nx, ny, nz = 128, 128, 32
    _setup(mg, nx, ny, nz, relax_method=method)
    _rhs(mg, None, nx, ny, nz)
    n_a, h_a, p_a = _solve(mg, 64)            # fresh fp64 solve
    _setup(mg, nx, ny, nz, relax_method=method)
    _rhs(mg, None, nx, ny, nz)
    _solve(mg, 32)
    _rhs(mg, None, nx, ny, nz)
    n_b, h_b, p_b = _solve(mg, 64)            # fp64 right after a mixed one, same process, same solver
    assert n_a == n_b
    assert np.array_equal(h_a, h_b)
    assert np.array_equal(p_a, p_b)


def test_mixed_follows_new_matrix(mg):
    nx, ny, nz = 64, 64, 16
    o = _setup(mg, nx, ny, nz)
    _rhs(mg, o, nx, ny, nz)
    n, h, p = _solve(mg, 32)
    assert abs(_oracle_res(o, p) - h[-1]) <= 1e-9 * h[-1]
    # nhydro_matrices again with another free surface: the fp32 coefficients must follow
    from oracle.mgoracle import seamount_geometry
    dx, dy, _, hh = seamount_geometry(nx, ny, 1, 1, 0)
    i = np.arange(nx + 2)[:, None]; j = np.arange(ny + 2)[None, :]
    zeta = 5.0 * np.sin(2 * np.pi * i / nx) * np.cos(2 * np.pi * j / ny)
    o2 = _setup(mg, nx, ny, nz, zeta=zeta)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro_matrices(dx, dy, zeta, hh, None, 4e3, 0.0, 0.0)
    _rhs(mg, o2, nx, ny, nz)
    n2, h2, p2 = _solve(mg, 32)
    assert h2[-1] <= PREC
    assert abs(_oracle_res(o2, p2) - h2[-1]) <= 1e-9 * h2[-1]
    # and the same within one solver: solve, change the matrix, solve again
    _setup(mg, nx, ny, nz)
    _rhs(mg, None, nx, ny, nz)
    _solve(mg, 32)
    mg.nhydro_matrices(dx, dy, zeta, hh, None, 4e3, 0.0, 0.0)
    _rhs(mg, o2, nx, ny, nz)
    n3, h3, p3 = _solve(mg, 32)
    assert abs(_oracle_res(o2, p3) - h3[-1]) <= 1e-9 * h3[-1]
    assert np.array_equal(p3, p2)


def test_nhydro_solve_entry_points_go_mixed(mg):
    import torch
    nx, ny, nz = 64, 64, 16
    _setup(mg, nx, ny, nz)
    out = {}
    for prec in (64, 32):
        mg.nhydro.set_option("cycle_precision", prec)
        it0 = mg.nhydro.get_option("mixed_iterations")
        u, v, w = _uvw(nx, ny, nz)
        mg.nhydro_solve(u, v, w)
        host_its = mg.nhydro.get_option("mixed_iterations") - it0
        u2, v2, w2 = (torch.from_numpy(a.copy()).cuda() for a in _uvw(nx, ny, nz))
        mg.nhydro.nhydro_solve_device(u2, v2, w2)
        torch.cuda.synchronize()
        dev_its = mg.nhydro.get_option("mixed_iterations") - it0 - host_its
        out[prec] = (w, w2.cpu().numpy(), host_its, dev_its)
    assert out[64][2] == 0 and out[64][3] == 0
    assert out[32][2] > 0 and out[32][3] > 0
    for k in (0, 1):
        ref = out[64][k]
        assert np.abs(out[32][k] - ref).max() <= 1e-6 * np.abs(ref).max()


def test_operator_entry_points_stay_fp64(mg):
    nx, ny, nz = 64, 64, 16
    _setup(mg, nx, ny, nz)
    rng = np.random.default_rng(3)
    vals = _random(mg, 1, ("p", "b"), rng)
    mg.nhydro.set_option("cycle_precision", 64)
    mg.relax(1, 2); mg.Vcycle(1)
    ref = mg.grid(1).p
    _restore(mg, 1, vals)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.relax(1, 2); mg.Vcycle(1)
    assert np.array_equal(mg.grid(1).p, ref)
    assert mg.nhydro.get_option("mixed_iterations") == 0


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_option_survives_clean_init(mg):
    _setup(mg, 32, 32, 8)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro_clean()
    _setup(mg, 32, 32, 8)
    assert mg.nhydro.get_option("cycle_precision") == 32
    assert mg.nhydro.get_option("mixed_iterations") == 0
    mg.nhydro.set_option("cycle_precision", 64)
    assert mg.nhydro.get_option("cycle_precision") == 64


@pytest.mark.parametrize("value", [0, 1, 16, 33, 63, 128, -32])
def test_other_values_refused(mg, value):
    from mgroms_amd._lib import MgxError
    before = mg.nhydro.get_option("cycle_precision")
    with pytest.raises(MgxError, match="cycle_precision"):
        mg.nhydro.set_option("cycle_precision", value)
    assert mg.nhydro.get_option("cycle_precision") == before


@pytest.mark.parametrize("how", ["GS", "rb_exact"])
def test_unsupported_combinations_refused(mg, how):
    from mgroms_amd._lib import MgxError
    nx, ny, nz = 32, 32, 8
    if how == "GS":
        _setup(mg, nx, ny, nz, relax_method="GS")
    else:
        _setup(mg, nx, ny, nz, relax_method="RB")
        mg.nhydro.set_option("rb_exact", 1)
    _rhs(mg, None, nx, ny, nz)
    mg.nhydro.set_option("cycle_precision", 32)
    with pytest.raises(MgxError, match="cycle_precision"):
        mg.solve_p(PREC, 50)
    with pytest.raises(MgxError, match="cycle_precision"):
        mg.nhydro.mixed_op("relax", 1, 1)
