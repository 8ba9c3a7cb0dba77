"""Mixed-precision solve_p (option "cycle_precision" = 32): fp32 F-cycles in correction form under the fp64 refinement loop.

Operators: every fp32 kernel of the cycle, through mgx_mixed_op, against the fp64 operator of the same name on the same input
(levels 1, 2 and the coarsest; |diff|_inf <= 1e-5 of the fp64 result's max: a few fp32 roundings of every term), and on every level of
seven shapes with the same bound in each region, the fp32 mirror images and coarse zeros exact, the conversions exact.
Cycle: the first mixed iterations against fp64 ones from the same start (refinement would hide a wrong but contracting cycle).
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

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, oracle_relative_residual, oracle_twin, regions, rhs, uvw

pytestmark = pytest.mark.gpu
mg = gpu_module(cycle_precision=64)

PREC = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _worst_table(mg):
    """what the operator tests measured, printed once at the end of the file"""
    yield
    if _WORST:
        print("\nworst |fp32 - fp64| / max|fp64| (operators: per region):")
        for (op, region), v in sorted(_WORST.items()):
            print(f"  {op:28s} {region:9s} {v:.2e}")


_restore_options = restore_options("cycle_precision", "rb_exact", "rb_seq", "warm_start")


def _setup(mg, nx, ny, nz, oracle=True, **kw):
    """the seamount problem on the GPU and the CPU oracle's copy of its matrix (bmask: the island mask on both; sigma: (hc, theta_b,
    theta_s), stretched coordinates; oracle=False: the GPU side only, returns None).  The oracle here only ever recomputes a level-1
    residual, never a cycle: it takes the members that shape the matrix and keeps its defaults for the rest."""
    pr = gpu_problem(mg, (nx, ny, nz), **dict(dict(relax_method="FC", solver_prec=PREC, solver_maxiter=50), **kw))
    return oracle_twin(pr, only=("relax_method", "cmatrix", "interp_type", "bmask")) if oracle else None


def _solve(mg, prec, maxite=50):
    mg.nhydro.set_option("cycle_precision", prec)
    n, hist = mg.solve_p(PREC, maxite)
    return n, hist, mg.grid(1).p


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
    _operators_match_fp64(mg, dims, method)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_match_fp64_on_a_curvilinear_metric(mg, method):
    """the same comparison on dx(i,j), dy(i,j) (testcases.curvilinear_metric): the fp32 kernels fetch their 2-D metric factors by the
    index arithmetic of the fp64 ones, and a factor taken one column off moves the result by the metric's variation (per cent), far
    above 1e-5"""
    _operators_match_fp64(mg, (64, 64, 16), method, metric="curvilinear")
    dx, dy = mg.grid(1).get("dx"), mg.grid(1).get("dy")
    assert np.ptp(dx, axis=0).min() > 0 and np.ptp(dx, axis=1).min() > 0 and np.ptp(dy, axis=0).min() > 0 and np.ptp(dy, axis=1).min() > 0


def _operators_match_fp64(mg, dims, method, **kw):
    nx, ny, nz = dims
    _setup(mg, nx, ny, nz, relax_method=method, **kw)
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


# ---- every level: region-wise bounds, exact mirrors, exact zeros, exact conversions ------------------------------------------
# The bound of _close is 1e-5 of the global max of the result: a wrong value confined to the mirror cells or to the k = 1 or k = nz
# row can hide under it.  _check keeps that bound and applies the same one to each region on its own (interior rows, k = 1, k = nz,
# halo cells), and requires every physical-boundary image of the fp32 result to equal its interior source bit for bit (the fp32
# kernels store the images as plain copies).  The worst ratios met are kept in _WORST and printed when the module ends (pytest -s).
_WORST = {}


def _note(op, region, ratio):
    _WORST[(op, region)] = max(_WORST.get((op, region), 0.0), ratio)


def _mirrored(a, what):
    """every physical-boundary image of a (edges and corners, all four sides: a single rank) equals its interior source bit for bit"""
    want = np.pad(a[1:-1, 1:-1], ((1, 1), (1, 1), (0, 0)), mode="edge")
    bad = np.argwhere(a != want)
    assert bad.size == 0, f"{what}: {len(bad)} halo cells differ from their interior source, first (i, j, k) {bad[:4].tolist()}"


def _check(a, ref, op, what):
    _close(a, ref, what)
    ra = regions(a)
    for name, r in regions(ref).items():
        m = np.abs(r).max()
        assert m > 0, f"{what}, {name}: the fp64 result is zero there"
        d = np.abs(ra[name] - r).max()
        _note(op, name, d / m)
        assert d <= 1e-5 * m, f"{what}, {name}: |diff| {d:.3e} > 1e-5 * {m:.3e}"
    _mirrored(a, what)


def _coarse_loaded(mg, lev, rng):
    """random values in the fp32 e and f of level lev (relax x0 converts p and b in), so that zeros the next operator owes are visible"""
    _random(mg, lev, ("p", "b"), rng)
    mg.nhydro.mixed_op("relax", lev, 0)


def _c2f(mg, lev, rng, tag):
    fine = _random(mg, lev, ("p",), rng)
    coarse = _random(mg, lev + 1, ("p",), rng)
    mg.coarse2fine(lev)
    ref = mg.grid(lev).p
    _restore(mg, lev, fine)
    _restore(mg, lev + 1, coarse)
    mg.nhydro.mixed_op("coarse2fine", lev)
    _check(mg.grid(lev).p, ref, "coarse2fine", f"{tag}: coarse2fine")


def _op_matrix(mg, levels, rng, what):
    """every fp32 operator of the cycle on each of `levels` against the fp64 operator of the same name on the same input: relax with
    1 and ns_pre sweeps (and ns_coarsest on the coarsest level), residual, and from each level to the next coarser one residual +
    restriction, restriction and coarse2fine (the set-up's interp_type)"""
    nl = mg.nlevs()
    ns = {mg.nhydro.get_option("ns_pre"), 1}
    for lev in levels:
        tag = f"{what} lev {lev}/{nl} ({mg.grid(lev).nx}x{mg.grid(lev).ny}x{mg.grid(lev).nz})"
        vals = _random(mg, lev, ("p", "b"), rng)
        for n in sorted(ns | ({mg.nhydro.get_option("ns_coarsest")} if lev == nl else set())):
            _restore(mg, lev, vals)
            mg.relax(lev, n)
            ref = mg.grid(lev).p
            _restore(mg, lev, vals)
            mg.nhydro.mixed_op("relax", lev, n)
            _check(mg.grid(lev).p, ref, f"relax x{n}" if n < 10 else "relax x ns_coarsest", f"{tag}: relax x{n}")
        _restore(mg, lev, vals)
        mg.compute_residual(lev)
        ref = mg.grid(lev).r
        _restore(mg, lev, vals)
        mg.nhydro.mixed_op("residual", lev)
        _check(mg.grid(lev).r, ref, "residual", f"{tag}: residual")
        if lev == nl:
            continue
        # residual + restriction (the V-cycle's down leg): coarse b, and a coarse p of exact zeros
        _restore(mg, lev, vals)
        mg.compute_residual(lev)
        mg.fine2coarse(lev)
        ref = mg.grid(lev + 1).b
        _coarse_loaded(mg, lev + 1, rng)
        _restore(mg, lev, vals)
        mg.nhydro.mixed_op("resrest", lev)
        _check(mg.grid(lev + 1).b, ref, "resrest", f"{tag}: residual + restriction")
        assert np.all(mg.grid(lev + 1).p == 0.0), f"{tag}: residual + restriction left a non-zero coarse p"
        # restriction (the F-cycle's first leg)
        r = rng.standard_normal(mg.grid(lev)._shape("r"))
        mg.grid(lev).set("r", r)
        mg.fine2coarse(lev)
        ref = mg.grid(lev + 1).b
        _coarse_loaded(mg, lev + 1, rng)
        mg.grid(lev).set("r", r)
        mg.nhydro.mixed_op("fine2coarse", lev)
        _check(mg.grid(lev + 1).b, ref, "fine2coarse", f"{tag}: restriction")
        assert np.all(mg.grid(lev + 1).p == 0.0), f"{tag}: restriction left a non-zero coarse p"
        _c2f(mg, lev, rng, tag)


# level 1 nz -> coarsest: 16 -> 2 (register instances 16, 8, 4, 2); 32 (instance 32); 64 (instance 64, nx != ny); 128 -> 8 (generic pass at
# 128); 96 -> 12 (generic 96, 48, 24, 12; ny/2 = 16 -> 2); 96x48 (half-rows of 24, 12, 6, 3: not a multiple of 32, odd on the coarsest);
# 40 -> 5 (generic 40, 20, 10, 5: an odd coarsest nz)
LEVEL_SHAPES = [(64, 64, 16), (128, 128, 32), (256, 128, 64), (64, 64, 128), (64, 32, 96), (96, 48, 16), (32, 32, 40)]


def _dims_id(d):
    return "x".join(map(str, d))


@pytest.mark.parametrize("dims", LEVEL_SHAPES, ids=_dims_id)
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_every_level(mg, dims, method):
    """Every fp32 operator on every level against fp64 (red-black: the rb_seq = 0 pass), region by region, mirrors exact.

    Worst |fp32 - fp64| / max|fp64| of a region over this test, the variants, the user matrix, the bench size and coarse2fine
    nearest (MI355X; regions interior / k = 1 / k = nz / halo; bound 1e-5):
      relax x1             2.3e-7 / 2.2e-7 / 1.9e-7 / 2.5e-7     residual     1.8e-7 / 1.5e-7 / 1.7e-7 / 1.5e-7
      relax x3 (ns_pre)    4.0e-7 / 4.2e-7 / 4.5e-7 / 3.6e-7     resrest      2.7e-7 / 2.5e-7 / 2.1e-7 / 2.3e-7
      relax x40 coarsest   2.1e-7 / 1.3e-6 / 1.0e-6 / 1.3e-6     fine2coarse  1.3e-7 / 1.2e-7 / 1.2e-7 / 1.4e-7
      coarse2fine          1.4e-7 / 1.1e-7 / 9.1e-8 / 1.4e-7
    """
    _setup(mg, *dims, relax_method=method, oracle=False)
    mg.nhydro.set_option("rb_seq", 0)
    _op_matrix(mg, range(1, mg.nlevs() + 1), np.random.default_rng(17), f"{method} {_dims_id(dims)}")


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_bench_size(mg, method):
    """levels 1 and 2 of 512x512x64: the instances k_relax32<64> and <32> at the benchmark's size"""
    _setup(mg, 512, 512, 64, relax_method=method, oracle=False)
    mg.nhydro.set_option("rb_seq", 0)
    _op_matrix(mg, (1, 2), np.random.default_rng(19), f"{method} 512x512x64")


@pytest.mark.parametrize("dims", LEVEL_SHAPES, ids=_dims_id)
def test_coarse2fine_nearest_every_level(mg, dims):
    _setup(mg, *dims, interp_type="nearest", oracle=False)
    rng = np.random.default_rng(23)
    for lev in range(1, mg.nlevs()):
        _c2f(mg, lev, rng, f"nearest {_dims_id(dims)} lev {lev}")


VARIANTS = {"bmask": dict(bmask=True), "simple": dict(cmatrix="simple"), "stretched": dict(sigma=(250.0, 0.4, 6.0))}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_every_level_variants(mg, variant, method):
    """the island mask, cmatrix = 'simple' (no k = 1 diagonal terms) and stretched sigma coordinates (theta_s, theta_b != 0)"""
    _setup(mg, 64, 64, 16, relax_method=method, oracle=False, **VARIANTS[variant])
    mg.nhydro.set_option("rb_seq", 0)
    _op_matrix(mg, range(1, mg.nlevs() + 1), np.random.default_rng(29), f"{method} {variant}")


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operators_follow_user_matrix(mg, method):
    """a matrix given through grid(lev).set("cA", ...) after the shadow was converted: each level's cA scaled by a factor that is not a
    power of two, so a shadow that was not converted again gives results off by that factor"""
    _setup(mg, 64, 64, 16, relax_method=method, oracle=False)
    mg.nhydro.set_option("rb_seq", 0)
    rng = np.random.default_rng(31)
    _random(mg, 1, ("p", "b"), rng)
    mg.nhydro.mixed_op("residual", 1)   # the shadow now holds the seamount matrix
    for lev in range(1, mg.nlevs() + 1):
        g = mg.grid(lev)
        g.set("cA", g.cA * (1.1 + 0.2 * lev))
    _op_matrix(mg, range(1, mg.nlevs() + 1), rng, f"{method} user cA")


@pytest.mark.parametrize("dims", [(96, 48, 16), (256, 128, 64)], ids=_dims_id)
def test_conversions_exact(mg, dims):
    """relax with 0 sweeps is the fp64 -> fp32 -> fp64 round trip of p (k_to32, k_to64): every cell, halo included, rounds to nearest
    fp32 bit for bit (both signs, exact zeros, magnitudes 1e-6 .. 1e6; the halo holds values of its own, not images)"""
    _setup(mg, *dims, oracle=False)
    rng = np.random.default_rng(37)
    for lev in range(1, mg.nlevs() + 1):
        g = mg.grid(lev)
        sh = g._shape("p")
        a = rng.choice([-1.0, 1.0], sh) * 10.0 ** rng.uniform(-6.0, 6.0, sh)
        a[rng.random(sh) < 0.05] = 0.0
        g.set("p", a)
        want = a.astype(np.float32).astype(np.float64)
        assert not np.array_equal(want, a)
        mg.nhydro.mixed_op("relax", lev, 0)
        got = g.p
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"lev {lev}: {len(bad)} cells not the fp32 rounding of their input, first (i, j, k) {bad[:4].tolist()}"


# ---- the mixed cycle against the fp64 cycle, iteration by iteration -------------------------------------------------------------
# From p = 0 one fp64 iteration gives p = Fcycle(b), one mixed iteration ||b|| Fcycle32(b / ||b||): the cycle is linear in b, so the
# two agree to fp32 rounding -- which iterative refinement would otherwise hide (test_mixed_solve passes with any cycle that contracts).
def _case_id(c):
    val = lambda v: "/".join(map(str, v)) if isinstance(v, tuple) else v
    return "-".join([("x".join(map(str, c["dims"])))] + [f"{k}={val(v)}" for k, v in c.items() if k != "dims"])


CYCLE_CASES = [
    dict(dims=(64, 64, 16)),
    dict(dims=(96, 48, 16)),
    dict(dims=(64, 64, 48)),              # coarsest nz = 3
    dict(dims=(64, 64, 128)),
    dict(dims=(64, 64, 16), bmask=True),
    dict(dims=(64, 64, 16), cmatrix="simple"),
    dict(dims=(64, 64, 16), interp_type="nearest"),
    dict(dims=(64, 64, 16), sigma=(250.0, 0.4, 6.0)),
    dict(dims=(64, 64, 16), ns_pre=1, ns_post=3, ns_coarsest=10),
    dict(dims=(64, 64, 16), ns_pre=2, ns_post=1, ns_coarsest=20),
]


@pytest.mark.parametrize("case", CYCLE_CASES, ids=_case_id)
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_mixed_cycle_matches_fp64(mg, case, method):
    """first iterations of solve_p in both precisions from p = 0 (red-black fp64: rb_seq = 0, the pass the fp32 cycle runs):
    p after one iteration within 1e-5 of max|p|; the residual history of three iterations within 1e-4 of h64[k] plus 1e-4 of h64[k-1].

    The second term: iteration k hands the cycle r / ||r|| with ||r|| = h[k-1] ||b||, so the fp32 rounding in its correction is a
    fraction of h[k-1], not of h[k], and what it leaves in the residual decays no faster than the residual itself.  Where the first
    iteration contracts by 5e-4 (64x64x128) that is up to 1e-2 of h[1] and 1e-3 of h[3], while p agrees within 3.5e-6: 1e-4 of
    h64[k] alone holds only where the cycle contracts slowly (6-7 digits at 512x512x64).
    Worst measured (MI355X): p after one iteration 3.5e-6 of max|p|; |h32[k] - h64[k]| 3.4e-5 of h64[k-1] (64x64x128 RB, k = 3).
    """
    c = dict(case)
    dims = c.pop("dims")
    _setup(mg, *dims, relax_method=method, oracle=False, **c)
    mg.nhydro.set_option("rb_seq", 0)
    rhs(mg, None, uvw(dims))
    out = {}
    for prec in (64, 32):
        n1, _, p1 = _solve(mg, prec, 1)
        n3, h3, _ = _solve(mg, prec, 3)
        assert (n1, n3) == (1, 3), (prec, n1, n3)
        out[prec] = (p1, h3)
    (p64, h64), (p32, h32) = out[64], out[32]
    d = np.abs(p32 - p64).max() / np.abs(p64).max()
    _note("cycle: p after 1", "", d)
    assert d <= 1e-5, f"p after one iteration: |diff| {d:.3e} of max|p|"
    d = np.abs(h32[1:] - h64[1:])
    _note("cycle: history 1..3", "of h64[k-1]", (d / h64[:-1]).max())
    assert np.all(d <= 1e-4 * (h64[1:] + h64[:-1])), (h32, h64)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_mixed_cycle_warm_start(mg, method):
    """warm_start = 1 from the p0 of two fp64 iterations: one more iteration in either precision gives the same correction p1 - p0
    (within 1e-5 of its max; measured 1.1e-6 on the MI355X)"""
    nx, ny, nz = 64, 64, 16
    _setup(mg, nx, ny, nz, relax_method=method, oracle=False)
    mg.nhydro.set_option("rb_seq", 0)
    rhs(mg, None, uvw((nx, ny, nz)))
    _, _, p0 = _solve(mg, 64, 2)
    mg.nhydro.set_option("warm_start", 1)
    dp = {}
    for prec in (64, 32):
        mg.grid(1).set("p", p0)
        n, _, p1 = _solve(mg, prec, 1)
        assert n == 1
        dp[prec] = p1 - p0
    m = np.abs(dp[64]).max()
    assert m > 0
    d = np.abs(dp[32] - dp[64]).max() / m
    _note("cycle: warm-start correction", "", d)
    assert d <= 1e-5, f"correction p1 - p0: |diff| {d:.3e} of its max"


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


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_mixed_solve(mg, case):
    c = dict(case)
    nx, ny, nz = c.pop("dims")
    maxite = c.pop("maxite", 50)
    o = _setup(mg, nx, ny, nz, **c)
    if nz == 48:
        assert mg.grid(mg.nlevs()).nz == 3
    rhs(mg, o, uvw((nx, ny, nz)))
    n64, h64, p64 = _solve(mg, 64, maxite)
    assert h64[-1] <= PREC, (n64, h64)
    it0 = mg.nhydro.get_option("mixed_iterations")
    n32, h32, p32 = _solve(mg, 32, maxite)
    assert h32[-1] <= PREC, (n32, h32)
    assert mg.nhydro.get_option("mixed_iterations") - it0 == n32
    assert n32 <= n64 + 2, (n32, n64, h32, h64)
    ro = oracle_relative_residual(o, p32)
    assert abs(ro - h32[-1]) <= 1e-9 * h32[-1], (ro, h32[-1])
    d = np.abs(p32 - p64).max() / np.abs(p64).max()
    assert d <= 1e-8, d


def test_mixed_is_deterministic(mg):
    nx, ny, nz = 128, 128, 32
    _setup(mg, nx, ny, nz, relax_method="RB")
    rhs(mg, None, uvw((nx, ny, nz)))
    n1, h1, p1 = _solve(mg, 32)
    n2, h2, p2 = _solve(mg, 32)
    assert n1 == n2
    assert np.array_equal(h1, h2)
    assert np.array_equal(p1, p2)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_fp64_after_mixed_is_unchanged(mg, method):
    nx, ny, nz = 128, 128, 32
    _setup(mg, nx, ny, nz, relax_method=method)
    rhs(mg, None, uvw((nx, ny, nz)))
    n_a, h_a, p_a = _solve(mg, 64)            # fresh fp64 solve
    _setup(mg, nx, ny, nz, relax_method=method)
    rhs(mg, None, uvw((nx, ny, nz)))
    _solve(mg, 32)
    rhs(mg, None, uvw((nx, ny, nz)))
    n_b, h_b, p_b = _solve(mg, 64)            # fp64 right after a mixed one, same process, same solver
    assert n_a == n_b
    assert np.array_equal(h_a, h_b)
    assert np.array_equal(p_a, p_b)


def test_mixed_follows_new_matrix(mg):
    nx, ny, nz = 64, 64, 16
    o = _setup(mg, nx, ny, nz)
    rhs(mg, o, uvw((nx, ny, nz)))
    n, h, p = _solve(mg, 32)
    assert abs(oracle_relative_residual(o, p) - h[-1]) <= 1e-9 * h[-1]
    # nhydro_matrices again with another free surface: the fp32 coefficients must follow
    from mgroms_amd.testcases import seamount_geometry
    dx, dy, _, hh = seamount_geometry(nx, ny, 1, 1, 0)
    i = np.arange(nx + 2)[:, None]; j = np.arange(ny + 2)[None, :]
    zeta = 5.0 * np.sin(2 * np.pi * i / nx) * np.cos(2 * np.pi * j / ny)
    o2 = _setup(mg, nx, ny, nz, zeta=zeta)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro_matrices(dx, dy, zeta, hh, None, 4e3, 0.0, 0.0)
    rhs(mg, o2, uvw((nx, ny, nz)))
    n2, h2, p2 = _solve(mg, 32)
    assert h2[-1] <= PREC
    assert abs(oracle_relative_residual(o2, p2) - h2[-1]) <= 1e-9 * h2[-1]
    # and the same within one solver: solve, change the matrix, solve again
    _setup(mg, nx, ny, nz)
    rhs(mg, None, uvw((nx, ny, nz)))
    _solve(mg, 32)
    mg.nhydro_matrices(dx, dy, zeta, hh, None, 4e3, 0.0, 0.0)
    rhs(mg, o2, uvw((nx, ny, nz)))
    n3, h3, p3 = _solve(mg, 32)
    assert abs(oracle_relative_residual(o2, p3) - h3[-1]) <= 1e-9 * h3[-1]
    assert np.array_equal(p3, p2)


def test_nhydro_solve_entry_points_go_mixed(mg):
    import torch
    nx, ny, nz = 64, 64, 16
    _setup(mg, nx, ny, nz)
    out = {}
    for prec in (64, 32):
        mg.nhydro.set_option("cycle_precision", prec)
        it0 = mg.nhydro.get_option("mixed_iterations")
        u, v, w = uvw((nx, ny, nz))
        mg.nhydro_solve(u, v, w)
        host_its = mg.nhydro.get_option("mixed_iterations") - it0
        u2, v2, w2 = (torch.from_numpy(a.copy()).cuda() for a in uvw((nx, ny, nz)))
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
    rhs(mg, None, uvw((nx, ny, nz)))
    mg.nhydro.set_option("cycle_precision", 32)
    with pytest.raises(MgxError, match="cycle_precision"):
        mg.solve_p(PREC, 50)
    with pytest.raises(MgxError, match="cycle_precision"):
        mg.nhydro.mixed_op("relax", 1, 1)
