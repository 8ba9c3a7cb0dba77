"""Option "mixed_direct": the coarsest solve of an fp32 cycle as one matrix-vector product (k_coarse_direct32 and the direct phase of k_tail32,
mgx_mixed.hip) with the fp64 operator rounded once to fp32.

(a) mixed_op("coarsest", nlevs) with the option on against the fp64 relax(nlevs, ns_coarsest) from p = 0 (rb_seq = 0: the parallel colour
    order the operator is built in) on the same random b: within 1e-5 of max|fp64| in each region of the level -- the bound
    tests/test_gpu_mixed_precision.py puts on every fp32 kernel -- every physical-boundary image equal to its interior value bit for bit,
    and "mixed_direct_solves" grows by one.  n = 32 (less than a wave), 128, 480 (ragged), 64 (nz = 4), 2048 (the largest), 48 (nz = 3
    under small_any_nz); 'simple', the island mask and stretched sigma at n = 2048.
    The bound was checked on the CPU with the oracle's four-colour sweeps, the operator built from the unit vectors and rounded to fp32 and
    the product accumulated sequentially in fp32 without fused multiply-adds (worse than the kernel's slabs of fmaf): at n = 2048 the worst
    region over five draws was 2.1e-6 (plain), 2.7e-6 (bmask), 2.4e-6 (stretched sigma), at n = 128 and 64 5e-7.  The kernel's largest
    ratio on an MI355X: 9.2e-7 (n = 2048, red-black, stretched sigma).
(b) a declined level keeps the sweeps and their bits, and so does a rough state (mixed_op "vcycle" at the coarsest level, "relax").
(c) V-cycles from a random state: mixed_tail = 0 and 1 the same bits under the option, in both register classes of the tail kernel.
(d) launch counts.  (e) solves: the assertions of tests/test_gpu_mixed_ring.py::test_mixed_solve, and the Krylov loop over the fp32 cycle.
(f) the operator follows the matrix and option "small_any_nz".  (g) the fp64 direct solve of "coarsest_direct" is not disturbed."""
import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, oracle_relative_residual, oracle_twin, regions, rhs, uvw

pytestmark = pytest.mark.gpu

OPTIONS = ("mixed_direct", "mixed_ring", "mixed_tail", "cycle_precision", "krylov", "krylov_precision", "rb_seq", "warm_start", "small_any_nz",
           "coarsest_direct")
METHODS = {"FC": dict(relax_method="FC"), "RB": dict(relax_method="RB"), "FC-simple": dict(relax_method="FC", cmatrix="simple"),
           "RB-simple": dict(relax_method="RB", cmatrix="simple")}
PREC = 1e-12

mg = gpu_module(mixed_direct=0)
_restore_options = restore_options(*OPTIONS)


def _setup(mg, dims, method="FC", any_nz=0, **kw):
    pr = gpu_problem(mg, dims, **dict(METHODS[method], solver_prec=PREC, solver_maxiter=50, **kw))
    mg.nhydro.set_option("rb_seq", 0)
    for k in ("krylov", "warm_start", "mixed_tail", "mixed_ring", "mixed_direct"):
        mg.nhydro.set_option(k, 0)
    mg.nhydro.set_option("small_any_nz", any_nz)
    mg.nhydro.set_option("cycle_precision", 64)
    return pr


def _id(d):
    return "x".join(map(str, d))


def _solves(mg):
    return mg.nhydro.get_option("mixed_direct_solves")


def _coarsest(mg, b, direct):
    """p after mixed_op("coarsest") on b, and the growth of the counter"""
    nl = mg.nlevs()
    mg.nhydro.set_option("mixed_direct", direct)
    g = mg.grid(nl)
    g.set("p", np.full(g._shape("p"), 7.0))   # the hook starts from e = 0 whatever p holds
    g.set("b", b)
    c0 = _solves(mg)
    mg.nhydro.mixed_op("coarsest", nl, 0)
    return mg.grid(nl).p, _solves(mg) - c0


def _fp64_solve(mg, b):
    """the fp64 relax(nlevs, ns_coarsest) from p = 0"""
    nl = mg.nlevs()
    g = mg.grid(nl)
    g.set("p", np.zeros(g._shape("p")))
    g.set("b", b)
    mg.relax(nl, mg.nhydro.get_option("ns_coarsest"))
    return mg.grid(nl).p


def _mirrored(a, what):
    want = np.pad(a[1:-1, 1:-1], ((1, 1), (1, 1), (0, 0)), mode="edge")
    bad = np.argwhere(a != want)
    assert bad.size == 0, f"{what}: {len(bad)} halo cells differ from their interior source, first (i, j, k) {bad[:4].tolist()}"


def _close_fp64(a, ref, what):
    ra = regions(a)
    for name, r in regions(ref).items():
        m = np.abs(r).max()
        assert m > 0, f"{what}, {name}: the fp64 result is zero there"
        d = np.abs(ra[name] - r).max()
        print(f"  {what}, {name}: |fp32 - fp64| / max|fp64| = {d / m:.2e}")
        assert d <= 1e-5 * m, f"{what}, {name}: |fp32 - fp64| {d:.3e} > 1e-5 * {m:.3e}"


def _check_product(mg, dims, any_nz, what, seed=61):
    nl = mg.nlevs()
    t = mg.nhydro.level_table(*dims)[-1]
    n = t["nx"] * t["ny"] * t["nz"]
    assert nl >= 2 and mg.nhydro.mixed_direct_cells(*dims, small_any_nz=any_nz) == n, (dims, nl, n)
    b = np.random.default_rng(seed).standard_normal(mg.grid(nl)._shape("b"))
    p32, grew = _coarsest(mg, b, 1)
    assert grew == 1, (what, grew)
    _close_fp64(p32, _fp64_solve(mg, b), what)
    _mirrored(p32, what)
    return b, p32


# ---- (a) the product against the fp64 solve ---------------------------------------------------------------------------------------------
# dims, small_any_nz, n of the coarsest level
SHAPES = [((16, 16, 8), 0, 32), ((16, 16, 4), 0, 128), ((24, 40, 4), 0, 480), ((16, 16, 16), 0, 64), ((64, 64, 4), 0, 2048), ((32, 32, 24), 1, 48)]


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("dims,any_nz,n", SHAPES, ids=[f"{_id(d)}-n{n}" for d, _, n in SHAPES])
def test_product_matches_fp64_solve(mg, dims, any_nz, n, method):
    _setup(mg, dims, method, any_nz)
    assert mg.nhydro.mixed_direct_cells(*dims, small_any_nz=any_nz) == n
    _check_product(mg, dims, any_nz, f"{_id(dims)} {method} n={n}")


@pytest.mark.parametrize("method", ["FC-simple", "RB-simple"])
def test_simple_matrix(mg, method):
    _setup(mg, (64, 64, 4), method)
    _check_product(mg, (64, 64, 4), 0, f"64x64x4 {method}")


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("variant", ["bmask", "stretched"])
def test_variants(mg, variant, method):
    """the island mask (coefficients that vanish on land) and stretched sigma coordinates at 64x64x4 (n = 2048)"""
    _setup(mg, (64, 64, 4), method, **(dict(bmask=True) if variant == "bmask" else dict(sigma=(250.0, 0.4, 6.0))))
    _check_product(mg, (64, 64, 4), 0, f"64x64x4 {method} {variant}")


# ---- (b) declined levels keep their bits ------------------------------------------------------------------------------------------------
DECLINED = [((128, 64, 4), 0), ((32, 32, 24), 0)]   # 64x32x2 = 4096 cells; 4x4x3 without small_any_nz


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("dims,any_nz", DECLINED, ids=[_id(d) for d, _ in DECLINED])
def test_declined_levels_keep_their_bits(mg, dims, any_nz, method):
    _setup(mg, dims, method, any_nz)
    assert mg.nhydro.mixed_direct_cells(*dims, small_any_nz=any_nz) == 0
    nl = mg.nlevs()
    b = np.random.default_rng(63).standard_normal(mg.grid(nl)._shape("b"))
    p0, c0 = _coarsest(mg, b, 0)
    p1, c1 = _coarsest(mg, b, 1)
    assert c0 == 0 and c1 == 0, (c0, c1)
    assert np.array_equal(p0, p1), f"{int((p0 != p1).sum())} cells differ"
    assert np.isfinite(p1).all() and np.abs(p1).max() > 0


ROUGH = [((16, 16, 4), 0), ((128, 64, 4), 0)]   # a served level and a declined one


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("dims,any_nz", ROUGH, ids=[_id(d) for d, _ in ROUGH])
def test_rough_state_keeps_the_sweeps(mg, dims, any_nz, tail, method):
    """mixed_op("vcycle", nlevs) and mixed_op("relax", nlevs, n) relax the e they find: the option changes no bit, the counter stands"""
    _setup(mg, dims, method, any_nz)
    mg.nhydro.set_option("mixed_tail", tail)
    nl = mg.nlevs()
    rng = np.random.default_rng(65)
    g = mg.grid(nl)
    p, b = rng.standard_normal(g._shape("p")), rng.standard_normal(g._shape("b"))
    for op, n in (("vcycle", 0), ("relax", 1), ("relax", 3)):
        out = []
        for direct in (0, 1):
            mg.nhydro.set_option("mixed_direct", direct)
            g.set("p", p); g.set("b", b); mg.fill_halo(nl, "p")
            c0 = _solves(mg)
            mg.nhydro.mixed_op(op, nl, n)
            assert _solves(mg) == c0, (op, n, direct)
            out.append(mg.grid(nl).p)
        assert np.array_equal(out[0], out[1]), f"{op} x{n}: {int((out[0] != out[1]).sum())} cells differ"
        assert np.isfinite(out[1]).all() and not np.array_equal(out[1], p)


# ---- (c) cycles ---------------------------------------------------------------------------------------------------------------------------
def _random_levels(mg, rng):
    state = {}
    for lev in range(1, mg.nlevs() + 1):
        g = mg.grid(lev)
        g.set("p", rng.standard_normal(g._shape("p")))
        g.set("b", rng.standard_normal(g._shape("b")))
        mg.fill_halo(lev, "p")
        state[lev] = (g.p, g.b)
    return state


# 64x64x16: the tail starts at level 2 (32x32x8), 768 lanes; 64x64x32: at 32x32x16, the 256-lane class
CYCLES = [((64, 64, 16), 0), ((64, 64, 32), 0), ((64, 64, 32), 1)]


@pytest.mark.parametrize("method", ["FC", "RB", "FC-simple", "RB-simple"])
@pytest.mark.parametrize("dims,ring", CYCLES, ids=[f"{_id(d)}-ring{r}" for d, r in CYCLES])
def test_vcycles_tail_on_and_off_same_bits(mg, dims, ring, method):
    _setup(mg, dims, method)
    assert mg.nhydro.mixed_tail_first(*dims) == 2 and mg.nhydro.mixed_direct_cells(*dims) > 0
    state = _random_levels(mg, np.random.default_rng(67))
    mg.nhydro.set_option("mixed_direct", 1)
    mg.nhydro.set_option("mixed_ring", ring)
    out = []
    for tail in (0, 1):
        mg.nhydro.set_option("mixed_tail", tail)
        for lev, s in state.items():
            g = mg.grid(lev)
            g.set("p", s[0]); g.set("b", s[1])
        c0, t0 = _solves(mg), mg.nhydro.get_option("mixed_tail_launches")
        mg.nhydro.mixed_op("vcycle", 1, 0)
        grew = _solves(mg) - c0, mg.nhydro.get_option("mixed_tail_launches") - t0
        assert grew[0] == 1 and (grew[1] > 0) == (tail == 1), (tail, grew)
        out.append({lev: mg.grid(lev).p for lev in state})
    for lev in state:
        assert np.array_equal(out[0][lev], out[1][lev]), f"{method}: level {lev}: {int((out[0][lev] != out[1][lev]).sum())} cells of p differ"
        assert np.isfinite(out[1][lev]).all()
        assert not np.array_equal(out[1][lev], state[lev][0])


# ---- (d) launch counts ------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mg):
    """64x64x16, four colours, cycle_precision = 32, three iterations of the second solve (the operator is built by the first)"""
    dims, ite = (64, 64, 16), 3
    _setup(mg, dims, "FC")
    rhs(mg, None, uvw(dims))
    mg.nhydro.set_option("cycle_precision", 32)
    nl, ns = mg.nlevs(), mg.nhydro.get_option("ns_coarsest")
    got = {}
    for tail in (0, 1):
        for direct in (0, 1):
            mg.nhydro.set_option("mixed_tail", tail)
            mg.nhydro.set_option("mixed_direct", direct)
            mg.solve_p(1e-300, 1)
            c0, s0 = mg.nhydro.counters()["launches"], _solves(mg)
            n, _ = mg.solve_p(1e-300, ite)
            assert n == ite
            got[tail, direct] = (mg.nhydro.counters()["launches"] - c0, _solves(mg) - s0)
    print(f"\nlaunches and served solves of {ite} iterations, (mixed_tail, mixed_direct): {got}")
    assert got[0, 0][1] == 0 and got[1, 0][1] == 0, got
    assert got[0, 1][1] == nl * ite and got[1, 1][1] == nl * ite, got
    assert got[0, 0][0] - got[0, 1][0] == ite * nl * (4 * ns - 1), got
    assert got[1, 0][0] == got[1, 1][0], got


# ---- (e) solves -------------------------------------------------------------------------------------------------------------------------
SOLVES = [((64, 64, 32), "FC"), ((64, 64, 32), "RB"), ((32, 32, 48), "FC")]


@pytest.mark.parametrize("dims,method", SOLVES, ids=[f"{_id(d)}-{m}" for d, m in SOLVES])
def test_mixed_solve(mg, dims, method):
    """cold start to 1e-12 with cycle_precision = 32 and the option on: what tests/test_gpu_mixed_ring.py::test_mixed_solve asserts"""
    pr = _setup(mg, dims, method)
    o = oracle_twin(pr, only=("relax_method", "cmatrix", "interp_type", "bmask"))
    rhs(mg, o, uvw(dims))
    n64, h64 = mg.solve_p(PREC, 50)
    p64 = mg.grid(1).p
    assert h64[-1] <= PREC, (n64, h64)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro.set_option("mixed_direct", 1)
    it0, s0 = mg.nhydro.get_option("mixed_iterations"), _solves(mg)
    n32, h32 = mg.solve_p(PREC, 50)
    p32 = mg.grid(1).p
    print(f"\n{_id(dims)} {method}: fp64 {n64} iterations, mixed with mixed_direct {n32}")
    assert h32[-1] <= PREC, (n32, h32)
    assert mg.nhydro.get_option("mixed_iterations") - it0 == n32 > 0
    # every coarsest solve of every F-cycle where the entry says the level is served (64x64x32: 8x8x4); 32x32x48 ends at 4x4x6, which the rule
    # declines: that solve must run the sweeps with the option on, to the same assertions, and the counter stands
    served = mg.nhydro.mixed_direct_cells(*dims) > 0
    assert served == (dims == (64, 64, 32))
    assert _solves(mg) - s0 == (n32 * mg.nlevs() if served else 0)
    assert n32 <= n64 + 2, (n32, n64, h32, h64)
    ro = oracle_relative_residual(o, p32)
    assert abs(ro - h32[-1]) <= 1e-9 * h32[-1], (ro, h32[-1])
    d = np.abs(p32 - p64).max() / np.abs(p64).max()
    assert d <= 1e-8, d


def test_krylov_over_the_fp32_cycle(mg):
    """krylov = 4 with krylov_precision = 32 at 64x64x32: the iteration count of mixed_direct = 0, +- 1"""
    dims = (64, 64, 32)
    _setup(mg, dims, "FC")
    rhs(mg, None, uvw(dims))
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("krylov_precision", 32)
    got = {}
    for direct in (0, 1):
        mg.nhydro.set_option("mixed_direct", direct)
        s0 = _solves(mg)
        n, hist = mg.solve_p(PREC, 50)
        assert hist[-1] <= PREC, (direct, n, hist)
        got[direct] = (n, _solves(mg) - s0)
    assert abs(got[1][0] - got[0][0]) <= 1, got
    assert got[0][1] == 0 and got[1][1] > 0, got


# ---- (f) the operator follows the matrix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_operator_follows_the_matrix(mg, method):
    """16x16x4: after a served solve, other matrices (a smooth zeta of a few metres): the product is the new fp64 relax's, a stale operator O(1) away"""
    dims = (16, 16, 4)
    pr = _setup(mg, dims, method)
    b, p_old = _check_product(mg, dims, 0, f"{_id(dims)} {method}, first matrix")
    dx, dy, zeta, h = pr.fields
    ii, jj = np.indices(zeta.shape)
    zeta2 = 3.0 * np.sin(2.0 * np.pi * ii / zeta.shape[0]) * np.cos(2.0 * np.pi * jj / zeta.shape[1]) + 1.5
    mg.nhydro_matrices(dx, dy, zeta2, h, pr.rmask, *pr.sigma)
    _, p_new = _check_product(mg, dims, 0, f"{_id(dims)} {method}, second matrix")
    assert not np.array_equal(p_new, p_old)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_small_any_nz_toggles_the_service(mg, method):
    """32x32x24 (coarsest 4x4x3): served with small_any_nz = 1, the sweeps and their bits with 0, served again with 1"""
    dims = (32, 32, 24)
    _setup(mg, dims, method, 1)
    b, p1 = _check_product(mg, dims, 1, f"{_id(dims)} {method} small_any_nz = 1")
    mg.nhydro.set_option("small_any_nz", 0)
    p0, grew = _coarsest(mg, b, 1)
    assert grew == 0
    sweeps, _ = _coarsest(mg, b, 0)
    assert np.array_equal(p0, sweeps)
    mg.nhydro.set_option("small_any_nz", 1)
    p2, grew = _coarsest(mg, b, 1)
    assert grew == 1 and np.array_equal(p2, p1)


# ---- (g) the fp64 direct solve is undisturbed -------------------------------------------------------------------------------------------
def test_fp64_direct_solve_undisturbed(mg):
    """64x64x16, red-black as it comes (rb_seq = 1, coarsest_direct = 1): the fp64 solve before and after a mixed solve with the option on"""
    dims = (64, 64, 16)
    _setup(mg, dims, "RB")
    mg.nhydro.set_option("rb_seq", 1)
    mg.nhydro.set_option("coarsest_direct", 1)
    rhs(mg, None, uvw(dims))
    d0 = mg.nhydro.get_option("coarsest_direct_solves")
    n_a, h_a = mg.solve_p(1e-10, 50)
    p_a = mg.grid(1).p
    assert mg.nhydro.get_option("coarsest_direct_solves") > d0
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro.set_option("mixed_direct", 1)
    s0 = _solves(mg)
    n_m, h_m = mg.solve_p(1e-10, 50)
    assert h_m[-1] <= 1e-10 and _solves(mg) > s0
    mg.nhydro.set_option("cycle_precision", 64)
    mg.nhydro.set_option("mixed_direct", 0)
    n_b, h_b = mg.solve_p(1e-10, 50)
    assert n_a == n_b and np.array_equal(h_a, h_b), (h_a, h_b)
    assert np.array_equal(mg.grid(1).p, p_a)
