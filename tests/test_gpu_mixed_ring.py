"""Option "mixed_ring": the software-pipelined fp32 colour pass (k_relax32r, mgx_mixed.hip) on the levels choose_relax32 (mgx_choice.h) gives it.

(a) mixed_op("relax", lev, n) with the option on against the fp64 relax (rb_seq = 0: the parallel red-black pass the fp32 one restates) on the
    same random p (halo filled) and b, n = 1 and ns_pre: within 1e-5 of max|fp64| in each region of the level -- the bound
    tests/test_gpu_mixed_precision.py puts on every fp32 kernel; a column or row taken one off gives O(1) on random fields.  Every
    physical-boundary image equals its interior value bit for bit, and "mixed_ring_passes" grows by four (four colours) or two (red-black) per
    sweep.  Every instance (nz = 16, 20, 24, 32, 40, 48, 64) at a level-1 size just above the small bound, with four colours and with red-black
    (cmatrix = 'real': the snapshot), 'simple' at 64x64x16; a ragged third wave; a served level below the first; the island mask; stretched
    sigma coordinates; and the launch geometry either side of its thresholds (GEOMETRY below).
(b) a declined level -- small, nz without an instance, tall -- keeps the row-by-row kernel: the option changes no bit and the counter stands.
(c) V-cycles from a random state (mixed_tail = 0 and 1 the same bits under the option) and solves: the assertions
    tests/test_gpu_mixed_precision.py makes on a mixed solve, with its numbers, and the Krylov loop over the fp32 cycle."""
import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, oracle_relative_residual, oracle_twin, regions, rhs, uvw

pytestmark = pytest.mark.gpu

OPTIONS = ("mixed_ring", "mixed_tail", "cycle_precision", "krylov", "krylov_precision", "rb_seq", "warm_start")
METHODS = {"FC": dict(relax_method="FC"), "RB": dict(relax_method="RB"), "FC-simple": dict(relax_method="FC", cmatrix="simple"),
           "RB-simple": dict(relax_method="RB", cmatrix="simple")}
PREC = 1e-12

mg = gpu_module(mixed_ring=0)
_restore_options = restore_options(*OPTIONS)


def _setup(mg, dims, method="FC", **kw):
    pr = gpu_problem(mg, dims, **dict(METHODS[method], solver_prec=PREC, solver_maxiter=50, **kw))
    mg.nhydro.set_option("rb_seq", 0)
    for k in ("krylov", "warm_start", "mixed_tail", "mixed_ring"):
        mg.nhydro.set_option(k, 0)
    mg.nhydro.set_option("cycle_precision", 64)
    return pr


def _random_level(mg, lev, rng):
    g = mg.grid(lev)
    g.set("p", rng.standard_normal(g._shape("p")))
    g.set("b", rng.standard_normal(g._shape("b")))
    mg.fill_halo(lev, "p")
    return g.p, g.b


def _put(mg, lev, state):
    g = mg.grid(lev)
    g.set("p", state[0])
    g.set("b", state[1])


def _mixed_relax(mg, lev, state, n, ring):
    """p after mixed_op("relax", lev, n) from `state`, and the growth of the counter"""
    mg.nhydro.set_option("mixed_ring", ring)
    _put(mg, lev, state)
    c0 = mg.nhydro.get_option("mixed_ring_passes")
    mg.nhydro.mixed_op("relax", lev, n)
    return mg.grid(lev).p, mg.nhydro.get_option("mixed_ring_passes") - c0


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


def _check_served(mg, levels, method, what, seed=51):
    rng = np.random.default_rng(seed)
    per_sweep = 4 if method.startswith("FC") else 2
    for lev in levels:
        state = _random_level(mg, lev, rng)
        for n in sorted({1, mg.nhydro.get_option("ns_pre")}):
            tag = f"{what} lev {lev} x{n}"
            p32, passes = _mixed_relax(mg, lev, state, n, 1)
            assert passes == per_sweep * n, (tag, passes)
            _put(mg, lev, state)
            mg.relax(lev, n)
            _close_fp64(p32, mg.grid(lev).p, tag)
            _mirrored(p32, tag)


# every instance, level 1 just above the small bound (32768 cells with nz <= 32; any size with nz > 32)
INSTANCES = [(64, 64, 16), (64, 64, 20), (64, 64, 24), (64, 64, 32), (32, 32, 40), (32, 32, 48), (32, 32, 64)]


def _id(d):
    return "x".join(map(str, d))


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("dims", INSTANCES, ids=_id)
def test_every_instance_matches_fp64(mg, dims, method):
    _setup(mg, dims, method)
    assert mg.nhydro.mixed_ring_levels(*dims) & 1
    _check_served(mg, [1], method, f"{_id(dims)} {method}")


@pytest.mark.parametrize("method", ["FC-simple", "RB-simple"])
def test_simple_matrix(mg, method):
    """cmatrix = 'simple': no k = 1 diagonal terms, no snapshot"""
    _setup(mg, (64, 64, 16), method)
    _check_served(mg, [1], method, f"64x64x16 {method}")


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_ragged_wave(mg, method):
    """32x320x16: ny / 2 = 160 lanes of a half-row, two full waves and a third with 32 lanes"""
    _setup(mg, (32, 320, 16), method)
    _check_served(mg, [1], method, f"32x320x16 {method}")


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_served_level_below_the_first(mg, method):
    """128x128x64: level 1 (nz = 64) and level 2 (64x64x32, 131072 cells)"""
    _setup(mg, (128, 128, 64), method)
    assert mg.nhydro.mixed_ring_levels(128, 128, 64) & 0b11 == 0b11
    _check_served(mg, [1, 2], method, f"128x128x64 {method}")


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("variant", ["bmask", "stretched"])
def test_variants(mg, variant, method):
    """the island mask (coefficients that vanish on land) and stretched sigma coordinates at 64x64x16"""
    _setup(mg, (64, 64, 16), method, **(dict(bmask=True) if variant == "bmask" else dict(sigma=(250.0, 0.4, 6.0))))
    _check_served(mg, [1], method, f"64x64x16 {method} {variant}")


# The launch geometry (choose_relax32 -> ch_pass_geometry, ch_ring_beyond_cache), red-black so that a colour has nx planes:
#   256x512x16   4 waves per half-row x 256 planes = 1024 workgroups of one plane (as every shape above: below 2048)
#   512x512x16   4 x 512 = 2048: the first size with two planes per workgroup
#   512x1024x16  8.4 M cells x 36 B > 256 MB: the first power-of-two size with the non-temporal instance (and two planes per workgroup)
GEOMETRY = [((256, 512, 16), 1, 0), ((512, 512, 16), 2, 0), ((512, 1024, 16), 2, 1)]


@pytest.mark.parametrize("dims,planes,stream", GEOMETRY, ids=[_id(d) for d, _, _ in GEOMETRY])
def test_launch_geometry_thresholds(mg, dims, planes, stream):
    _setup(mg, dims, "RB")
    # the launch itself is made by the function this entry reports: the case covers the variant it is named for
    c = mg.nhydro.mixed_ring_choice(*dims, dims[0])
    assert (c["served"], c["planes_per_workgroup"], c["stream"], c["instance_nz"]) == (1, planes, stream, 16), c
    _check_served(mg, [1], "RB", f"{_id(dims)} RB")


# ---- (b) declined levels --------------------------------------------------------------------------------------------------------------
# 32x32x32: exactly 32768 cells with nz <= 32, small; 32x32x16: small; 64x64x16: levels 2.. (32x32x8 and below: nz without an instance, and
# small); 16x32x128: tall (level 1), then 8x16x64 and below -- a hierarchy of one level more than nsmall allows is not needed: level 1 is the case
DECLINED = [((32, 32, 32), None), ((32, 32, 16), None), ((64, 64, 16), "below"), ((16, 32, 128), "first")]


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("dims,which", DECLINED, ids=[_id(d) for d, _ in DECLINED])
def test_declined_levels_keep_their_bits(mg, dims, which, method):
    _setup(mg, dims, method)
    nl = mg.nlevs()
    levels = {None: range(1, nl + 1), "below": range(2, nl + 1), "first": [1]}[which]
    mask = mg.nhydro.mixed_ring_levels(*dims)
    rng = np.random.default_rng(53)
    for lev in levels:
        assert not mask >> (lev - 1) & 1, (dims, lev, mask)
        state = _random_level(mg, lev, rng)
        for n in sorted({1, mg.nhydro.get_option("ns_pre")}):
            p0, c0 = _mixed_relax(mg, lev, state, n, 0)
            p1, c1 = _mixed_relax(mg, lev, state, n, 1)
            assert c0 == 0 and c1 == 0, (dims, lev, c0, c1)
            assert np.array_equal(p0, p1), f"{_id(dims)} {method} lev {lev} x{n}: {int((p0 != p1).sum())} cells differ"
            assert np.isfinite(p1).all() and not np.array_equal(p1, state[0])


# ---- (c) cycles and solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_vcycles_tail_on_and_off_same_bits(mg, method):
    """64x64x32: level 1 served, the tail from level 2 on.  mixed_op("vcycle", lev) from a random state on every level"""
    dims = (64, 64, 32)
    _setup(mg, dims, method)
    assert mg.nhydro.mixed_ring_levels(*dims) == 1 and mg.nhydro.mixed_tail_first(*dims) == 2
    rng = np.random.default_rng(57)
    nl = mg.nlevs()
    state = {lev: _random_level(mg, lev, rng) for lev in range(1, nl + 1)}
    mg.nhydro.set_option("mixed_ring", 1)
    out = []
    for tail in (0, 1):
        mg.nhydro.set_option("mixed_tail", tail)
        for lev, s in state.items():
            _put(mg, lev, s)
        r0, t0 = mg.nhydro.get_option("mixed_ring_passes"), mg.nhydro.get_option("mixed_tail_launches")
        mg.nhydro.mixed_op("vcycle", 1, 0)
        grew = mg.nhydro.get_option("mixed_ring_passes") - r0, mg.nhydro.get_option("mixed_tail_launches") - t0
        assert grew[0] > 0 and (grew[1] > 0) == (tail == 1), (tail, grew)
        out.append({lev: mg.grid(lev).p for lev in state})
    for lev in state:
        assert np.array_equal(out[0][lev], out[1][lev]), f"{method}: level {lev}: {int((out[0][lev] != out[1][lev]).sum())} cells of p differ"
        assert np.isfinite(out[1][lev]).all()
    assert not np.array_equal(out[1][1], state[1][0])


SOLVES = [((64, 64, 32), "FC"), ((64, 64, 32), "RB"), ((32, 32, 48), "FC")]


@pytest.mark.parametrize("dims,method", SOLVES, ids=[f"{_id(d)}-{m}" for d, m in SOLVES])
def test_mixed_solve(mg, dims, method):
    """cold start to 1e-12 with cycle_precision = 32 and the option on: what tests/test_gpu_mixed_precision.py::test_mixed_solve asserts"""
    pr = _setup(mg, dims, method)
    o = oracle_twin(pr, only=("relax_method", "cmatrix", "interp_type", "bmask"))
    rhs(mg, o, uvw(dims))
    n64, h64 = mg.solve_p(PREC, 50)
    p64 = mg.grid(1).p
    assert h64[-1] <= PREC, (n64, h64)
    mg.nhydro.set_option("cycle_precision", 32)
    mg.nhydro.set_option("mixed_ring", 1)
    it0, r0 = mg.nhydro.get_option("mixed_iterations"), mg.nhydro.get_option("mixed_ring_passes")
    n32, h32 = mg.solve_p(PREC, 50)
    p32 = mg.grid(1).p
    print(f"\n{_id(dims)} {method}: fp64 {n64} iterations, mixed with mixed_ring {n32}")
    assert h32[-1] <= PREC, (n32, h32)
    assert mg.nhydro.get_option("mixed_iterations") - it0 == n32 > 0
    assert mg.nhydro.get_option("mixed_ring_passes") > r0
    assert n32 <= n64 + 2, (n32, n64, h32, h64)
    ro = oracle_relative_residual(o, p32)
    assert abs(ro - h32[-1]) <= 1e-9 * h32[-1], (ro, h32[-1])
    d = np.abs(p32 - p64).max() / np.abs(p64).max()
    assert d <= 1e-8, d


def test_krylov_over_the_fp32_cycle(mg):
    """krylov = 4 with krylov_precision = 32 at 64x64x32: the iteration count of mixed_ring = 0, +- 1"""
    dims = (64, 64, 32)
    _setup(mg, dims, "FC")
    rhs(mg, None, uvw(dims))
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("krylov_precision", 32)
    got = {}
    for ring in (0, 1):
        mg.nhydro.set_option("mixed_ring", ring)
        r0 = mg.nhydro.get_option("mixed_ring_passes")
        n, hist = mg.solve_p(PREC, 50)
        assert hist[-1] <= PREC, (ring, n, hist)
        got[ring] = (n, mg.nhydro.get_option("mixed_ring_passes") - r0)
    assert abs(got[1][0] - got[0][0]) <= 1, got
    assert got[0][1] == 0 and got[1][1] > 0, got
