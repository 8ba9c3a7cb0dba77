"""Option "mixed_tail": the small levels of an fp32 cycle inside one workgroup (k_tail32, mgx_mixed.hip) against one launch per colour pass
and transfer ("mixed_tail" = 0), on identical inputs, bit for bit (np.array_equal) -- the tail kernel calls the device functions of the
per-launch kernels, so it owes the same bits:

  (i)   mixed_op("relax", lev, n) on every small level, n = 1, ns_pre, ns_coarsest -- and against the fp64 relax within the bound
        tests/test_gpu_mixed_precision.py puts on every fp32 kernel, 1e-5 of max|fp64| in each region of the level;
  (ii)  mixed_op("vcycle", lev) from every level, from random p and b: p of every level, halos included.  A solve only ever enters a cycle
        with e = 0, which hides an error in the e-couplings of the first pass; this does not;
  (iii) solve_p with three iterations: p, the history, "mixed_iterations".

Shapes: the smallest that take each path of the kernel (SHAPES below); at 512x512x64 the launch counters as well."""
import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, regions, rhs, uvw

pytestmark = pytest.mark.gpu

OPTIONS = ("mixed_tail", "cycle_precision", "krylov", "krylov_precision", "rb_seq", "warm_start")
# relax_method and cmatrix: four colours, red-black with the k = 1 snapshot before each colour, and 'simple' (no k = 1 diagonal terms) with either
METHODS = {"FC": dict(relax_method="FC"), "RB": dict(relax_method="RB"), "FC-simple": dict(relax_method="FC", cmatrix="simple"),
           "RB-simple": dict(relax_method="RB", cmatrix="simple")}
# 16x16x8   three levels, all small: the register instances 8, 4, 2
# 32x32x24  all small, the generic pass: nz = 24, 12, 6 and the odd 3
# 96x48x4   two levels; 1152 columns in a four-colour colour: the strided loop takes a second, ragged trip; ny / 2 = 24 is no wave multiple
# 64x64x16  the tail starts at level 2: the transfers that straddle its boundary stay launches
# 128x64x32 level 2 = 64x32x16 = exactly 32768 cells, the bound; the instances 16 and 8 (the 256-lane class of the kernel)
# 32x32x20  nz = 20, 10, 5, 2: an odd nz in the middle of the tail, halved by integer division (the top fine row has no coarse row of its own)
SHAPES = [((16, 16, 8), 1), ((32, 32, 24), 1), ((96, 48, 4), 1), ((64, 64, 16), 2), ((128, 64, 32), 2), ((32, 32, 20), 1)]
SHAPE_IDS = ["x".join(map(str, d)) for d, _ in SHAPES]


mg = gpu_module()


_restore_options = restore_options(*OPTIONS)


def _setup(mg, dims, method="FC", bmask=False, **par):
    nx, ny, nz = dims
    gpu_problem(mg, dims, bmask=bmask, **dict(METHODS[method], solver_prec=1e-12, solver_maxiter=50, **par))
    mg.nhydro.set_option("rb_seq", 0)   # the fp64 red-black pass the fp32 one restates
    for k in ("krylov", "warm_start"):
        mg.nhydro.set_option(k, 0)
    mg.nhydro.set_option("cycle_precision", 64)
    first = mg.nhydro.mixed_tail_first(nx, ny, nz)
    assert first >= 1
    return first


def _random_state(mg, rng):
    """random p (halo filled) and b on every level"""
    state = {}
    for lev in range(1, mg.nlevs() + 1):
        g = mg.grid(lev)
        g.set("p", rng.standard_normal(g._shape("p")))
        g.set("b", rng.standard_normal(g._shape("b")))
        mg.fill_halo(lev, "p")
        state[lev] = (g.p, g.b)
    return state


def _put(mg, state):
    for lev, (p, b) in state.items():
        g = mg.grid(lev)
        g.set("p", p)
        g.set("b", b)


def _both(mg, state, run):
    """run() from `state` with mixed_tail = 0 and 1 -> the p of every level after each, and the tail launches of the second"""
    out = []
    for tail in (0, 1):
        mg.nhydro.set_option("mixed_tail", tail)
        _put(mg, state)
        t0 = mg.nhydro.get_option("mixed_tail_launches")
        run()
        launches = mg.nhydro.get_option("mixed_tail_launches") - t0
        assert (launches > 0) == (tail == 1), (tail, launches)
        out.append({lev: mg.grid(lev).p for lev in state})
    return out[0], out[1], launches


def _same(a, b, what):
    for lev in a:
        bad = np.argwhere(a[lev] != b[lev])
        assert bad.size == 0, f"{what}: level {lev}: {len(bad)} cells of p differ, first (i, j, k) {bad[:4].tolist()}, max |diff| {np.abs(a[lev] - b[lev]).max():.3e}"


def _close_fp64(a, ref, what):
    ra = regions(a)
    for name, r in regions(ref).items():
        m = np.abs(r).max()
        assert m > 0, f"{what}, {name}: the fp64 result is zero there"
        d = np.abs(ra[name] - r).max()
        assert d <= 1e-5 * m, f"{what}, {name}: |fp32 - fp64| {d:.3e} > 1e-5 * {m:.3e}"


def _check_relax(mg, first, rng, what):
    nl = mg.nlevs()
    sweeps = sorted({1, mg.nhydro.get_option("ns_pre"), mg.nhydro.get_option("ns_coarsest")})
    state = _random_state(mg, rng)
    for lev in range(first, nl + 1):
        for n in sweeps:
            one = {lev: state[lev]}
            p0, p1, launches = _both(mg, one, lambda: mg.nhydro.mixed_op("relax", lev, n))
            assert launches == 1
            _same(p0, p1, f"{what}: relax x{n}")
            _put(mg, one)
            mg.relax(lev, n)
            _close_fp64(p1[lev], mg.grid(lev).p, f"{what}: relax x{n} lev {lev}")


def _check_vcycles(mg, first, rng, what):
    nl = mg.nlevs()
    state = _random_state(mg, rng)
    for lev in range(1, nl + 1):
        p0, p1, launches = _both(mg, state, lambda: mg.nhydro.mixed_op("vcycle", lev, 0))
        assert launches == 1, (lev, launches)   # the part of the cycle below max(lev, first)
        _same(p0, p1, f"{what}: vcycle from level {lev}")
        assert all(np.isfinite(a).all() for a in p1.values())
        assert np.abs(p1[nl]).max() > 0


def _check_solve(mg, dims, what, maxite=3):
    rhs(mg, None, uvw(dims))
    out = []
    for tail in (0, 1):
        mg.nhydro.set_option("mixed_tail", tail)
        key = "krylov_mixed_iterations" if mg.nhydro.get_option("krylov") else "mixed_iterations"
        it0, t0 = mg.nhydro.get_option(key), mg.nhydro.get_option("mixed_tail_launches")
        n, hist = mg.solve_p(1e-30, maxite)   # (the tolerance is out of reach: maxite iterations)
        out.append((n, hist, mg.grid(1).p, mg.nhydro.get_option(key) - it0, mg.nhydro.get_option("mixed_tail_launches") - t0))
    (n0, h0, p0, it0, tl0), (n1, h1, p1, it1, tl1) = out
    assert n0 == n1 == it0 == it1 == maxite, (what, n0, n1, it0, it1)
    assert np.array_equal(h0, h1), (what, h0, h1)
    _same({1: p0}, {1: p1}, f"{what}: solve_p")
    assert tl0 == 0 and tl1 > 0, (what, tl0, tl1)
    assert h1[-1] < h1[0]
    return tl1


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("dims,first", SHAPES, ids=SHAPE_IDS)
def test_tail_is_the_launches_bit_for_bit(mg, dims, first, method):
    assert _setup(mg, dims, method) == first
    what = f"{'x'.join(map(str, dims))} {method}"
    rng = np.random.default_rng(41)
    _check_relax(mg, first, rng, what)
    _check_vcycles(mg, first, rng, what)
    mg.nhydro.set_option("cycle_precision", 32)
    tails = _check_solve(mg, dims, what)
    assert tails == 3 * first   # per F-cycle: its own tail and one V-cycle tail from each level above `first`


@pytest.mark.parametrize("method", ["FC", "RB"])
@pytest.mark.parametrize("variant", ["bmask", "nearest"])
def test_variants(mg, variant, method):
    """the island mask (coefficients that vanish on land) and interp_type = 'nearest' (the other coarse2fine) at 64x64x16"""
    dims = (64, 64, 16)
    first = _setup(mg, dims, method, **(dict(bmask=True) if variant == "bmask" else dict(interp_type="nearest")))
    rng = np.random.default_rng(43)
    what = f"64x64x16 {method} {variant}"
    _check_relax(mg, first, rng, what)
    _check_vcycles(mg, first, rng, what)
    mg.nhydro.set_option("cycle_precision", 32)
    _check_solve(mg, dims, what)


@pytest.mark.parametrize("method", ["FC", "RB"])
def test_krylov_with_fp32_cycles(mg, method):
    """"krylov" = 2 with "krylov_precision" = 32 at 64x64x16: the preconditioner is the same fp32 F-cycle"""
    dims = (64, 64, 16)
    first = _setup(mg, dims, method)
    mg.nhydro.set_option("krylov", 2)
    mg.nhydro.set_option("krylov_precision", 32)
    assert _check_solve(mg, dims, f"64x64x16 {method} krylov") == 3 * first


def _cycle_launches(nl, first, pre, post, nc, sweep):
    """launches of one fp32 F-cycle, restated from fcycle32 / vcycle32 / relax32 (mgx_cycle.cpp).  first = 0: every colour pass (and red-black
    snapshot) and every transfer is a launch, `sweep` per sweep.  first > 0 (option "mixed_tail"): a relax call on a level >= first is one
    launch, and a cycle entered at lev1 hands everything from level max(lev1, first) down and back up to one launch."""
    relax = lambda lev, n: 0 if n == 0 else (1 if first and lev >= first else sweep * n)

    def vcycle(lev1):   # with Fcycle's leading coarse2fine
        hand = max(lev1, first) if first else nl
        n = 0
        for lev in range(lev1, hand):
            n += (1 if lev == lev1 else 0) + relax(lev, pre) + 1
        n += 1 if first else relax(nl, nc)
        for lev in range(hand - 1, lev1 - 1, -1):
            n += 1 + relax(lev, post)
        return n

    hand = first if first else nl
    return (hand - 1) + (1 if first else relax(nl, nc)) + sum(vcycle(lev) for lev in range(hand - 1, 0, -1))


def test_bench_size_and_launch_counters(mg):
    """512x512x64, four colours: three iterations the same bit for bit, and per iteration the tail kernel runs `first` = 4 times (the F-cycle's
    tail and the V-cycle tails from levels 3, 2, 1) while the launches drop from the per-launch schedule's count to the tail schedule's.  An
    iteration = the cycle + 4: the conversion of r, the conversion of e, the fp64 residual and the reduction of its norm."""
    dims = (512, 512, 64)
    first = _setup(mg, dims, "FC")
    assert first == 4 and mg.nlevs() == 6
    mg.nhydro.set_option("cycle_precision", 32)
    assert _check_solve(mg, dims, "512x512x64 FC") == 3 * first
    pre, post, nc = (mg.nhydro.get_option(k) for k in ("ns_pre", "ns_post", "ns_coarsest"))
    per = {}
    for tail in (0, 1):
        mg.nhydro.set_option("mixed_tail", tail)
        cnt = []
        for maxite in (2, 3):
            c0, t0 = mg.nhydro.counters()["launches"], mg.nhydro.get_option("mixed_tail_launches")
            n, _ = mg.solve_p(1e-30, maxite)
            assert n == maxite
            cnt.append((mg.nhydro.counters()["launches"] - c0, mg.nhydro.get_option("mixed_tail_launches") - t0))
        per[tail] = (cnt[1][0] - cnt[0][0], cnt[1][1] - cnt[0][1])
    hand0, hand1 = (_cycle_launches(6, f, pre, post, nc, 4) + 4 for f in (0, first))
    print(f"\n512x512x64 FC: launches per iteration {per[0][0]} -> {per[1][0]} (by hand {hand0} -> {hand1}), tail launches per iteration {per[1][1]}")
    assert per[0] == (hand0, 0), (per, hand0)
    assert per[1] == (hand1, first), (per, hand1)
    assert per[1][0] < per[0][0]


def test_single_level_hierarchy(mg):
    """16x16x2 has one level: the F-cycle is the coarsest relax, one tail launch per iteration"""
    dims = (16, 16, 2)
    assert _setup(mg, dims, "RB") == 1 and mg.nlevs() == 1
    rng = np.random.default_rng(47)
    _check_relax(mg, 1, rng, "16x16x2 RB")
    mg.nhydro.set_option("cycle_precision", 32)
    assert _check_solve(mg, dims, "16x16x2 RB") == 3
