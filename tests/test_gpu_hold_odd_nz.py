"""Option "hold_odd_nz" on the GPU (include/mgx.h): once a level has an odd nz the coarser levels keep it and coarsen
in x and y only, so that nz = 20, 28, 40 converge.

The reference has no such hierarchy.  What pins it: the transfers of a held pair against the reference's 2-D operators in numpy, bit for
bit (tests/_hold_ref.py); the matrix and the smoother of every held level against an Oracle of that level's size fed with the library's own
dx, dy, zeta, h of the level, bit for bit with four colours; a V-cycle over the held levels against the composite of those; and solves to
1e-10 whose residual a level-1 Oracle of the full size recomputes in fp64.

Measured on the MI355X (iterations to 1e-10, seamount): 64 x 64 x 32: 8 and 64 x 64 x 48: 6 on the default hierarchy, 64 x 64 x 40 held: 6,
with "krylov" = 4 also 6 (bound: max(8, 6) + 2 = 10); 32 x 32 x 20 held: 6 with four colours, 6 with red-black, 9 with the island mask, 8
with interp_type = 'nearest', 6 with "periodic" = 3; 64 x 64 x 28 held: 10.  The fp64 residuals the Oracle recomputes equal the last
history entries to the printed digits (2.8e-11 .. 3.9e-11).  Red-black default on the held levels: <= 1.6e-16 of max|p| per relax call."""
import os
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import gpu_problem, oracle_twin, rhs, uvw
from _ranks import free_port, run_process_ranks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
HC = 4e3


mg = gpu_module(hold_odd_nz=0, periodic=0, rb_seq=1, rb_exact=0, krylov=0, krylov_precision=64, cycle_precision=64, mixed_tail=0, exact_halos=0, keep_r=0)


def _init(mg, dims, hold=1, bmask=False, **par):
    """mgx_init reads the option: clean, set, init; the seamount geometry (bmask: with the island mask)"""
    return gpu_problem(mg, dims, bmask=bmask, sigma=(HC, 0.0, 0.0), init_options=dict(hold_odd_nz=hold),
                       **dict(dict(relax_method="FC", solver_prec=1e-10), **par))


def _fp64_residual(pr, p, b):
    """||b - A p|| / ||b|| by a level-1 Oracle of the full size (its own coarse levels are never used)"""
    o = oracle_twin(pr)
    o.field("p")[...] = p; o.field("b")[...] = b
    o.residual(1)
    r = o.field("r")[1:-1, 1:-1]
    return np.sqrt((r ** 2).sum()) / np.sqrt((b[1:-1, 1:-1] ** 2).sum())


# ---- 1. the transfers of a held pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("dims", [(32, 32, 20), (48, 80, 12), (64, 64, 28)], ids=lambda d: "%dx%dx%d" % d)
def test_transfers_bitwise(mg, dims, interp):
    """fine2coarse(lev) and coarse2fine(lev) of every held pair from random fields against numpy, bit for bit: b_c with its physical images,
    p_c exactly 0; the fine r (interior and images: the operator keeps it) and p = p + r over the whole array.  48 x 80 x 12: ragged
    half-rows (12 x 20 -> 6 x 10, no multiple of 16)."""
    from _hold_ref import held_levels, mirror, prolong_held, restrict_held
    _init(mg, dims, interp_type=interp)
    held = held_levels(mg)
    assert held and {(32, 32, 20): [3], (48, 80, 12): [3], (64, 64, 28): [3, 4]}[dims] == held
    rng = np.random.default_rng(5)
    for exact in (0, 1):
        mg.nhydro.set_option("exact_halos", exact); mg.nhydro.set_option("keep_r", exact)
        for lev in held:
            F, C = mg.grid(lev), mg.grid(lev + 1)
            assert F.nz == C.nz and F.nx == 2 * C.nx and F.ny == 2 * C.ny
            r = rng.standard_normal(F._shape("r"))
            F.set("r", r); C.set("p", rng.standard_normal(C._shape("p"))); C.set("b", rng.standard_normal(C._shape("b")))
            mg.fine2coarse(lev)
            assert np.array_equal(C.get("b"), mirror(restrict_held(r))), (lev, "b_c")
            assert not C.get("p").any(), (lev, "p_c")
            pc = mirror(rng.standard_normal(C._shape("p")))
            pf = mirror(rng.standard_normal(F._shape("p")))
            C.set("p", pc); F.set("p", pf); F.set("r", np.full(F._shape("r"), np.nan))
            mg.coarse2fine(lev)
            want = mirror(prolong_held(pc, interp == "linear"))
            assert np.array_equal(F.get("r"), want), (lev, "r")
            assert np.array_equal(F.get("p"), pf + want), (lev, "p")
            assert np.array_equal(C.get("p"), pc)
    mg.nhydro.set_option("exact_halos", 0); mg.nhydro.set_option("keep_r", 0)


# ---- 2. and 3. the matrix and the smoother of every held level -------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 20), (48, 80, 12), (64, 64, 28)], ids=lambda d: "%dx%dx%d" % d)
def test_matrix_and_four_colour_relax_of_held_levels_bitwise(mg, dims):
    """cA of every level of a held pair equals the level-1 cA of the Oracle built at that level's size from the level's own dx, dy, zeta,
    h; relax(lev, 1) and relax(lev, 3) from random p and b equal that Oracle's, bit for bit"""
    from _hold_ref import held_levels, level_oracle
    _init(mg, dims)
    rng = np.random.default_rng(9)
    levels = sorted({l for h in held_levels(mg) for l in (h, h + 1)})
    for lev in levels:
        o = level_oracle(mg, lev, HC, relax_method="FC")
        g = mg.grid(lev)
        a, c = g.get("cA")[1:-1, 1:-1], o.field("cA")[1:-1, 1:-1]
        assert np.array_equal(a, c), (lev, "cA", np.abs(a - c).max())
        for sweeps in (1, 3):
            p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
            g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
            o.field("p")[...] = p; o.field("b")[...] = b; o.fill_halo(1, "p")
            mg.relax(lev, sweeps); o.relax(1, sweeps)
            assert np.array_equal(g.get("p"), o.field("p")), (lev, sweeps)
        o.close()


def test_red_black_default_on_held_levels(mg):
    """the red-black default (sequential order at speed) on the held levels of 32 x 32 x 20: each relax call within 1e-12 of max|p| of the
    Oracle's sequential loop, the bound of tests/test_gpu_vertical_sizes.py::test_rb_default_relax_every_level"""
    from _hold_ref import held_levels, level_oracle
    _init(mg, (32, 32, 20), relax_method="RB")
    assert mg.nhydro.get_option("rb_seq") == 1 and mg.nhydro.get_option("rb_exact") == 0
    rng = np.random.default_rng(41)
    for lev in sorted({l for h in held_levels(mg) for l in (h, h + 1)}):
        o = level_oracle(mg, lev, HC, relax_method="RB")
        g = mg.grid(lev)
        p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
        g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
        o.field("p")[...] = p; o.field("b")[...] = b; o.fill_halo(1, "p")
        for call in range(2):
            mg.relax(lev, 1); o.relax(1, 1)
            a, c = g.get("p"), o.field("p")
            err = np.abs(a - c).max() / np.abs(c).max()
            print(f"level {lev} call {call}: red-black default against the sequential loop {err:.3e}")
            assert err <= 1e-12, (lev, call, err)
            g.set("p", c.copy())   # per relax call: the next one starts from the yardstick's state
        o.close()


# ---- 4. a cycle on the held levels alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 20), (64, 64, 28)], ids=lambda d: "%dx%dx%d" % d)
def test_vcycle_on_the_held_levels_bitwise(mg, dims):
    """a random b (and p) on the first held level, Vcycle(that level): p equals the composite of the per-level Oracles and the numpy
    transfers, bit for bit, on every level it touches"""
    from _hold_ref import composite_vcycle, held_levels, level_oracle
    _init(mg, dims)
    first, last = held_levels(mg)[0], mg.nlevs()
    os_ = [level_oracle(mg, lev, HC, relax_method="FC") for lev in range(first, last + 1)]
    rng = np.random.default_rng(13)
    g = mg.grid(first)
    p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
    g.set("p", p); g.set("b", b); mg.fill_halo(first, "p")
    os_[0].field("p")[...] = p; os_[0].field("b")[...] = b; os_[0].fill_halo(1, "p")
    par = {k: mg.nhydro.get_option(k) for k in ("ns_pre", "ns_post", "ns_coarsest")}
    mg.Vcycle(first)
    composite_vcycle(os_, first, par["ns_pre"], par["ns_post"], par["ns_coarsest"])
    for q, o in enumerate(os_):
        a, c = mg.grid(first + q).get("p"), o.field("p")
        assert np.array_equal(a, c), (first + q, np.abs(a - c).max())
        o.close()
    assert not np.array_equal(mg.grid(first).get("p"), p)


# ---- 5. solves at 1e-10 ----------------------------------------------------------------------------------------------------------------
def _solve(mg, dims, maxit=30, **kw):
    hold = kw.pop("hold", 1)
    bmask = kw.pop("bmask", False)
    geo = _init(mg, dims, hold=hold, bmask=bmask, **kw)
    rhs(mg, None, uvw(dims))
    b = mg.grid(1).b
    n, hist = mg.solve_p(1e-10, maxit)
    return n, hist, geo, mg.grid(1).p, b


SOLVES = [((32, 32, 20), dict(relax_method="FC")), ((32, 32, 20), dict(relax_method="RB")), ((64, 64, 28), dict(relax_method="FC")),
          ((64, 64, 40), dict(relax_method="FC")), ((32, 32, 20), dict(relax_method="FC", bmask=True)), ((32, 32, 20), dict(relax_method="FC", interp_type="nearest"))]


@pytest.mark.parametrize("dims,kw", SOLVES, ids=["%dx%dx%d-%s" % (*d, "-".join(str(v) for v in k.values())) for d, k in SOLVES])
def test_solves_to_1e10(mg, dims, kw):
    """solve_p to 1e-10 on a held hierarchy: the history falls monotonically and the fp64 residual of the returned p, recomputed by a
    level-1 Oracle of the full size, is <= 1e-10 ||b|| (1 + 1e-6)"""
    n, hist, geo, p, b = _solve(mg, dims, **dict(kw))
    print(dims, kw, "iterations", n, "history", hist)
    assert n < 30 and hist[-1] <= 1e-10, (n, hist)
    assert np.all(np.diff(hist) < 0), hist
    res = _fp64_residual(geo, p, b)
    print("fp64 residual by the Oracle", res)
    assert res <= 1e-10 * (1 + 1e-6), res


def test_iterations_of_nz40_against_its_even_neighbours(mg):
    """64 x 64 x 40 held (four colours, seamount, 1e-10) needs at most max(iterations at 64 x 64 x 32, at 64 x 64 x 48) + 2, the neighbours
    measured here on the default hierarchy (the CPU oracle gives 8 and 6 for them: the bound is then 10; the margin is for a threshold
    crossed one iteration later); "krylov" = 4 at 64 x 64 x 40 needs no more iterations than the plain solve.
    Measured on the MI355X: 8 and 6 for the neighbours, 6 for 64 x 64 x 40 held, 6 with "krylov" = 4."""
    n32 = _solve(mg, (64, 64, 32), hold=0, relax_method="FC")[0]
    n48 = _solve(mg, (64, 64, 48), hold=0, relax_method="FC")[0]
    n40, hist40 = _solve(mg, (64, 64, 40), relax_method="FC")[:2]
    mg.nhydro.set_option("krylov", 4)
    try:
        nk, histk = _solve(mg, (64, 64, 40), relax_method="FC")[:2]
    finally:
        mg.nhydro.set_option("krylov", 0)
    print(f"iterations to 1e-10: nz = 32: {n32}, nz = 48: {n48} (default hierarchy); nz = 40 held: {n40}, with krylov = 4: {nk}")
    assert hist40[-1] <= 1e-10 and histk[-1] <= 1e-10
    assert n40 <= max(n32, n48) + 2, (n32, n40, n48)
    assert nk <= n40, (nk, n40)


# ---- 6. process grid -------------------------------------------------------------------------------------------------------------------
def test_process_grid_2x2_bitwise():
    """2 x 2 ranks of 16 x 16 x 20 (four processes, tests/_gpu_hold_grid_worker.py), four colours, three iterations: every rank's p on
    every level and b hold the block of the one-rank 32 x 32 x 20 run bit for bit, through the default transport and through the hooks"""
    run_process_ranks(os.path.join(HERE, "_gpu_hold_grid_worker.py"), 4, (4, 2, 2, free_port(), 16, 16, 20, 8))


# ---- 7. periodic -----------------------------------------------------------------------------------------------------------------------
def test_periodic_converges_and_rolls(mg):
    """"periodic" = 3 at 32 x 32 x 20 held: the solve converges to 1e-10, and every input rolled by 16 cells along i (a whole and even
    number of cells on each of the four levels) rolls p bit for bit"""
    from test_gpu_periodic import geometry, matrices, velocities_from, velocity_bases
    dims, per, s = (32, 32, 20), 3, 16
    g = geometry(32, 32, per)
    bases = velocity_bases(32, 32, 20, per, 11)

    def run(geo, bas):
        mg.nhydro_clean()
        mg.nhydro.set_option("periodic", per); mg.nhydro.set_option("hold_odd_nz", 1)
        mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(relax_method="FC", solver_prec=1e-10))
        assert [mg.grid(l).nz for l in range(1, mg.nlevs() + 1)] == [20, 10, 5, 5]
        matrices(mg, geo, per)
        mg.nhydro.compute_rhs(*velocities_from(bas, per))
        n, hist = mg.solve_p(1e-10, 30)
        return n, hist, mg.grid(1).p[1:-1, 1:-1]
    try:
        n, hist, p = run(g, bases)
        print("periodic = 3, 32 x 32 x 20 held:", n, "iterations", hist)
        assert n < 30 and hist[-1] <= 1e-10 and np.all(np.diff(hist) < 0), hist
        g2 = dict(g)
        for name in ("dx", "dy", "zeta", "h"):
            g2[name] = np.roll(g[name], s, axis=0)
        n2, hist2, p2 = run(g2, tuple(np.roll(b, s, axis=2) for b in bases))
        assert n2 == n and not np.array_equal(p, p2)
        assert np.array_equal(np.roll(p, s, axis=0), p2)
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("periodic", 0)


# ---- 8. the option on, no odd level ----------------------------------------------------------------------------------------------------
def test_option_on_without_an_odd_level_changes_nothing(mg):
    """32 x 32 x 16 (nz 16, 8, 4, 2): p after three iterations and mgx_counters with the option on equal the run with it off, for four
    colours and the red-black default"""
    for method in ("FC", "RB"):
        out = []
        for hold in (0, 1):
            _init(mg, (32, 32, 16), hold=hold, relax_method=method)
            rhs(mg, None, uvw((32, 32, 16)))
            c0 = mg.nhydro.counters()
            n, hist = mg.solve_p(1e-30, 3)
            c1 = mg.nhydro.counters()
            out.append((n, hist, mg.grid(1).p, {k: c1[k] - c0[k] for k in c0}, [mg.grid(l).nz for l in range(1, mg.nlevs() + 1)]))
        (n0, h0, p0, c0, z0), (n1, h1, p1, c1, z1) = out
        assert z0 == z1 == [16, 8, 4, 2]
        assert n0 == n1 == 3 and np.array_equal(h0, h1) and np.array_equal(p0, p1)
        assert c0 == c1 and c0["launches"] > 0, (c0, c1)


def test_fp32_cycles_refused_with_a_held_pair_only(mg):
    """cycle_precision = 32, krylov_precision = 32 (and mixed_tail with them) are refused where the hierarchy has a held pair, in words that
    name the option; the same settings are served with the option on and no odd level (32 x 32 x 16); a change of the option under a live
    hierarchy is refused"""
    from mgroms_amd._lib import MgxError

    def settings():
        yield ("cycle_precision", 32), ()
        yield ("cycle_precision", 32), (("mixed_tail", 1),)
        yield ("krylov_precision", 32), (("krylov", 2),)
    try:
        for dims, served in (((32, 32, 20), False), ((32, 32, 16), True)):
            _init(mg, dims)
            rhs(mg, None, uvw(dims))
            for (name, value), extra in settings():
                for k, v in extra:
                    mg.nhydro.set_option(k, v)
                mg.nhydro.set_option(name, value)
                try:
                    n, hist = mg.solve_p(1e-8, 30)
                    assert served and hist[-1] <= 1e-8, (dims, name, hist)
                except MgxError as e:
                    assert not served, str(e)
                    assert '"hold_odd_nz" = 1' in str(e) and "fp32 cycles (cycle_precision = 32, krylov_precision = 32, mixed_tail)" in str(e), str(e)
                finally:
                    mg.nhydro.set_option(name, 64)
                    for k, v in extra:
                        mg.nhydro.set_option(k, 0)
            n, hist = mg.solve_p(1e-8, 30)   # and the hierarchy is usable afterwards
            assert hist[-1] <= 1e-8
            with pytest.raises(MgxError, match="hold_odd_nz = 0: the hierarchy in use was built with hold_odd_nz = 1"):
                mg.nhydro.set_option("hold_odd_nz", 0)
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("hold_odd_nz", 0)
