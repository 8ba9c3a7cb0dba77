"""The smoother identities on the GPU, with no oracle call in any assertion (tests/_smoother_identity.py states the rule, the bounds and
the cases).

The column system of the line smoother -- diagonal, sub-diagonal, the 12 to 16 off-column terms, the bottom-row diagonals of
cmatrix = 'real' -- is written out in more than a dozen kernel families (k_relax_wave, _reg, _tiny, _small, _ks, _ks2, _ksp, _nz stored and
matrix-free, _tall, _tall_st, _colour, _gs_front, _gs_front_any, the rbseq walk and correction), and the residual kernels hold further texts
of the same operator.  Every other smoother test holds relax() to the CPU oracle's relax(), i.e. to a restatement; here each level's
relax() is held to the same level's compute_residual(), through the ABI alone, on one rank:

  1  relax(lev, 2) from p* with b = A p* leaves p*                                      (every method, every column)
  2  relax(lev, 1) from p* + delta on the first colour's non-ring columns gives p*     (four colours, red-black)
  3  after relax(lev, 1) from random p, b the last colour's non-ring columns have r = 0 (four colours, red-black; 'real': rows k >= 2)

with the controls that show each check looked (delta on the last colour stays; the other colours keep a residual; row k = 1 of red-black
'real' keeps one).  Gauss-Seidel: check 1 only.  A wrong coefficient, slot, pivot, neighbour index or colour offset in a smoother breaks
them at O(1e-2 .. 1) on the levels that kernel serves; the bounds are 16 x what the CPU oracle's own smoother leaves (1.9e-12, 1.5e-12,
9.5e-13: _smoother_identity.TOL).  Red-black with cmatrix = 'real' in the sequential order at speed -- every level of the cases with
rb_seq = 1 and rb_exact = 0: the window, walk_apply, scan_apply, the fused launch, k_relax_wave's walk -- takes the project's bound of that
mode instead, 1e-12 of max|p| per relax call (checks 1 and 2), and in check 3 what such an error can leave in r; rb_exact = 1 and
rb_seq = 0 take the 16 x bounds.

Each case runs every level of its hierarchy, one seed.  Which kernel served a level is shown only by the counters the ABI has
(rbseq_window_colours, tall_stored_passes, small_any_nz_calls, launches).

Measured on the MI355X (the test prints every level's figures; none was taken into a bound): checks 1, 2, 3 at most 8.1e-14, 9.1e-14,
4.3e-14 (level 1 of the island at 32x32x96 and 32x32x128, where the oracle has 1.2e-13, 9.5e-14, 5.9e-14), every other case at most
7.7e-15, 6.6e-15, 1.8e-15; the sequential-order routes 1.1e-15 without the island.  Smallest controls: 2.1e-2 (check 2), 0.34 (check 3),
2.5e-4 (row k = 1, the 4x64x2 level of 16x256x8).  The adjoint: at most 1.2e-17."""
import numpy as np
import pytest

import _smoother_identity as S
from _gpu import gpu_module
from _problem import gpu_problem, on_gpu

pytestmark = pytest.mark.gpu

# every option a case sets, at its default (tests/test_host_logic.py holds the defaults of the red-black ones)
DEFAULTS = dict(hold_odd_nz=0, periodic=0, small_any_nz=0, rb_exact=0, rb_seq=1, rbseq_window=1, rbseq_fuse=1, rbseq_fuse_min=4 << 20)
mg = gpu_module(**DEFAULTS)


@pytest.fixture(autouse=True)
def _restore_options(mg):
    """after every test: no grid (hold_odd_nz and periodic cannot be set back under a hierarchy built with them), every option at its default"""
    yield
    mg.nhydro_clean()
    for k, v in DEFAULTS.items():
        mg.nhydro.set_option(k, v)


def _counter(mg, name):
    return mg.nhydro.counters()["launches"] if name == "launches" else mg.nhydro.get_option(name)


def _levels(mg, case, be, levels, tag=""):
    """the checks on the given levels; returns {counter: {level: growth}} for the counters the case names"""
    names = list(case.moved or {}) + list(case.still or ())
    grew = {n: {} for n in names}
    for lev in levels:
        before = {n: _counter(mg, n) for n in names}
        f = S.run_level(be, lev, case.method, case.cmatrix == "real", S.SEEDS[0], rb_seq=S.is_rb_seq(case))
        for n in names:
            grew[n][lev] = _counter(mg, n) - before[n]
        print(case.name + tag, "level", lev, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in f.items() if k != "tol"},
              "bounds", {k: "%.2e" % v for k, v in f["tol"].items()})
        S.assert_level(f, (case.name + tag, lev))
    return grew


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_smoother_identities(mg, case):
    assert all(k in DEFAULTS for k in list(case.options or {}) + list(case.init or {})), "an option this file does not restore"
    on_gpu(mg, S.case_problem(case), init_options=case.init)
    for k, v in (case.options or {}).items():
        mg.nhydro.set_option(k, v)
    be = S.GpuBackend(mg)
    nlev = mg.nlevs()
    assert be.dims(1) == case.dims and nlev >= 2
    grew = _levels(mg, case, be, range(1, nlev + 1))
    for name, levels in (case.moved or {}).items():
        for lev in levels:
            assert grew[name][lev] > 0, (case.name, name, "did not move on level", lev, grew[name])
    for name in case.still or ():
        assert not any(grew[name].values()), (case.name, name, grew[name])
    if case.stored:     # writing cA makes level 1 read the stored slots from now on: the same checks on the other text of the level
        g = mg.grid(1)
        g.set("cA", g.get("cA"))
        _levels(mg, case, be, [1], tag=" (stored slots)")
    if case.fewer_than:
        def launches():
            S.fixed_point(be, 1, S.SEEDS[0])     # leaves p*, b = A p* on the level
            n0 = _counter(mg, "launches")
            mg.relax(1, 1)
            return _counter(mg, "launches") - n0
        own = launches()
        for k, v in case.fewer_than.items():
            mg.nhydro.set_option(k, v)
        other = launches()
        print(case.name, "launches of relax(1, 1):", own, "against", other, "under", case.fewer_than)
        assert own < other, (case.name, own, other)


def test_hold_odd_nz_cases_have_the_levels_they_are_named_for(mg):
    """32x32x40 under hold_odd_nz ends at 4x4x5, the horizontal bound, and holds nothing; the held levels of nz = 5 are those of 32x32x10"""
    from _hold_ref import held_levels
    want = {(32, 32, 40): [], (32, 32, 10): [2, 3]}
    for dims in S.HELD_DIMS:
        gpu_problem(mg, dims, init_options=dict(hold_odd_nz=1), relax_method="FC")
        assert held_levels(mg) == want[dims], (dims, held_levels(mg))
    assert [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)] == [10, 5, 5, 5]


@pytest.mark.parametrize("dims", S.ADJOINT_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_nearest_transfers_are_adjoint(mg, dims):
    """<R r, q> = <r, P q> through mg.fine2coarse / mg.coarse2fine with interp_type = 'nearest' on every level pair with an even fine nz
    (the oracle: 7.3e-18 of ||r|| ||P q||, sums in longdouble; bound 16 x the held reference's 1.4e-17)"""
    gpu_problem(mg, dims, relax_method="FC", interp_type="nearest")
    be = S.GpuBackend(mg)
    pairs = S.even_fine_pairs(be)
    assert pairs and pairs == list(range(1, mg.nlevs()))      # every pair of these hierarchies (32x32x12 ends at 8x8x3)
    for lev in pairs:
        d = S.adjoint_defect(be, lev, S.SEEDS[0])
        print(dims, be.dims(lev), "->", be.dims(lev + 1), "%.2e" % d)
        assert d <= S.ADJOINT_TOL, (dims, lev, d)


def test_nearest_transfers_are_adjoint_on_held_pairs(mg):
    """the held pairs of 32x32x10 under hold_odd_nz (16x16x5 -> 8x8x5 -> 4x4x5: the rows are kept, the transfers are the reference's 2-D ones
    per row); their reference, tests/_hold_ref.py, keeps the identity to 1.4e-17 (tests/test_oracle.py).  32x32x40 has no held pair."""
    from _hold_ref import held_levels
    gpu_problem(mg, (32, 32, 10), init_options=dict(hold_odd_nz=1), relax_method="FC", interp_type="nearest")
    be = S.GpuBackend(mg)
    held = held_levels(mg)
    assert held == [2, 3]
    for lev in held:
        d = S.adjoint_defect(be, lev, S.SEEDS[0])
        print("held", be.dims(lev), "->", be.dims(lev + 1), "%.2e" % d)
        assert d <= S.ADJOINT_TOL, (lev, d)
