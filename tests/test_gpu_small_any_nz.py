"""Option "small_any_nz" on the GPU (include/mgx.h): a relax call on a closed level of at most 1024 columns with
nz = 3, 5, 6 or 7 in one launch of one workgroup, and the direct coarsest solve of a 16 x 16 x 3 level.

The instances expand the rows of the colour passes, and the build does not contract: four colours, red-black with cmatrix = 'simple', the
parallel red-black pass (rb_seq = 0) and the plane loop (rb_exact) are compared BIT FOR BIT with option 0 -- and, on the hierarchies the
reference has (no held pair), with the CPU oracle.  The red-black default (the sequential order at speed: the walk at nz = 3) keeps the
project's bound for that mode, 1e-12 of max|p| per relax call of rb_exact.  The levels of the held hierarchies are compared with option 0
only: tests/test_gpu_hold_odd_nz.py pins option 0 per level.

Tolerances: 1e-12 relative on histories of bit-identical fields (the norm is reduced in another order: test_gpu_vertical_sizes.py); 1e-10
on the red-black histories and fields after three iterations (the bound of the recorded red-black histories, test_gpu_parity.py); 1e-12
of max|p| between the direct coarsest product and the sweeps (the existing bound of "coarsest_direct")."""
import os
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import gpu_problem, hist_close, oracle_twin, rhs, uvw
from _ranks import free_port, run_process_ranks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
HC = 4e3

mg = gpu_module(small_any_nz=0, hold_odd_nz=0, rb_exact=0, rb_seq=1, coarsest_direct=1, periodic=0)

# shape -> (hold_odd_nz, the levels of the hierarchy)
LEVELS = {
    (32, 32, 6): (0, [(32, 32, 6), (16, 16, 3)]),                                  # nz 6 at 1024 columns; nz 3 in one wave
    (64, 64, 6): (0, [(64, 64, 6), (32, 32, 3)]),                                  # level 1 declined (4096 columns); nz 3 in four waves
    (32, 64, 6): (0, [(32, 64, 6), (16, 32, 3)]),                                  # non-square
    (64, 32, 6): (0, [(64, 32, 6), (32, 16, 3)]),
    (64, 64, 12): (0, [(64, 64, 12), (32, 32, 6), (16, 16, 3)]),                   # two served levels under one that is not
    (32, 32, 12): (0, [(32, 32, 12), (16, 16, 6), (8, 8, 3)]),                     # the register class of nz 6
    (32, 32, 10): (1, [(32, 32, 10), (16, 16, 5), (8, 8, 5), (4, 4, 5)]),          # nz 5; a level narrower than a wave
    (64, 64, 10): (1, [(64, 64, 10), (32, 32, 5), (16, 16, 5), (8, 8, 5), (4, 4, 5)]),   # nz 5 at 1024 columns
    (32, 32, 14): (1, [(32, 32, 14), (16, 16, 7), (8, 8, 7), (4, 4, 7)]),
    (64, 64, 14): (1, [(64, 64, 14), (32, 32, 7), (16, 16, 7), (8, 8, 7), (4, 4, 7)]),
}
# mode -> (namelist, options, compared bit for bit with option 0?, the oracle computes the same bits?)
MODES = {
    "FC": (dict(relax_method="FC"), {}, True, True),
    "RB_simple": (dict(relax_method="RB", cmatrix="simple"), {}, True, True),    # no k = 1 diagonals: order independent
    "RB_parallel": (dict(relax_method="RB"), {"rb_seq": 0}, True, False),         # the snapshot pass: not the reference's order
    "RB_exact": (dict(relax_method="RB"), {"rb_exact": 1}, True, True),
    "RB_default": (dict(relax_method="RB"), {}, False, False),
}


def _ids(d):
    return "%dx%dx%d" % d


def _served(dims, mode="FC"):
    """the served set of include/mgx.h, less the classes the dispatcher declines by measurement: the red-black default
    where only the plane loop could serve it (nz = 6, 7; nz = 5 above 64 columns), and 'simple' red-black at nz = 6, 7 above 256 columns"""
    nx, ny, nz = dims
    if not (nz in (3, 5, 6, 7) and nx * ny <= 1024 and nx % 2 == 0 and ny % 2 == 0):
        return False
    if mode == "RB_default":
        return (nz == 3 and ny // 2 <= 64) or (nz == 5 and nx * ny <= 64)
    if mode == "RB_simple":
        return not (nz >= 6 and nx * ny > 256)
    return True


def _setup(mg, dims, bmask=False, oracle=False, periodic=0, **par):
    """the seamount problem of `dims` (held where LEVELS says so); oracle: also on the CPU oracle (hierarchies without a held pair)"""
    hold = LEVELS[dims][0]
    pr = gpu_problem(mg, dims, bmask=bmask, sigma=(HC, 0.0, 0.0), init_options=dict(hold_odd_nz=hold, periodic=periodic),
                     **dict(dict(relax_method="FC", solver_prec=1e-10), **par))
    got = [(mg.grid(l).nx, mg.grid(l).ny, mg.grid(l).nz) for l in range(1, mg.nlevs() + 1)]
    assert got == LEVELS[dims][1], got
    if not oracle:
        return None
    assert not hold
    o = oracle_twin(pr)
    assert o.nlevs == len(got)
    return o


def _calls(mg):
    return mg.nhydro.get_option("small_any_nz_calls")


def _launches(mg):
    return mg.nhydro.counters()["launches"]


def _relax_from(mg, lev, p, b, n, small, **options):
    """relax(lev, n) from p, b (halo filled) under the option; returns p with its halo, the launches and the served calls it took"""
    g = mg.grid(lev)
    g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
    mg.nhydro.set_option("small_any_nz", small)
    for k, v in options.items():
        mg.nhydro.set_option(k, v)
    l0, c0 = _launches(mg), _calls(mg)
    mg.relax(lev, n)
    out = g.get("p")
    return out, _launches(mg) - l0, _calls(mg) - c0


def _check_relax(mg, dims, mode, bmask=False):
    par, opts, bits, oracle_bits = MODES[mode]
    hold = LEVELS[dims][0]
    for k, v in opts.items():
        mg.nhydro.set_option(k, v)
    try:
        o = _setup(mg, dims, bmask=bmask, oracle=oracle_bits and not hold, **par)
        rng = np.random.default_rng(sum(dims))
        small = [l for l, d in enumerate(LEVELS[dims][1], 1) if _served(d)]
        assert small
        for lev in small:
            g = mg.grid(lev)
            for n in (1, 3, 40):
                p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
                p1, l1, c1 = _relax_from(mg, lev, p, b, n, 1)
                if not _served(LEVELS[dims][1][lev - 1], mode):   # a class declined by measurement: the launches and the bits of option 0
                    p0, l0, c0 = _relax_from(mg, lev, p, b, n, 0)
                    assert c1 == 0 and c0 == 0 and l1 == l0 > 1, (lev, n, l1, l0, c1)
                    assert np.array_equal(p1, p0), (lev, n)
                    continue
                assert (l1, c1) == (1, 1), (lev, n, l1, c1)
                if bits:
                    p0, l0, c0 = _relax_from(mg, lev, p, b, n, 0)
                    assert c0 == 0 and l0 > 1, (lev, n, l0, c0)
                    assert np.array_equal(p1, p0), (lev, n, np.abs(p1 - p0).max())
                    if o is not None:
                        o.field("p", lev)[...] = p; o.field("b", lev)[...] = b; o.fill_halo(lev, "p")
                        o.relax(lev, n)
                        assert np.array_equal(p1, o.field("p", lev)), (lev, n, np.abs(p1 - o.field("p", lev)).max())
                else:
                    pe, _, ce = _relax_from(mg, lev, p, b, n, 0, rb_exact=1)
                    mg.nhydro.set_option("rb_exact", 0)
                    err = np.abs(p1 - pe).max() / np.abs(pe).max()
                    print(f"{_ids(dims)} level {lev} relax({n}) {mode}: {err:.3e} of max|p| from rb_exact")
                    assert ce == 0 and err <= 1e-12, (lev, n, err)
    finally:
        mg.nhydro.set_option("small_any_nz", 0); mg.nhydro.set_option("rb_exact", 0); mg.nhydro.set_option("rb_seq", 1)


# ---- 1. every served level from a random p, b ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dims", list(LEVELS), ids=_ids)
def test_relax_every_served_level(mg, dims, mode):
    """relax(lev, n), n = 1, 3, 40, on every small level with nz = 3, 5, 6, 7: served = one launch, and the bits of option 0 (halo included)
    -- the oracle's too where the reference has the hierarchy and the order; the red-black default within 1e-12 of max|p| of rb_exact.  A
    class the dispatcher declines by measurement takes the launches of option 0 and leaves the counter alone."""
    _check_relax(mg, dims, mode)


@pytest.mark.parametrize("mode", ["FC", "RB_exact", "RB_default"])
@pytest.mark.parametrize("dims", [(32, 32, 12), (64, 64, 10)], ids=_ids)
def test_relax_island_mask(mg, dims, mode):
    """the same with bmask (the island mask): rows of masked cells, stored coefficients"""
    _check_relax(mg, dims, mode, bmask=True)


# ---- 2. routing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,lev", [((32, 32, 6), 1), ((32, 32, 6), 2), ((64, 64, 6), 2), ((32, 32, 12), 2), ((64, 64, 10), 2), ((32, 32, 14), 4)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_served_call_is_one_launch(mg, dims, lev):
    """four colours, relax(lev, 3): option 1 = one launch and one served call; option 0 = the counter rests and the call takes the generic
    launches, a colour pass and a physical-halo fill per colour (3 sweeps x 4 colours x 2)"""
    _setup(mg, dims)
    try:
        mg.nhydro.set_option("small_any_nz", 0)
        l0, c0 = _launches(mg), _calls(mg)
        mg.relax(lev, 3)
        assert (_launches(mg) - l0, _calls(mg) - c0) == (24, 0)
        mg.nhydro.set_option("small_any_nz", 1)
        l0, c0 = _launches(mg), _calls(mg)
        mg.relax(lev, 3)
        assert (_launches(mg) - l0, _calls(mg) - c0) == (1, 1)
    finally:
        mg.nhydro.set_option("small_any_nz", 0)


@pytest.mark.parametrize("case", ["4096_columns", "periodic", "GS"])
def test_declined_level_moves_nothing(mg, case):
    """a level outside the served set takes the launches of option 0 and leaves the counter alone: 64 x 64 x 6 level 1 (4096 columns),
    every level of a periodic hierarchy (an open side), relax_method = 'GS'"""
    dims, levs, kw = {"4096_columns": ((64, 64, 6), [1], {}), "periodic": ((32, 32, 6), [1, 2], {"periodic": 1}),
                      "GS": ((32, 32, 6), [1, 2], {"relax_method": "GS"})}[case]
    try:
        _setup(mg, dims, **kw)
        rng = np.random.default_rng(3)
        for lev in levs:
            g = mg.grid(lev)
            p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
            p0, l0, c0 = _relax_from(mg, lev, p, b, 2, 0)
            p1, l1, c1 = _relax_from(mg, lev, p, b, 2, 1)
            assert c0 == 0 and c1 == 0 and l1 == l0 > 1, (lev, l0, l1, c0, c1)
            assert np.array_equal(p0, p1)
    finally:
        mg.nhydro.set_option("small_any_nz", 0)
        mg.nhydro_clean()
        mg.nhydro.set_option("periodic", 0)


# ---- 3. solves -------------------------------------------------------------------------------------------------------------------------
def _solve3(mg, dims, small, oracle=False, **par):
    o = _setup(mg, dims, oracle=oracle, **par)
    mg.nhydro.set_option("small_any_nz", small)
    rhs(mg, o, uvw(dims))
    l0, c0 = _launches(mg), _calls(mg)
    n, hist = mg.solve_p(1e-30, 3)
    out = dict(n=n, hist=hist, launches=_launches(mg) - l0, calls=_calls(mg) - c0,
               p=[mg.grid(l).get("p") for l in range(1, mg.nlevs() + 1)], b=[mg.grid(l).get("b") for l in range(1, mg.nlevs() + 1)])
    return out, o


@pytest.mark.parametrize("dims", [(64, 64, 12), (64, 64, 6), (64, 64, 10)], ids=_ids)
def test_fc_solve_bitwise(mg, dims):
    """three iterations of solve_p with four colours: p and b of every level bit for bit between option 1 and 0, the history to 1e-12,
    fewer launches; without a held pair also against the oracle's solve_p (tests/test_gpu_vertical_sizes.py::test_fc_solve_bitwise)"""
    try:
        s0, _ = _solve3(mg, dims, 0)
        s1, o = _solve3(mg, dims, 1, oracle=not LEVELS[dims][0])
        assert s0["n"] == s1["n"] == 3 and hist_close(s1["hist"], s0["hist"], rtol=1e-12, atol=1e-13, same_length=True), (s1["hist"], s0["hist"])
        for lev, (a, c) in enumerate(zip(s1["p"], s0["p"]), 1):
            assert np.array_equal(a, c), (lev, "p", np.abs(a - c).max())
        for lev, (a, c) in enumerate(zip(s1["b"], s0["b"]), 1):
            assert np.array_equal(a, c), (lev, "b", np.abs(a - c).max())
        print(f"{_ids(dims)}: {s0['launches']} launches with option 0, {s1['launches']} with 1 ({s1['calls']} served calls)")
        assert s0["calls"] == 0 and s1["calls"] > 0 and s1["launches"] < s0["launches"]
        if o is not None:
            no, ho, _ = o.solve_p(1e-30, 3)
            assert no == 3 and hist_close(s1["hist"], ho, rtol=1e-12, atol=1e-13, same_length=True), (s1["hist"], ho)
            for lev in range(1, o.nlevs + 1):
                for name in ("p", "b"):
                    a, c = s1[name][lev - 1], o.field(name, lev)
                    assert np.array_equal(a, c), (lev, name, np.abs(a - c).max())
    finally:
        mg.nhydro.set_option("small_any_nz", 0)


def test_rb_default_solve(mg):
    """the red-black default on 64 x 64 x 12, three iterations: histories and p within 1e-10 of option 0 (the walk at nz = 3 and the
    direct coarsest solve are the same maps in another association)"""
    try:
        s0, _ = _solve3(mg, (64, 64, 12), 0, relax_method="RB")
        s1, _ = _solve3(mg, (64, 64, 12), 1, relax_method="RB")
        assert s0["n"] == s1["n"] == 3 and hist_close(s1["hist"], s0["hist"], rtol=1e-10, atol=1e-13, same_length=True), (s1["hist"], s0["hist"])
        err = np.abs(s1["p"][0] - s0["p"][0]).max() / np.abs(s0["p"][0]).max()
        print(f"red-black default, 64x64x12, three iterations: p {err:.3e} of max|p| from option 0; launches {s0['launches']} -> {s1['launches']}")
        assert err <= 1e-10
        assert s1["calls"] > 0 and s1["launches"] < s0["launches"]
    finally:
        mg.nhydro.set_option("small_any_nz", 0)


def test_nhydro_solve_bitwise(mg):
    """the whole nhydro_solve from a rough state on 32 x 32 x 12 with four colours: u, v, w bit for bit between option 1 and 0"""
    dims = (32, 32, 12)
    out = []
    try:
        for small in (0, 1):
            _setup(mg, dims, solver_maxiter=8)
            mg.nhydro.set_option("small_any_nz", small)
            u, v, w = uvw(dims, seed=17)
            c0 = _calls(mg)
            mg.nhydro_solve(u, v, w)
            out.append((u, v, w, mg.grid(1).p, _calls(mg) - c0))
        assert out[0][4] == 0 and out[1][4] > 0
        for a, c in zip(out[0][:4], out[1][:4]):
            assert np.array_equal(a, c), np.abs(a - c).max()
    finally:
        mg.nhydro.set_option("small_any_nz", 0)


# ---- 4. the direct coarsest solve ------------------------------------------------------------------------------------------------------
def _vcycle_rb(mg, small, direct):
    dims = (64, 64, 12)
    _setup(mg, dims, relax_method="RB")
    mg.nhydro.set_option("small_any_nz", small); mg.nhydro.set_option("coarsest_direct", direct)
    rhs(mg, None, uvw(dims))
    d0 = mg.nhydro.get_option("coarsest_direct_solves")
    mg.nhydro.Vcycle(1)
    return mg.grid(1).get("p"), mg.nhydro.get_option("coarsest_direct_solves") - d0


def test_direct_coarsest_solve_nz3(mg):
    """64 x 64 x 12, red-black default: the 16 x 16 x 3 coarsest level (768 cells) takes the direct solve with option 1 only; p after one
    V-cycle within 1e-12 of max|p| of the sweeps (coarsest_direct = 0)"""
    try:
        _, d = _vcycle_rb(mg, 0, 1)
        assert d == 0
        p1, d = _vcycle_rb(mg, 1, 1)
        assert d == 1
        ps, d = _vcycle_rb(mg, 1, 0)
        assert d == 0
        err = np.abs(p1 - ps).max() / np.abs(ps).max()
        print(f"direct coarsest solve of 16x16x3: {err:.3e} of max|p| from the sweeps after one V-cycle")
        assert err <= 1e-12
    finally:
        mg.nhydro.set_option("small_any_nz", 0); mg.nhydro.set_option("coarsest_direct", 1)


def test_toggling_rebuilds_the_operator(mg):
    """the option is part of the cached operator's key: after a solve with option 1 (direct coarsest solve), a solve with option 0 from
    the same start equals a fresh option-0 run bit for bit, and a further one with option 1 equals the first"""
    dims = (64, 64, 12)

    def solve(small):
        mg.nhydro.set_option("small_any_nz", small)
        g = mg.grid(1)
        g.set("p", np.zeros(g._shape("p")))
        rhs(mg, None, uvw(dims))
        d0 = mg.nhydro.get_option("coarsest_direct_solves")
        n, hist = mg.solve_p(1e-30, 2)
        return g.get("p"), hist, mg.nhydro.get_option("coarsest_direct_solves") - d0

    try:
        _setup(mg, dims, relax_method="RB")
        fresh0 = solve(0)
        _setup(mg, dims, relax_method="RB")
        first1 = solve(1)
        again0 = solve(0)
        again1 = solve(1)
        assert fresh0[2] == 0 and again0[2] == 0 and first1[2] > 0 and again1[2] == first1[2]
        assert np.array_equal(again0[0], fresh0[0]) and np.array_equal(again0[1], fresh0[1])
        assert np.array_equal(again1[0], first1[0]) and np.array_equal(again1[1], first1[1])
    finally:
        mg.nhydro.set_option("small_any_nz", 0)


# ---- 5. a gathered level ---------------------------------------------------------------------------------------------------------------
def test_gathered_level_2x2():
    """2 x 2 ranks of 16 x 16 x 12 (four processes, tests/_gpu_small_any_nz_worker.py), four colours, three iterations: level 2 (8 x 8 x 6
    with neighbours) is declined, level 3 (8 x 8 x 3, gathered and closed) is served on every rank; every rank's p of every level bit
    for bit between option 1 and 0"""
    run_process_ranks(os.path.join(HERE, "_gpu_small_any_nz_worker.py"), 4, (4, 2, 2, free_port(), 16, 16, 12, 8))
