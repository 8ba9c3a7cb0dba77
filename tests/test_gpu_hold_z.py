"""Option "hold_z_levels" on the GPU (include/mgx.h): the first m coarsenings keep nz and halve nx, ny, so that
cells taller than wide (the seamount at 128 x 128 x 16: dx = 78 m, dz = 250 m) are coarsened in x and y until they are not.

The reference has no such hierarchy.  What pins it is what pins "hold_odd_nz" (tests/test_gpu_hold_odd_nz.py): the transfers of every held
pair -- level 1 -> 2 included -- against the reference's 2-D operators in numpy, bit for bit (tests/_hold_ref.py); the matrix and the
smoother of every held level against an Oracle of that level's size; twelve V-cycles against the composite of those Oracles, the numpy
transfers and the reference's Vcycle below the last held level; solves whose residual a level-1 Oracle recomputes in fp64.  New here is the
one-kernel down leg of a held pair (mgx_resrest_held.hip): its coarse b has the bits of the two launches, its norm agrees to 1e-13.

Measured on the MI355X: twelve V-cycles at 128 x 128 x 16 with m = 2 end at 7.91e-10 (the CPU composite: 7.9e-10; m = 0: 5.6e-2); solve_p to
1e-8 there: 4 iterations with m = 2 for four colours and for red-black, 50 without reaching it (2.1e-6, 2.4e-6) with m = 0; the closing
norms of the fused and the unfused route agree to the last bit on the three shapes; red-black default on the held levels <= 3.6e-16 of
max|p| per relax call; 32 x 32 x 16 periodic = 3 with m = 1: 6 iterations to 1e-10; 64 x 64 x 16 with m = 1: 6, with "krylov" = 4 also 6."""
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
CASES = [((32, 32, 16), 1), ((48, 80, 12), 2), ((64, 64, 16), 1)]
IDS = ["%dx%dx%d-m%d" % (*d, m) for d, m in CASES]
BIG = (128, 128, 16)


mg = gpu_module(hold_z_levels=0, hold_odd_nz=0, periodic=0, rb_seq=1, rb_exact=0, krylov=0, krylov_precision=64, cycle_precision=64, mixed_tail=0,
                exact_halos=0, keep_r=0, fuse_closing=1, hold_z_fuse=1)


def _init(mg, dims, m, bmask=False, **par):
    """mgx_init reads the option: clean, set, init; the seamount geometry (bmask: with the island mask)"""
    return gpu_problem(mg, dims, bmask=bmask, sigma=(HC, 0.0, 0.0), init_options=dict(hold_z_levels=m),
                       **dict(dict(relax_method="FC", solver_prec=1e-10), **par))


def _nz(mg):
    return [mg.grid(lev).nz for lev in range(1, mg.nlevs() + 1)]


def _fp64_residual(pr, p, b):
    """||b - A p|| / ||b|| by a level-1 Oracle of the full size (its own coarse levels are never used)"""
    o = oracle_twin(pr)
    o.field("p")[...] = p; o.field("b")[...] = b
    o.residual(1)
    r = o.field("r")[1:-1, 1:-1]
    o.close()
    return np.sqrt((r ** 2).sum()) / np.sqrt((b[1:-1, 1:-1] ** 2).sum())


# ---- 1. the live table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_live_table_equals_host_table(mg, dims, m):
    from _hold_ref import held_levels
    _init(mg, dims, m)
    table = mg.nhydro.level_table(*dims, hold_z_levels=m)
    assert mg.nlevs() == len(table)
    for lev, t in enumerate(table, 1):
        g = mg.grid(lev)
        assert (g.nx, g.ny, g.nz, g.gather, g.neighb) == (t["nx"], t["ny"], t["nz"], t["gather"], t["neighb"]), lev
    assert held_levels(mg) == list(range(1, m + 1))
    assert mg.nhydro.get_option("hold_z_levels") == m


# ---- 2. the transfers of every held pair, level 1 -> 2 included ------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_transfers_bitwise(mg, dims, m, interp):
    """fine2coarse(lev) and coarse2fine(lev) of every held pair from random fields against numpy, bit for bit: b_c with its physical images,
    p_c exactly 0; the fine r and p = p + r over the whole array.  48 x 80 x 12: ragged half-rows on levels 2 and 3."""
    from _hold_ref import held_levels, mirror, prolong_held, restrict_held
    _init(mg, dims, m, interp_type=interp)
    rng = np.random.default_rng(5)
    try:
        for exact in (0, 1):
            mg.nhydro.set_option("exact_halos", exact); mg.nhydro.set_option("keep_r", exact)
            for lev in held_levels(mg):
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
    finally:
        mg.nhydro.set_option("exact_halos", 0); mg.nhydro.set_option("keep_r", 0)


# ---- 3. the one-kernel down leg of a held pair ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bmask", [False, True], ids=["matrix-free", "bmask-stored"])
@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_fused_down_leg_has_the_bits_of_the_two_launches(mg, dims, m, bmask):
    """Vcycle2(lev, lev + 1) from the same random p and b on every held pair: b of the coarse level (what the down leg leaves, physical
    images included) and p of the fine level with "keep_r" = 0 -- residual and 2-D restriction in one kernel, r never written -- equal the
    "keep_r" = 1 route, compute_residual then k_fine2coarse_held, bit for bit, and the "hold_z_fuse" = 0 route, the same two launches with
    nothing else changed; and b_c equals the numpy restriction of the r that
    compute_residual leaves after the same pre-smoothing.  The read-only counter "hold_z_fused" moves by one per down leg on the first
    route and not at all on the second.  Matrix-free on the level's slopes, and on the stored slots under bmask."""
    from _hold_ref import held_levels, mirror, restrict_held
    _init(mg, dims, m, bmask=bmask)
    rng = np.random.default_rng(17)
    ns_pre = mg.nhydro.get_option("ns_pre")
    try:
        for lev in held_levels(mg):
            F, C = mg.grid(lev), mg.grid(lev + 1)
            p = rng.standard_normal(F._shape("p")); b = rng.standard_normal(F._shape("b"))
            out = []
            for keep, fuse in ((0, 1), (1, 1), (0, 0)):
                mg.nhydro.set_option("keep_r", keep); mg.nhydro.set_option("hold_z_fuse", fuse)
                F.set("p", p); F.set("b", b); mg.fill_halo(lev, "p")
                C.set("b", np.full(C._shape("b"), np.nan))
                c0 = mg.nhydro.get_option("hold_z_fused")
                mg.Vcycle2(lev, lev + 1)
                out.append((C.get("b"), F.get("p"), mg.nhydro.get_option("hold_z_fused") - c0))
            (b0, p0, n0), (b1, p1, n1), (b2, p2, n2) = out
            assert (n0, n1, n2) == (1, 0, 0), (lev, n0, n1, n2)
            assert np.isfinite(b0).all() and np.array_equal(b0, b1), (lev, np.abs(b0 - b1).max())
            assert np.array_equal(p0, p1), lev
            assert np.array_equal(b0, b2) and np.array_equal(p0, p2), lev   # the A/B option: two launches, nothing else changed
            # the yardstick of the yardstick: the same pre-smoothing, compute_residual, numpy
            F.set("p", p); F.set("b", b); mg.fill_halo(lev, "p")
            mg.relax(lev, ns_pre); mg.compute_residual(lev)
            assert np.array_equal(b1, mirror(restrict_held(F.get("r")))), lev
    finally:
        mg.nhydro.set_option("keep_r", 0); mg.nhydro.set_option("hold_z_fuse", 1)


@pytest.mark.parametrize("bmask", [False, True], ids=["matrix-free", "bmask-stored"])
@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_fused_closing_residual_on_a_held_pair(mg, dims, m, bmask):
    """three solve_p iterations with "fuse_closing" = 1 (levels 1 and 2 are a held pair: the closing residual of an iteration is the held
    pair's kernel with the norm) against "fuse_closing" = 0 (compute_residual, then Fcycle's two launches): p bit for bit, every history
    entry within 1e-13 relative (the norm's sum is a pair rounded once, formed in another order); the counter moves with 1 only"""
    out = []
    for fuse in (1, 0):
        _init(mg, dims, m, bmask=bmask, solver_prec=1e-30)
        mg.nhydro.set_option("fuse_closing", fuse)
        try:
            rhs(mg, None, uvw(dims, seed=23))
            c0 = mg.nhydro.get_option("hold_z_fused")
            n, hist = mg.solve_p(1e-30, 3)
            out.append((n, hist, mg.grid(1).p, mg.grid(1).r, mg.nhydro.get_option("hold_z_fused") - c0))
        finally:
            mg.nhydro.set_option("fuse_closing", 1)
    (n1, h1, p1, r1, c1), (n0, h0, p0, r0, c0) = out
    print(dims, m, "bmask" if bmask else "", "closing norms", h1, "relative difference", np.abs(h1 - h0) / h0)
    assert n1 == n0 == 3 and np.array_equal(p1, p0) and np.array_equal(r1, r0)
    assert np.all(np.abs(h1 - h0) <= 1e-13 * h0), (h1, h0)
    # fused: three closing residuals + the down legs of the F-cycles' V-cycles on the held pairs; not fused: the down legs alone
    assert c1 == c0 + 3 and c0 > 0, (c1, c0)


# ---- 4. the matrix and the smoother of every held level --------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_matrix_and_four_colour_relax_of_held_levels_bitwise(mg, dims, m):
    """cA of every level of a held pair equals the level-1 cA of the Oracle built at that level's size from the level's own dx, dy, zeta,
    h; relax(lev, 1) and relax(lev, 3) from random p and b equal that Oracle's, bit for bit"""
    from _hold_ref import held_levels, level_oracle
    _init(mg, dims, m)
    rng = np.random.default_rng(9)
    for lev in sorted({l for h in held_levels(mg) for l in (h, h + 1)}):
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


@pytest.mark.parametrize("dims,m", CASES, ids=IDS)
def test_red_black_default_on_held_levels(mg, dims, m):
    """the red-black default (sequential order at speed) on every level of a held pair: each relax call within 1e-12 of max|p| of the
    Oracle's sequential loop, the bound of tests/test_gpu_hold_odd_nz.py"""
    from _hold_ref import held_levels, level_oracle
    _init(mg, dims, m, relax_method="RB")
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
            print(f"{dims} level {lev} call {call}: red-black default against the sequential loop {err:.3e}")
            assert err <= 1e-12, (lev, call, err)
            g.set("p", c.copy())
        o.close()


# ---- 5. twelve V-cycles against the CPU composite ---------------------------------------------------------------------------------------
def _composite_vcycle(os_, ns_pre, ns_post):
    """Vcycle(1) on a hierarchy whose first len(os_) - 1 pairs are held: relax and residual of a held level by its own Oracle, the transfers
    by the numpy operators, and from the last Oracle's level down the reference's own Vcycle (that Oracle's whole hierarchy)"""
    from _hold_ref import mirror, prolong_held, restrict_held
    n = len(os_)
    for q in range(n - 1):
        os_[q].relax(1, ns_pre)
        os_[q].residual(1)
        os_[q + 1].field("b")[...] = mirror(restrict_held(os_[q].field("r")))
        os_[q + 1].field("p")[...] = 0.0
    os_[n - 1].vcycle(1)
    for q in range(n - 2, -1, -1):
        r = mirror(prolong_held(os_[q + 1].field("p"), True))
        p = os_[q].field("p")
        p[...] = p + r
        os_[q].relax(1, ns_post)


def test_twelve_vcycles_against_the_composite(mg):
    """128 x 128 x 16, m = 2, four colours, seamount, the resting column: twelve mgx_vcycle(1) from p = 0 against the composite of one
    Oracle per held level (fed the library's dx, dy, zeta, h of the level), the numpy transfers between them and the reference's Vcycle
    from level 3 down.  p bit for bit after every cycle, ||r|| / ||b|| to 1e-12 relative (the norm's sum has another order), and the last
    entry below 1e-8: the composite reaches 7.9e-10 on the CPU and the m = 0 hierarchy 5.6e-2, so this cannot pass without the option."""
    from _hold_ref import level_oracle
    _init(mg, BIG, 2)
    assert _nz(mg) == [16, 16, 16, 8, 4, 2]
    rhs(mg, None, uvw(BIG))
    b = mg.grid(1).b
    bn = np.sqrt((b[1:-1, 1:-1] ** 2).sum())
    os_ = [level_oracle(mg, lev, HC, relax_method="FC") for lev in (1, 2, 3)]
    os_[0].field("b")[...] = b; os_[0].field("p")[...] = 0.0
    mg.grid(1).set("p", np.zeros_like(b))
    ns_pre, ns_post = mg.nhydro.get_option("ns_pre"), mg.nhydro.get_option("ns_post")
    hist, want = [], []
    for it in range(12):
        mg.Vcycle(1)
        _composite_vcycle(os_, ns_pre, ns_post)
        assert np.array_equal(mg.grid(1).p, os_[0].field("p")), it
        hist.append(mg.compute_residual(1) / bn); want.append(os_[0].residual(1) / bn)
    for o in os_:
        o.close()
    hist, want = np.array(hist), np.array(want)
    print("twelve V-cycles, 128 x 128 x 16, m = 2:", hist)
    assert np.all(np.abs(hist - want) <= 1e-12 * want), (hist, want)
    assert hist[-1] < 1e-8, hist


# ---- 6. solves -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["FC", "RB"])
def test_solve_at_128x128x16_needs_fewer_iterations(mg, method):
    """solve_p to 1e-8 at 128 x 128 x 16 within solver_maxiter: with m = 2 (the hint's value) the history falls monotonically, the fp64
    residual a level-1 Oracle recomputes is <= 1e-8 ||b|| (1 + 1e-6), and the solve needs strictly fewer iterations than with m = 0.
    Measured on the MI355X: see DESIGN.md 7.1.1."""
    from mgroms_amd.testcases import seamount_geometry
    dx, dy, _, h = seamount_geometry(BIG[0], BIG[1], 1, 1, 0)
    assert mg.nhydro.hold_z_hint(dx, dy, h, BIG[2]) == 2
    out = {}
    for m in (0, 2):
        pr = _init(mg, BIG, m, relax_method=method, solver_prec=1e-8)
        maxit = mg.nhydro.get_option("solver_maxiter")
        rhs(mg, None, uvw(BIG))
        b = mg.grid(1).b
        n, hist = mg.solve_p(1e-8, maxit)
        out[m] = (n, hist, pr, mg.grid(1).p, b)
        print(f"128 x 128 x 16 {method} m = {m}: {n} iterations, last {hist[-1]:.3e}")
    n2, hist2, pr, p, b = out[2]
    assert hist2[-1] <= 1e-8 and n2 < maxit, (n2, hist2)
    assert np.all(np.diff(hist2) < 0), hist2
    res = _fp64_residual(pr, p, b)
    print("fp64 residual by the Oracle", res)
    assert res <= 1e-8 * (1 + 1e-6), res
    assert n2 < out[0][0], (n2, out[0][0])


# ---- 7. m = 0 with the machinery present ------------------------------------------------------------------------------------------------
def test_m0_changes_nothing(mg):
    """32 x 32 x 16, four colours and the red-black default: the table, mgx_counters and p after three iterations with the option at 0
    are the same before and after a hierarchy with m = 1 has lived in the process, the table is mgx_level_table's (which knows nothing of
    the option), and "hold_z_fused" stays 0: no held pair, no launch of the held pair's kernel"""
    dims = (32, 32, 16)
    for method in ("FC", "RB"):
        out = []
        for before in (True, False):
            if not before:
                _init(mg, dims, 1, relax_method=method)
                rhs(mg, None, uvw(dims)); mg.solve_p(1e-30, 1)
                assert mg.nhydro.get_option("hold_z_fused") > 0
            _init(mg, dims, 0, relax_method=method)
            rhs(mg, None, uvw(dims))
            c0 = mg.nhydro.counters()
            n, hist = mg.solve_p(1e-30, 3)
            c1 = mg.nhydro.counters()
            out.append((n, hist, mg.grid(1).p, {k: c1[k] - c0[k] for k in c0}, [(mg.grid(l).nx, mg.grid(l).ny, mg.grid(l).nz) for l in range(1, mg.nlevs() + 1)]))
            assert mg.nhydro.get_option("hold_z_fused") == 0
        (n0, h0, p0, c0, z0), (n1, h1, p1, c1, z1) = out
        assert z0 == z1 == [(32, 32, 16), (16, 16, 8), (8, 8, 4), (4, 4, 2)]
        assert z0 == [(l["nx"], l["ny"], l["nz"]) for l in mg.nhydro.level_table(*dims)]
        assert n0 == n1 == 3 and np.array_equal(h0, h1) and np.array_equal(p0, p1)
        assert c0 == c1 and c0["launches"] > 0, (c0, c1)


# ---- 8. compositions -------------------------------------------------------------------------------------------------------------------
def test_process_grid_2x2_bitwise():
    """2 x 2 ranks of 16 x 16 x 16 with m = 1 (four processes, tests/_gpu_hold_z_grid_worker.py), four colours, three iterations: every
    rank's p on every level and b hold the block of the one-rank 32 x 32 x 16 run bit for bit, through the default transport and the hooks"""
    run_process_ranks(os.path.join(HERE, "_gpu_hold_z_grid_worker.py"), 4, (4, 2, 2, free_port(), 16, 16, 16, 8, 1))


def test_periodic_converges_and_rolls(mg):
    """"periodic" = 3 at 32 x 32 x 16 with m = 1: the solve converges to 1e-10, and every input rolled by 16 cells along i (a whole and
    even number of cells on each level) rolls p bit for bit"""
    from test_gpu_periodic import geometry, matrices, velocities_from, velocity_bases
    dims, per, s = (32, 32, 16), 3, 16
    g = geometry(32, 32, per)
    bases = velocity_bases(32, 32, 16, per, 11)

    def run(geo, bas):
        mg.nhydro_clean()
        mg.nhydro.set_option("periodic", per); mg.nhydro.set_option("hold_z_levels", 1)
        mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(relax_method="FC", solver_prec=1e-10))
        assert _nz(mg) == [16, 16, 8, 4]
        matrices(mg, geo, per)
        mg.nhydro.compute_rhs(*velocities_from(bas, per))
        n, hist = mg.solve_p(1e-10, 30)
        return n, hist, mg.grid(1).p[1:-1, 1:-1]
    try:
        n, hist, p = run(g, bases)
        print("periodic = 3, 32 x 32 x 16, m = 1:", n, "iterations", hist)
        assert n < 30 and hist[-1] <= 1e-10 and np.all(np.diff(hist) < 0), hist
        g2 = dict(g)
        for name in ("dx", "dy", "zeta", "h"):
            g2[name] = np.roll(g[name], s, axis=0)
        n2, hist2, p2 = run(g2, tuple(np.roll(b, s, axis=2) for b in bases))
        assert n2 == n and not np.array_equal(p, p2)
        assert np.array_equal(np.roll(p, s, axis=0), p2)
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("periodic", 0); mg.nhydro.set_option("hold_z_levels", 0)


def test_krylov_converges(mg):
    """"krylov" = 4 with m = 1 at 64 x 64 x 16: converges to 1e-10 in no more iterations than the plain solve on the same hierarchy, the fp64
    residual recomputed by the Oracle"""
    dims = (64, 64, 16)
    pr = _init(mg, dims, 1)
    rhs(mg, None, uvw(dims))
    b = mg.grid(1).b
    n0, hist0 = mg.solve_p(1e-10, 30)
    mg.nhydro.set_option("krylov", 4)
    try:
        n, hist = mg.solve_p(1e-10, 30)
        p = mg.grid(1).p
    finally:
        mg.nhydro.set_option("krylov", 0)
    print(f"64 x 64 x 16 m = 1: plain {n0} iterations, krylov = 4 {n}: {hist}")
    assert hist0[-1] <= 1e-10 and hist[-1] <= 1e-10 and n <= n0 < 30
    assert _fp64_residual(pr, p, b) <= 1e-10 * (1 + 1e-6)


def test_update_zeta_device_equals_matrices(mg):
    """mgx_update_zeta_device on an m = 1 hierarchy (32 x 32 x 16): after matrices_device(zeta_a) and a refresh with zeta_b, every field of
    every level equals nhydro_matrices(zeta_b) on a fresh instance, bit for bit; the 2-D zeta chain serves it (it does not depend on nz)"""
    import torch
    from mgroms_amd.testcases import seamount_geometry
    dims = (32, 32, 16)
    dx, dy, _, h = seamount_geometry(32, 32, 1, 1, 0)
    i = np.arange(34, dtype=np.float64)[:, None]; j = np.arange(34, dtype=np.float64)[None, :]
    za = 0.8 * np.sin(2 * np.pi * i / 32) * np.cos(2 * np.pi * j / 32)
    zb = 0.5 * np.cos(2 * np.pi * i / 32 + 1.3) * np.sin(2 * np.pi * j / 32 - 0.4) + 0.05 * np.random.default_rng(3).standard_normal((34, 34))
    names = ("dx", "dy", "zeta", "h", "zr", "zw", "cw", "cA")

    def fresh():
        mg.nhydro_clean()
        mg.nhydro.set_option("hold_z_levels", 1)
        mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(relax_method="FC"))
        assert _nz(mg) == [16, 16, 8, 4]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    try:
        fresh()
        mg.nhydro_matrices(dx, dy, zb, h, None, HC, 0.0, 0.0)
        ref = {(lev, n): mg.grid(lev).get(n) for lev in range(1, mg.nlevs() + 1) for n in names}
        fresh()
        mg.nhydro_matrices_device(dev(dx), dev(dy), dev(za), dev(h), None, HC, 0.0, 0.0)
        mg.nhydro_update_zeta_device(dev(zb))
        for key, a in ref.items():
            assert np.array_equal(mg.grid(key[0]).get(key[1]), a), key
        assert mg.nhydro.get_option("zeta_refreshes") == 1 and mg.nhydro.get_option("zeta_chain_launches") == 1
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("hold_z_levels", 0)


def test_fp32_cycles_refused_with_a_held_pair_only(mg):
    """cycle_precision = 32, krylov_precision = 32 (and mixed_tail with them) are refused with m >= 1, in the words the fp32 cycles use for
    a held pair, and served with m = 0; a change of the option under a live hierarchy is refused in the words of "hold_odd_nz\""""
    from mgroms_amd._lib import MgxError

    def settings():
        yield ("cycle_precision", 32), ()
        yield ("cycle_precision", 32), (("mixed_tail", 1),)
        yield ("krylov_precision", 32), (("krylov", 2),)
    dims = (32, 32, 16)
    try:
        for m, served in ((1, False), (0, True)):
            _init(mg, dims, m)
            rhs(mg, None, uvw(dims))
            for (name, value), extra in settings():
                for k, v in extra:
                    mg.nhydro.set_option(k, v)
                mg.nhydro.set_option(name, value)
                try:
                    n, hist = mg.solve_p(1e-8, 30)
                    assert served and hist[-1] <= 1e-8, (m, name, hist)
                except MgxError as e:
                    assert not served, str(e)
                    assert "holds nz = 16 from level 1 on" in str(e) and "fp32 cycles (cycle_precision = 32, krylov_precision = 32, mixed_tail)" in str(e), str(e)
                finally:
                    mg.nhydro.set_option(name, 64)
                    for k, v in extra:
                        mg.nhydro.set_option(k, 0)
            n, hist = mg.solve_p(1e-8, 30)   # and the hierarchy is usable afterwards
            assert hist[-1] <= 1e-8
            with pytest.raises(MgxError, match="hold_z_levels = %d: the hierarchy in use was built with hold_z_levels = %d" % (1 - m, m)):
                mg.nhydro.set_option("hold_z_levels", 1 - m)
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("hold_z_levels", 0)
