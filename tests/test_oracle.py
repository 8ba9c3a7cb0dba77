"""Pins the CPU oracle (oracle/mgoracle.c) against the reference's own outputs.

Tolerance: the normalised residual ||r||/||b|| is compared with an absolute floor of 1e-14 (the rounding floor
of r = b - A p in units of ||b||: the oracle calls this libm's exp() for the seamount, the reference ran
flang's) plus 1e-13 relative.

Where the reference records no answer, the oracle's matrix, divergence and pressure gradient are held to each other instead (the
operator identity at the end of this file; the rule: tests/_operator_identity.py)."""
import numpy as np
import pytest

from oracle.mgoracle import Oracle, make_seamount


def _close(a, b):
    return abs(a - b) <= 1e-14 + 1e-13 * abs(b)


def test_level_tables():
    # levels and gather decisions (mg_grids.f90:468-577)
    o = Oracle(64, 64, 16)
    assert o.nlevs == 4
    assert [(o.level_info(l)["nx"], o.level_info(l)["nz"]) for l in range(1, 5)] == [(64, 16), (32, 8), (16, 4), (8, 2)]
    o = Oracle(512, 512, 64)
    assert o.nlevs == 6 and o.level_info(6)["nx"] == 16 and o.level_info(6)["nz"] == 2
    o = Oracle(32, 32, 16, 2, 2)
    li = o.level_info(4)
    assert (li["gather"], li["npx"], li["npy"], li["nx"], li["ny"]) == (1, 1, 1, 8, 8)
    assert o.level_info(1, rank=0)["neighb"] == [-1, 1, 2, -1, -1, -1, 3, -1]
    o = Oracle(64, 32, 32, 4, 2)  # 256x64... 4x2 ranks: 2x1 gather on the coarsest level
    assert o.nlevs >= 3


def test_rb_1rank_history_and_scalars(golden):
    g = golden["seamount_64x64x16_RB_1rank"]
    o = make_seamount(64, 64, 16, relax_method="RB", solver_prec=1e-6)
    n, h, bn = o.nhydro_solve()
    assert n == g["nite"] and o.nlevs == g["nlevs"]
    for k, ref in enumerate(g["res"]):
        assert _close(h[k + 1], ref), (k + 1, h[k + 1], ref)
    p = o.field("p")
    assert np.isclose((p[1:-1, 1:-1, :] ** 2).sum(), g["sum_p2"], rtol=1e-12)
    assert np.isclose(bn * bn, g["sum_b2"], rtol=1e-13)
    assert np.isclose(p[1, 1, 0], g["p_1_1_1"], rtol=1e-12)
    assert np.isclose(p[64, 64, 15], g["p_nz_ny_nx"], rtol=1e-11)
    assert np.isclose(p[32, 32, 7], g["p_8_32_32"], rtol=1e-12)
    o.check_nondivergence()
    b = o.field("b")
    assert np.isclose((b[1:-1, 1:-1, :] ** 2).sum(), g["sum_div2_after"], rtol=1e-10)


def test_rb_2x2_reproduces_decomposition_dependence(golden):
    # RB is order dependent at k=1 (mg_relax.f90:271-276): the 2x2 history differs from 1 rank at 2.5e-6
    g = golden["seamount_64x64x16_RB_2x2ranks"]
    o = make_seamount(32, 32, 16, 2, 2, relax_method="RB", solver_prec=1e-6)
    n, h, _ = o.nhydro_solve()
    assert n == g["nite"]
    for k, ref in enumerate(g["res"]):
        assert _close(h[k + 1], ref), (k + 1, h[k + 1], ref)
    one = golden["seamount_64x64x16_RB_1rank"]["res"][0]
    assert abs(h[1] - one) / one > 1e-6


@pytest.mark.parametrize("case,npx", [("seamount_64x64x16_FC_1rank", 1), ("seamount_64x64x16_FC_2x2ranks", 2)])
def test_fc_history(golden, case, npx):
    g = golden[case]
    o = make_seamount(64 // npx, 64 // npx, 16, npx, npx, relax_method="FC", solver_prec=1e-10)
    n, h, _ = o.nhydro_solve()
    assert n == g["nite"]
    for k, ref in g["res_at"].items():
        assert _close(h[int(k)], ref), (k, h[int(k)], ref)


def test_16x16x8_fc_fixture(golden):
    g = golden["seamount_16x16x8_FC_1rank"]
    o = make_seamount(16, 16, 8, relax_method="FC", solver_prec=1e-12)
    n, h, bn = o.nhydro_solve()
    assert n == g["nite"] and o.nlevs == g["nlevs"]
    for k, ref in enumerate(g["res_printed"]):
        assert abs(h[k + 1] - ref) <= 0.006 * ref  # 3 printed digits
    p = o.field("p")
    assert np.isclose((p[1:-1, 1:-1, :] ** 2).sum(), g["sum_p2"], rtol=1e-12)
    assert np.isclose(bn * bn, g["sum_b2"], rtol=1e-13)
    assert np.isclose(p[1, 1, 0], g["p_1_1_1"], rtol=1e-13)
    assert np.isclose(p[16, 16, 7], g["p_8_16_16"], rtol=1e-12)
    assert np.isclose(p[8, 8, 3], g["p_4_8_8"], rtol=1e-13)
    assert np.allclose(o.field("cA")[8, 8, 3, :], g["cA_k4_j8_i8"], rtol=0, atol=6e-9)


def test_operator_is_symmetric_and_consistent():
    # <x, A y> == <A x, y> in the interior (the 8-slot storage is the lower half of a symmetric A)
    o = make_seamount(16, 16, 8, relax_method="FC")
    rng = np.random.default_rng(0)

    def apply(x):
        o.field("p")[...] = 0
        o.field("p")[1:-1, 1:-1, :] = x
        o.fill_halo(1, "p")
        o.field("b")[...] = 0
        o.residual(1)
        return -o.field("r")[1:-1, 1:-1, :].copy()

    # the mirrored (Neumann) halo breaks the symmetry of the boundary rows (own slot 6 vs neighbour slot 8):
    # test on fields supported away from the lateral boundaries
    x, y = np.zeros((16, 16, 8)), np.zeros((16, 16, 8))
    x[2:-2, 2:-2, :] = rng.standard_normal((12, 12, 8))
    y[2:-2, 2:-2, :] = rng.standard_normal((12, 12, 8))
    assert np.isclose((x * apply(y)).sum(), (apply(x) * y).sum(), rtol=1e-10)


@pytest.mark.parametrize("npx,npy,nsmall", [(4, 2, 8), (4, 2, 32), (2, 4, 16)])
def test_fc_is_decomposition_independent_on_4x2(npx, npy, nsmall):
    # the process grid of the 8-GPU configuration (BASELINE configs[4]) with one and with two consecutive gathers:
    # four-colour ordering gives the same iterates as one rank, up to the norm's summation order
    one = make_seamount(64, 64, 16, relax_method="FC", solver_prec=1e-8)
    n1, h1, _ = one.nhydro_solve()
    many = make_seamount(64 // npx, 64 // npy, 16, npx, npy, relax_method="FC", solver_prec=1e-8, nsmall=nsmall)
    assert any(many.level_info(l)["gather"] for l in range(1, many.nlevs + 1))
    n2, h2, _ = many.nhydro_solve()
    assert n1 == n2
    assert np.all(np.abs(h1 - h2) <= 1e-14 + 1e-13 * h1)
    p1 = one.field("p")
    for r in range(npx * npy):
        pi, pj = r % npx, r // npx
        nx, ny = 64 // npx, 64 // npy
        blk = many.field("p", 1, r)[1:-1, 1:-1, :]
        assert np.array_equal(blk, p1[1 + pi * nx:1 + (pi + 1) * nx, 1 + pj * ny:1 + (pj + 1) * ny, :]), r


@pytest.mark.parametrize("npx,npy", [(2, 2), (2, 1)])
def test_fc_is_decomposition_independent_on_a_curvilinear_metric(npx, npy):
    """The same on dx(i,j), dy(i,j) (testcases.curvilinear_metric) from seeded random u, v, w: every rank takes its block of the global
    metric, so the dx, dy halos between ranks and the face averages across a rank boundary carry values that differ from both
    neighbours'; p of every rank is the one-rank p bit for bit, the history within the same bound"""
    from _problem import load_uvw, oracle_twin, problem, uvw
    dims = (32, 32, 8)
    pr = problem(dims, metric="curvilinear", relax_method="FC", solver_prec=1e-8)
    state = uvw(dims, seed=3)
    one, many = oracle_twin(pr), oracle_twin(pr, npx, npy)
    assert np.ptp(one.field("dx")) > 0 and np.ptp(one.field("dy")) > 0
    for o in (one, many):
        load_uvw(o, state)
    n1, h1, _ = one.nhydro_solve()
    n2, h2, _ = many.nhydro_solve()
    assert n1 == n2 and n1 < 30
    assert np.all(np.abs(h1 - h2) <= 1e-14 + 1e-13 * h1)
    p1 = one.field("p")
    nx, ny = 32 // npx, 32 // npy
    for r in range(npx * npy):
        pi, pj = r % npx, r // npx
        blk = many.field("p", 1, r)[1:-1, 1:-1, :]
        assert np.array_equal(blk, p1[1 + pi * nx:1 + (pi + 1) * nx, 1 + pj * ny:1 + (pj + 1) * ny, :]), r


def _bmask_world(nx, ny, nz, npx, npy):
    from _problem import load_uvw, oracle_twin, problem, uvw
    o = oracle_twin(problem((nx * npx, ny * npy, nz), bmask=True, relax_method="FC", solver_prec=1e-8), npx, npy)
    load_uvw(o, uvw((nx * npx, ny * npy, nz)))
    return o


def test_bmask_branch_converges_and_is_decomposition_independent():
    """bmask=.true..  The reference records no known answers for this branch, so the restatement of
    it is NOT pinned (oracle header); what can be checked without the reference: the masked operator
    keeps the multigrid convergence, land columns carry no flux, and the 4-D cA halo exchange + masks give the same
    iterates on 2x2 ranks as on one."""
    one = _bmask_world(32, 32, 8, 1, 1)
    n1, h1, _ = one.nhydro_solve()
    assert n1 < 30 and np.all(h1[1:] < 0.5 * h1[:-1])
    rm = one.field("rmask")
    um = rm[1:, :] * rm[:-1, :]  # umask(j,i) = rmask(j,i-1)*rmask(j,i), i = 1..nx+1
    u = one.field("u")           # [k][j][i-1]
    assert np.all(u[:, um.T == 0] == 0.0)  # no pressure-gradient correction through masked faces
    many = _bmask_world(16, 16, 8, 2, 2)
    n2, h2, _ = many.nhydro_solve()
    assert n1 == n2 and np.all(np.abs(h1 - h2) <= 1e-14 + 1e-13 * h1)
    p1 = one.field("p")
    for r in range(4):
        pi, pj = r % 2, r // 2
        assert np.array_equal(many.field("p", 1, r)[1:-1, 1:-1, :], p1[1 + pi * 16:17 + pi * 16, 1 + pj * 16:17 + pj * 16, :]), r


def test_intergrid_properties_like_the_reference_unit_programs():
    """The checks of the reference's (stale) unit program src/old_tests/mg_testintergrids.f90:84-128, on the oracle:
    restricting a constant gives 8x the constant (fine2coarse sums 8 cells, no 1/8: mg_intergrids.f90:139-162), and the
    tri-linear prolongation reproduces a linear ramp away from the boundaries (weights (27,9,9,9,3,3,3,1)/64)."""
    o = make_seamount(32, 32, 16, relax_method="FC")
    o.field("r", 1)[...] = 2.5
    o.fine2coarse(1)
    assert np.all(o.field("b", 2)[1:-1, 1:-1, :] == 20.0)
    assert np.all(o.field("p", 2) == 0.0)  # p_c = 0 over the whole array (mg_intergrids.f90:70)
    # linear ramp in i, j and k on the coarse grid; cell centres: coarse index c <-> fine indices 2c-1, 2c at +-1/4
    pc = o.field("p", 2)
    nxc, nyc, nzc = pc.shape[0] - 2, pc.shape[1] - 2, pc.shape[2]
    ic, jc, kc = np.meshgrid(np.arange(nxc + 2), np.arange(nyc + 2), np.arange(1, nzc + 1), indexing="ij")
    pc[...] = 3.0 * ic + 5.0 * jc + 7.0 * kc
    o.field("p", 1)[...] = 0.0
    o.coarse2fine(1)
    pf = o.field("p", 1)  # p_f = 0 + interpolant
    i, j, k = np.meshgrid(np.arange(34), np.arange(34), np.arange(1, 17), indexing="ij")
    exact = 3.0 * ((i + 0.5) / 2.0) + 5.0 * ((j + 0.5) / 2.0) + 7.0 * ((k + 0.5) / 2.0)
    inner = (slice(1, 33), slice(1, 33), slice(1, 15))  # k = 2..15: the bottom and top rows use their own weights
    assert np.allclose(pf[inner], exact[inner], rtol=0, atol=1e-12)


def test_halo_fill_carries_the_neighbour_rank_like_mg_testhalo():
    """src/old_tests/mg_testhalo.f90:75-92: fill p with the rank number, fill the halo, every halo plane must hold the
    neighbour's rank (or the own one across a physical boundary: mirror)."""
    o = make_seamount(16, 16, 8, 2, 2, relax_method="FC")
    for r in range(4):
        o.field("p", 1, r)[...] = float(r)
    o.fill_halo(1, "p")
    for r in range(4):
        nb = o.level_info(1, r)["neighb"]  # S, E, N, W, SW, SE, NE, NW
        p = o.field("p", 1, r)             # [i][j][k]
        want = lambda q: float(q if q >= 0 else r)
        assert np.all(p[1:-1, 0, :] == want(nb[0])) and np.all(p[-1, 1:-1, :] == want(nb[1]))
        assert np.all(p[1:-1, -1, :] == want(nb[2])) and np.all(p[0, 1:-1, :] == want(nb[3]))
        assert np.all(p[1:-1, 1:-1, :] == float(r))


def test_galerkin_consistency_probe():
    """testgalerkin (mg_solvers.f90:203-288): <xc, Ac xc> against <I xc, Af I xc> for a smooth coarse field -- the
    rediscretised coarse operator (restriction = plain sum, geometry coarsened by define_matrices) must carry the energy of
    the interpolated field; the reference prints the ratio and expects it near 1."""
    o = make_seamount(32, 32, 16, relax_method="FC")

    def apply(lev, x):
        p = o.field("p", lev); p[...] = 0; p[1:-1, 1:-1, :] = x
        o.fill_halo(lev, "p"); o.field("b", lev)[...] = 0; o.residual(lev)
        return -o.field("r", lev)[1:-1, 1:-1, :].copy()

    i, j, k = np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij")
    xc = np.sin(np.pi * (i + 0.5) / 16) ** 2 * np.sin(np.pi * (j + 0.5) / 16) ** 2 * np.sin(np.pi * (k + 0.5) / 8)
    ec = (xc * apply(2, xc)).sum()
    o.field("p", 2)[...] = 0; o.field("p", 2)[1:-1, 1:-1, :] = xc; o.fill_halo(2, "p")
    o.field("p", 1)[...] = 0
    o.coarse2fine(1)
    xf = o.field("p", 1)[1:-1, 1:-1, :].copy()
    ef = (xf * apply(1, xf)).sum()
    assert ec < 0 and ef < 0            # the operator is negative definite on fields that vanish at the boundary
    assert 0.85 < ef / ec < 1.1, ef / ec


def test_multigrid_solution_equals_a_direct_solve():
    """The reference's Matlab cross-check (matlab/check_real_relaxation.m:30-57,406-409: direct sparse solve vs mgroms p):
    assemble the level-1 operator column by column from the residual routine, solve A p = b densely, compare with solve_p."""
    nx, ny, nz = 16, 16, 8
    o = make_seamount(nx, ny, nz, relax_method="FC", solver_prec=1e-13, solver_maxiter=60)
    o.compute_rhs()
    b = o.field("b")[1:-1, 1:-1, :].copy()
    n = nx * ny * nz
    A = np.zeros((n, n))
    for q in range(n):
        e = np.zeros(n); e[q] = 1.0
        p = o.field("p"); p[...] = 0; p[1:-1, 1:-1, :] = e.reshape(nx, ny, nz)
        o.fill_halo(1, "p"); o.field("b")[...] = 0; o.residual(1)
        A[:, q] = -o.field("r")[1:-1, 1:-1, :].ravel()
    o.field("b")[1:-1, 1:-1, :] = b
    direct = np.linalg.solve(A, b.ravel())
    o.field("p")[...] = 0
    nit, hist, _ = o.solve_p()
    assert hist[-1] < 1e-13
    pm = o.field("p")[1:-1, 1:-1, :].ravel()
    assert np.abs(pm - direct).max() <= 1e-11 * np.abs(direct).max()


def test_call_mask_semantics():
    """The mask of the call (rmaska of nhydro_solve, nhydro.f90:56,72): handing compute_rhs / correct_uvw the mask that
    nhydro_matrices got changes nothing; with bmask off a land mask still removes the w cross terms of compute_rhs
    (mg_compute_rhs.f90:110-111) and leaves umask = vmask = 1 (:69-71)."""
    from _problem import oracle_twin, problem
    nx, ny, nz = 16, 16, 8
    rng = np.random.default_rng(2)
    mask = np.ones((nx + 2, ny + 2)); mask[4:8, 6:11] = 0.0

    def run(bmask, call_mask):
        o = oracle_twin(problem((nx, ny, nz), bmask=bmask, rmask=mask if bmask else None, relax_method="FC", solver_maxiter=3))
        r = np.random.default_rng(7)
        o.field("u")[...] = r.uniform(-1, 1, o.field("u").shape)
        o.field("v")[...] = r.uniform(-1, 1, o.field("v").shape)
        o.field("w")[...] = r.uniform(-1, 1, o.field("w").shape)
        if call_mask is not None:
            o.field("rmaska")[...] = call_mask
            o.use_call_mask(True)
        o.nhydro_solve()
        return o.field("b").copy(), o.field("u").copy(), o.field("w").copy()

    b0, u0, w0 = run(True, None)
    b1, u1, w1 = run(True, mask)
    assert np.array_equal(b0, b1) and np.array_equal(u0, u1) and np.array_equal(w0, w1)
    b2, u2, _ = run(False, None)
    b3, u3, _ = run(False, mask)
    assert not np.array_equal(b2, b3)            # the cross terms saw the land
    b4, _, _ = run(False, np.ones_like(mask))
    assert np.array_equal(b2, b4)                # an all-ones mask is the no-mask case


# ---- genuine reference pin: mg_zr_zw.f90 compiled unmodified (oracle/_ref, `make -C oracle ref`) --------------------------
def _zrzw_cases():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_zrzw.npz"))
    return z, sorted({k.split("/")[0] for k in z.files})


def test_zr_zw_equal_the_reference_compiled_module():
    """Row a13 against the REAL reference: tests/golden/ref_zrzw.npz holds zr, zw written by setup_zr_zw
    (mg_zr_zw.f90:46-215, branch new_s_coord) of the reference compiled unmodified with flang (oracle/Makefile target `ref`,
    driver oracle/ref_driver.f90, generator oracle/make_ref_golden.py) for theta = 0, for theta_s or theta_b alone, and for the
    stretched coordinate (theta_s = 6, theta_b = 0.4, hc = 250) with zeta /= 0 at nz = 4 ... 128.  The oracle's restatement must
    give the same bits on the whole 0:n+1 ring: with theta = 0 there is no libm call at all; with cosh / exp both sides call
    the same glibc functions on the same arguments (the tables depend on k only).  The outer ring (-1, n+2) is filled later by
    fill_halo(nh=2), not by setup_zr_zw, and is not compared."""
    z, names = _zrzw_cases()
    assert len(names) >= 6
    for n in names:
        nx, ny, nz = (int(v) for v in z[n + "/par"][:3])
        hlim, tb, ts = (float(v) for v in z[n + "/par"][3:])
        o = Oracle(nx, ny, nz, 1, 1, relax_method="FC")
        o.field("h")[...] = z[n + "/h"]
        o.field("zeta")[...] = z[n + "/zeta"]
        o.field("dx")[...] = 100.0
        o.field("dy")[...] = 100.0
        o.matrices(hlim, tb, ts)
        ring = (slice(1, -1), slice(1, -1))
        assert np.array_equal(o.field("zr")[ring], z[n + "/zr"][ring]), n
        assert np.array_equal(o.field("zw")[ring], z[n + "/zw"][ring]), n
        assert np.all(z[n + "/zw"][ring][..., -1] == z[n + "/zeta"]), n  # the free surface is the last interface
        o.close()


# ---- the operator identity: matrix, divergence and pressure gradient against each other (tests/_operator_identity.py) -------
# name: (nx, ny, nz), geometry, island mask, stretched sigma + rough zeta, bmask
_IDENTITY_CASES = {
    "seamount-16x16x8": ((16, 16, 8), "seamount", False, False, False),
    "rndtopo-24x20x12": ((24, 20, 12), "rndtopo", False, False, False),
    "seamount-island-32x32x8": ((32, 32, 8), "seamount", True, False, True),
    "rndtopo-island-stretched-24x20x12": ((24, 20, 12), "rndtopo", True, True, True),
    "seamount-32x32x24": ((32, 32, 24), "seamount", False, False, False),   # levels of 24, 12, 6, 3 rows
    "call-mask-32x32x8": ((32, 32, 8), "seamount", True, False, False),     # bmask = 0: the island is handed to the calls only
    # the name's prefix: dx, dy times testcases.curvilinear_metric, a metric that varies in i and in j
    "curvilinear-rndtopo-island-stretched-24x20x12": ((24, 20, 12), "rndtopo", True, True, True),
}
_DIRECT_TOL = 1.1e-14   # 16 x 6.7e-16 (test_identity_direct_form)


def _identity_world(name):
    from _operator_identity import case_inputs, make_oracle, water_interior, assert_set_is_meaningful
    (nx, ny, nz), geom, mask, stretched, bmask = _IDENTITY_CASES[name]
    inp = case_inputs(nx, ny, geom, mask, stretched, curvilinear=name.startswith("curvilinear-"))
    o = make_oracle(nx, ny, nz, inp, bmask=bmask)
    sel = water_interior(inp["rmask"], nx, ny)
    assert_set_is_meaningful(sel, inp["rmask"])
    return o, inp, sel


def _apply_A(o, x):
    """A x on the interior: residual(1) with b = 0 and the halo of p filled"""
    o.field("p")[...] = 0
    o.field("p")[1:-1, 1:-1, :] = x
    o.fill_halo(1, "p")
    o.field("b")[...] = 0
    o.residual(1)
    return -o.field("r")[1:-1, 1:-1, :].copy()


@pytest.mark.parametrize("name", list(_IDENTITY_CASES))
def test_identity_direct_form(name):
    """compute_rhs(correct_uvw(u = v = w = 0; p)) = -A p for a random p (zero on the land of bmask) on the water-interior set: the matrix
    (define_matrices), the divergence and the pressure gradient are three texts of the restatement, and on those columns they are one
    operator.  No reference answer enters: this is what pins bmask, the per-call mask, the stretched coordinate with a rough zeta,
    rndtopo and a vertical size that is no power of two, for which the reference records nothing.

    Measured max|lhs - rhs| / max|A p| on the set (this seed; eight seeds stay below 6.7e-16):
        seamount-16x16x8 3.5e-16   rndtopo-24x20x12 5.4e-16   seamount-island-32x32x8 3.7e-16
        rndtopo-island-stretched-24x20x12 6.7e-16   seamount-32x32x24 5.3e-16   call-mask-32x32x8 3.7e-16
        curvilinear-rndtopo-island-stretched-24x20x12 (dx(i,j), dy(i,j): testcases.curvilinear_metric) 3.6e-16
    Bound: 16 x the largest = 1.1e-14, the margin for other seeds and summation lengths.  Outside the set the same figure is
    5e-4 (seamount), 2e-5 (rndtopo), 9e-4 (island coast), 9e-7 (stretched rndtopo): the reference's own inconsistency.

    call-mask: with bmask = 0 the matrix and correct_uvw see no land (umask = vmask = 1) while compute_rhs drops the w cross terms of
    uf, vf on the land of the call's mask (mg_compute_rhs.f90:110-111).  By design the identity is then broken on the columns with such a
    column in their neighbourhood -- by 1e-2 of max|A p| at the worst coast column -- and holds on the set built from the CALL's mask,
    which is what is asserted; that the coast does break is asserted too, so that the mask is known to have been read."""
    from _operator_identity import scaled_defect, water_interior
    o, inp, sel = _identity_world(name)
    (nx, ny, nz), _, _, _, bmask = _IDENTITY_CASES[name]
    x = np.random.default_rng(0).standard_normal((nx, ny, nz))
    if bmask:
        x *= inp["rmask"][1:-1, 1:-1, None]
    Ap = _apply_A(o, x)                  # leaves p = x with its halo filled
    for f in ("u", "v", "w"):
        o.field(f)[...] = 0.0
    if inp["rmask"] is not None and not bmask:
        o.field("rmaska")[...] = inp["rmask"]
        o.use_call_mask(True)
    o.correct_uvw()
    o.compute_rhs()
    b = o.field("b")[1:-1, 1:-1, :].copy()
    d = scaled_defect(b, -Ap, sel)
    outside = np.abs(b + Ap).max(axis=2)[~sel].max() / np.abs(Ap).max()
    print(name, "set: %.1f %% of the columns, defect %.3e, outside the set %.3e" % (100 * sel.mean(), d, outside))
    assert d <= _DIRECT_TOL, (name, d)
    if name.startswith("call-mask"):
        coast = water_interior(None, nx, ny) & ~sel
        assert scaled_defect(b, -Ap, coast) > 1000 * _DIRECT_TOL   # measured: 2.8e-2
    o.close()


@pytest.mark.parametrize("name", ["seamount-island-32x32x8", "rndtopo-island-stretched-24x20x12"])
def test_masked_operator_is_symmetric_and_negative(name):
    """<x, A y> = <A x, y> within 1e-12 relative and <x, A x> < 0 for fields supported on the water-interior set, with bmask
    (measured: 4e-16 and 8e-16 relative).  The unmasked test above covers 16x16x8 only."""
    from _operator_identity import inner
    o, inp, sel = _identity_world(name)
    (nx, ny, nz) = _IDENTITY_CASES[name][0]
    rng = np.random.default_rng(100)
    x, y = (rng.standard_normal((nx, ny, nz)) * sel[:, :, None] for _ in range(2))
    Ax, Ay = _apply_A(o, x), _apply_A(o, y)
    xAy, Axy = inner(x, Ay), inner(Ax, y)
    print(name, "symmetry %.3e relative" % (abs(xAy - Axy) / abs(xAy)), "<x, A x> =", inner(x, Ax))
    assert abs(xAy - Axy) <= 1e-12 * abs(xAy)
    assert inner(x, Ax) < 0 and inner(y, Ay) < 0
    o.close()


def _coupling_cases():
    from _operator_identity import CASES
    return CASES


@pytest.mark.parametrize("case", _coupling_cases(), ids=[c.name for c in _coupling_cases()])
def test_identity_through_the_model_calls(case):
    """The form the GPU is held to (tests/test_gpu_operator_identity.py), on the oracle: nhydro_solve with two iterations, then
    b' = compute_rhs(u', v', w') against r = b - A p*.  The figures behind COUPLING_TOL come from this test's output."""
    from _operator_identity import oracle_coupling_defect, COUPLING_TOL
    f = oracle_coupling_defect(case)
    print(case.name, f)
    assert f["Ap_over_b"] > 1e-3
    assert f["defect"] <= COUPLING_TOL, (case.name, f)


# ---- the smoother identities: every smoother against its level's operator (tests/_smoother_identity.py) ---------------------
def _smoother_cases():
    from _smoother_identity import oracle_cases
    return oracle_cases()


@pytest.mark.parametrize("case", _smoother_cases(), ids=[c.name for c in _smoother_cases()])
def test_smoother_identities_on_the_oracle(case):
    """The three identities of tests/_smoother_identity.py and their controls on every level of the case, eight seeds: the fixed point
    (every method), the first colour as a complete solve and the last colour without a residual (four colours, red-black).  This is
    where the bounds asserted on the GPU were measured (16 x the maxima: _smoother_identity.TOL).  Largest defect per check over every
    case, level and seed, as printed here:

        check 1  1.21e-13    check 2  9.54e-14    check 3  5.95e-14   (island-32x32x96 and -32x32x128, level 1; every other case
                                                                       stays below 8.1e-15, 6.8e-15, 3.3e-15)
        four colours real / simple at most 8.1e-15 / 6.8e-15 / 3.3e-15 without the island; red-black real 1.3e-15 / 1.5e-15 / 1.4e-15
        without it; red-black simple 1.2e-15 / 1.3e-15 / 6.4e-16; Gauss-Seidel 1.7e-15 (check 1)

    and the smallest control: check 2 with delta on the last colour 1.3e-2 (rndtopo-island-stretched-24x16x12, its 6x4x3 level), the
    other colours' residual in check 3 0.13 (RB-simple-32x32x24), row k = 1 of red-black 'real' 1.8e-4 (32x512x16, its 4x64x2 level).
    The first two are asserted at three times their thresholds; the third cannot be (see _smoother_identity.py: on a level four columns wide the
    inner columns lie at the summit, where the bottom row's diagonals vanish with the slope) and is asserted at the threshold."""
    import _smoother_identity as S
    from _problem import oracle_twin
    o = oracle_twin(S.case_problem(case))
    be = S.OracleBackend(o)
    worst, least = {}, {}
    for lev in range(1, o.nlevs + 1):
        for seed in S.SEEDS:
            f = S.run_level(be, lev, case.method, case.cmatrix == "real", seed)
            S.assert_level(f, (case.name, lev, seed))
            for k in ("c1", "c2", "c3"):
                if f[k] is not None:
                    worst[k] = max(worst.get(k, 0.0), f[k])
            for k in ("k2", "k3", "row1"):
                if f[k] is not None:
                    least[k] = min(least.get(k, np.inf), f[k])
    print(case.name, "largest", {k: "%.2e" % v for k, v in worst.items()}, "smallest control", {k: "%.2e" % v for k, v in least.items()})
    # the recorded maxima still describe this build (a factor 2: another libm's last bits in the geometry move them a little)
    assert worst["c1"] <= S.MEASURED[1] * 2
    if case.method != "GS":
        assert worst["c2"] <= S.MEASURED[2] * 2 and worst["c3"] <= S.MEASURED[3] * 2
        assert least["k2"] >= 3 * S.CONTROL_2 and least["k3"] >= 3 * S.CONTROL_3, least
    o.close()


def test_smoother_identity_bounds_are_sixteen_times_the_measured():
    import _smoother_identity as S
    for k in (1, 2, 3):
        assert abs(S.TOL[k] / S.MEASURED[k] - 16.0) < 0.1
    assert abs(S.ADJOINT_TOL / 1.4e-17 - 16.0) < 0.5 and S.ADJOINT_MEASURED <= 1.4e-17


def test_smoother_identity_sees_a_wrong_term():
    """the checks can fail: one off-column slot of the oracle's level-2 matrix scaled by 1 + 1e-6 BETWEEN forming b = A p* and relaxing
    (the smoother then solves another operator than the residual's) moves the fixed point by far more than the bound"""
    import _smoother_identity as S
    from _problem import oracle_twin
    case = next(c for c in S.CASES if c.name == "FC-real-32x32x8")
    o = oracle_twin(S.case_problem(case))

    class Skewed(S.OracleBackend):
        def relax(self, lev, n):
            cA = self.o.field("cA", lev)
            keep = cA.copy()
            cA[..., 6] *= 1.0 + 1e-6
            self.o.relax(lev, n)
            cA[...] = keep

    assert S.fixed_point(S.OracleBackend(o), 2, 0) <= S.TOL[1]
    d = S.fixed_point(Skewed(o), 2, 0)
    print("fixed point with slot 7 of the smoother off by 1e-6: %.2e" % d)
    assert d > 1000 * S.TOL[1]
    o.close()


def test_nearest_transfers_are_adjoint_on_the_oracle():
    """<R r, q> = <r, P q> for fine2coarse and the nearest coarse2fine on every level pair with an even fine nz (measured: at most
    7.3e-18 of ||r|| ||P q||, sums in longdouble), and NOT on the pair 16x16x5 -> 8x8x2 of 64x64x20 (measured 0.16 .. 0.24): the
    reference leaves the top row of an odd fine level out of both transfers, its own known inconsistency.  The held pairs of option
    "hold_odd_nz" have no oracle: their reference, the numpy transfers of tests/_hold_ref.py, keeps the identity to 1.4e-17."""
    import _smoother_identity as S
    from _hold_ref import mirror, prolong_held, restrict_held
    from _operator_identity import inner
    from _problem import oracle_twin, problem
    worst = 0.0
    for dims in S.ADJOINT_DIMS + [S.ODD_PAIR_DIMS]:
        o = oracle_twin(problem(dims, relax_method="FC", interp_type="nearest"))
        be = S.OracleBackend(o)
        odd = [lev for lev in range(1, o.nlevs) if lev not in S.even_fine_pairs(be)]
        assert bool(odd) == (dims == S.ODD_PAIR_DIMS)
        for lev in range(1, o.nlevs):
            ds = [S.adjoint_defect(be, lev, seed) for seed in S.SEEDS]
            print(dims, be.dims(lev), "->", be.dims(lev + 1), "%.2e .. %.2e" % (min(ds), max(ds)))
            if lev in odd:
                assert min(ds) > S.ODD_PAIR, (dims, lev, ds)
            else:
                assert max(ds) <= S.ADJOINT_TOL, (dims, lev, ds)
                worst = max(worst, max(ds))
        o.close()
    assert worst <= S.ADJOINT_MEASURED * 2
    held = 0.0
    for nx, ny, nz in ((4, 4, 5), (8, 8, 5), (16, 16, 5)):
        for seed in S.SEEDS:
            rng = np.random.default_rng([5, nx, seed])
            r = np.zeros((nx + 2, ny + 2, nz)); r[1:-1, 1:-1] = rng.standard_normal((nx, ny, nz))
            q = np.zeros((nx // 2 + 2, ny // 2 + 2, nz)); q[1:-1, 1:-1] = rng.standard_normal((nx // 2, ny // 2, nz))
            Rr, Pq = restrict_held(r)[1:-1, 1:-1], prolong_held(mirror(q.copy()), linear=False)[1:-1, 1:-1]
            held = max(held, abs(inner(Rr, q[1:-1, 1:-1]) - inner(r[1:-1, 1:-1], Pq)) / np.sqrt(inner(r, r) * inner(Pq, Pq)))
    print("held pairs of tests/_hold_ref.py: %.2e" % held)
    assert held <= S.ADJOINT_TOL
