"""The operator identity on the GPU, with no oracle call in any assertion: the level-1 matrix (mgx_setup.hip; the matrix-free forms of
mgx_operator.h and k_residual_mf), the divergence (compute_rhs: k_rhs_uf / vf / wf, k_rhs_accum_m) and the pressure-gradient correction
(k_correct_uvw_m) are separate texts, and every other GPU test holds them to the CPU oracle, which was written from the same reading of
the reference.  Here they are held to EACH OTHER, through the model-facing calls alone (tests/_operator_identity.py: coupling_defect):

    nhydro_solve(u, v, w[, rmask]) with solver_maxiter = 2       -> p* and u' = u - G p* (the identity is linear in p*: any p* /= 0 serves)
    compute_rhs(u, v, w), compute_residual(1)                    -> b and r = b - A p*
    compute_rhs(u', v', w')                                      -> b'

On the water-interior set (not the outermost ring of the domain, 3 x 3 neighbourhood all water) b' must equal r in units of
max(|b|, |A p*|).  A wrong coefficient, slot, sign, metric factor or index in any of the three texts shows at O(1) (1e-6 relative in
one slot of cA: test_a_perturbed_slot_is_seen).

TOL.  The same sequence on the CPU oracle (OracleBackend; tests/test_oracle.py::test_identity_through_the_model_calls prints the
cases of the list), with the seeds used here, gives

    seamount-32x16x8-stored 3.3e-16       seamount-64x32x64 7.1e-16 (either path)    seamount-32x32x24 6.3e-16
    island-32x32x96 1.1e-15               rndtopo-island-stretched-24x16x12 9.7e-16  call-mask-32x32x8 3.4e-16
    zeta refresh 32x32x16: 2.2e-15 before, 1.6e-15 after                             the unperturbed case of the slot test 3.9e-16
    run layouts: 16x16x2 3.5e-16, 64x64x16 6.5e-16, 256x512x96 6.7e-16, 512x512x48 5.1e-16, 512x512x64 6.9e-16
    on the curvilinear metric (dx(i,j), dy(i,j): testcases.curvilinear_metric)
    seamount-32x16x8-stored 3.4e-16       seamount-64x32x64 6.1e-16                  seamount-32x32x24 4.5e-16
    island-32x32x96 1.0e-15               rndtopo-island-stretched-24x16x12 1.4e-15

and TOL = 16 x the largest of them = 16 x 2.2e-15 = 3.5e-14 (COUPLING_TOL).  The margin is for other seeds and nothing else: b, r
and b' are reduction-free fields which the GPU computes in the oracle's operation order without FMA contraction, bit for bit where
the coordinate has no transcendental function (tests/test_gpu_model_coupling.py), and to the last bits of cosh / exp where it has.
Measured on the MI355X: the same digits in every case with theta = 0; 1.3e-15 (24x16x12) and 1.3e-15 / 1.9e-15 (zeta refresh) with the
stretched coordinate."""
import numpy as np
import pytest

from _gpu import gpu_module
from _operator_identity import CASES, COUPLING_TOL as TOL, MIN_FRACTION, case_inputs, coupling_defect, water_interior, assert_set_is_meaningful, inner

pytestmark = pytest.mark.gpu

SYM_TOL = 1e-12      # <x, A y> = <A x, y>, relative, sums in longdouble
HC = 4e3


mg = gpu_module()


class _Gpu:
    """coupling_defect's three calls on the library"""

    def __init__(self, mg):
        self.mg = mg

    def solve(self, u, v, w, rmask):
        self.mg.nhydro_solve(u, v, w, rmask)

    def rhs(self, u, v, w, rmask):
        self.mg.nhydro.compute_rhs(u, v, w, rmask)
        return self.mg.grid(1).b[1:-1, 1:-1, :]

    def residual(self):
        self.mg.compute_residual(1)
        return self.mg.grid(1).r[1:-1, 1:-1, :]


def _init(mg, dims, bmask, monkeypatch=None, stored=False, maxiter=2):
    if monkeypatch is not None:
        if stored:
            monkeypatch.setenv("MGX_NO_MF", "1")   # read by every nhydro_init: the stored slots instead of the in-kernel coefficients
        else:
            monkeypatch.delenv("MGX_NO_MF", raising=False)
    mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(relax_method="FC", solver_prec=1e-30, solver_maxiter=maxiter,
                                                            bmask=1 if bmask else 0))


def _check(mg, dims, rmask, seed, what):
    f = coupling_defect(_Gpu(mg), *dims, rmask, seed)
    print(what, dims, f)
    # p* is there, and A p* is as large as b: the identity is linear in p*, so how far the solve got does not matter
    assert np.abs(mg.grid(1).p).max() > 0 and f["Ap_over_b"] > 1e-3, (what, f)
    return f["defect"]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_identity(mg, case, monkeypatch):
    """b' = r on the water-interior set, every case within TOL (module docstring).  call-mask: bmask = 0, so the matrix and correct_uvw
    see no land, and compute_rhs drops the w cross terms on the land of the call's mask (mg_compute_rhs.f90:110-111): by design the
    identity then holds on the set built from the CALL's mask and fails at its coast (measured on the oracle: 1e-2 of max|A p|)."""
    inp = case_inputs(*case.dims[:2], case.geom, case.mask, case.stretched, case.curvilinear)
    bmask = case.mask and not case.call_mask
    _init(mg, case.dims, bmask, monkeypatch, case.stored)
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], inp["rmask"] if bmask else None, inp["hc"], inp["theta_b"], inp["theta_s"])
    d = _check(mg, case.dims, inp["rmask"], 1, case.name)
    assert d <= TOL, (case.name, d)


def test_24x20x12_is_refused(mg):
    """Why the stretched rndtopo case runs at 24 x 16 x 12 here and at 24 x 20 x 12 on the oracle only: the library serves no hierarchy
    with an odd nx or ny on any level (the reference's stated assumptions), and says so."""
    from mgroms_amd._lib import MgxError
    with pytest.raises(MgxError, match="level 3 has local size 6x5x3: odd sizes are not supported"):
        mg.nhydro_init(24, 20, 12, 1, 1, 0, mg.nhydro.default_params(relax_method="FC"))


def test_identity_after_a_zeta_refresh(mg, monkeypatch):
    """nhydro_matrices_device, then nhydro_update_zeta_device with another free surface, stretched coordinate, bmask: everything zeta
    reaches was rebuilt -- the matrix of every level, the slopes, and the model-space zw, dzw, cw, zxdy, zydx that compute_rhs and
    correct_uvw read -- so the identity holds after the refresh as it does before.  A piece left at the old zeta (0.3 m against
    depths of metres) would show at 1e-2."""
    import torch
    dims = (32, 32, 16)
    inp = case_inputs(32, 32, "rndtopo", mask=True, stretched=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _init(mg, dims, True, monkeypatch)
    mg.nhydro_matrices_device(*(dev(inp[n]) for n in ("dx", "dy", "zeta", "h", "rmask")), inp["hc"], inp["theta_b"], inp["theta_s"])
    d = _check(mg, dims, inp["rmask"], 2, "before")
    assert d <= TOL, ("before the refresh", d)
    zeta2 = 0.3 * np.random.default_rng(100).standard_normal((34, 34))
    mg.nhydro_update_zeta_device(dev(zeta2))
    assert mg.nhydro.get_option("zeta_refreshes") == 1
    assert np.array_equal(mg.grid(1).zeta[1:-1, 1:-1], zeta2[1:-1, 1:-1])
    d = _check(mg, dims, inp["rmask"], 3, "after")
    assert d <= TOL, ("after the refresh", d)


# ---- every run layout of the model kernels -------------------------------------------------------------------------------------
def _layout_class(dims):
    """what distinguishes the run layouts test_shape_list_covers_every_run_layout guards: per kernel, one run / equal runs / a shorter
    last run, and the run length where it is above the heuristic's floor of eight rows"""
    from test_gpu_model_coupling import _layout
    lay = _layout(*dims)

    def cls(r):
        return ("one" if len(r) == 1 else "equal" if len(set(r)) == 1 else "ragged", r[0] if r[0] > 8 else "floor")
    return tuple(cls(lay[k]) for k in ("uf", "vf", "wf", "correct_uvw")) + (lay["accum_kr"] >= 8,)


_WIDER = {(8, 16, 2): (16, 16, 2)}   # the list's only one-run shape keeps 66 % of its columns inside the ring: the same layout on 16 x 16


def _layout_shapes():
    """the smallest shape of each layout class in the list of tests/test_gpu_model_coupling.py on which the water-interior set holds its
    70 % of the columns (62 x 6 does not: its class is served by 64 x 64 x 16)"""
    from test_gpu_model_coupling import SHAPES
    best = {}
    for dims, _, _ in SHAPES:
        key = _layout_class(dims)
        dims = _WIDER.get(dims, dims)
        assert _layout_class(dims) == key
        if water_interior(None, *dims[:2]).mean() < MIN_FRACTION:
            continue
        if key not in best or np.prod(dims) < np.prod(best[key]):
            best[key] = dims
    assert len(best) == len({_layout_class(d) for d, _, _ in SHAPES})   # no class was lost to the 70 % rule
    return sorted(best.values())


@pytest.mark.parametrize("dims", _layout_shapes(), ids=["%dx%dx%d" % d for d in _layout_shapes()])
def test_identity_run_layouts(mg, dims, monkeypatch):
    """compute_rhs and correct_uvw climb the columns in runs of rows whose count depends on the plane's size; a run start that reloaded
    the wrong row, or a lane tail left out, breaks b' = r in the rows or columns it touches.  The seamount at every shape: the layout
    does not depend on the geometry, and the random topography at 512 x 512 (20 m cells under depth jumps of hundreds of metres: fluxes
    1e4 times their divergence, a diverging F-cycle) lets the oracle itself keep the identity to 5.8e-12 only, too blunt a bound."""
    inp = case_inputs(*dims[:2], "seamount")
    _init(mg, dims, False, monkeypatch)
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], None, HC, 0.0, 0.0)
    d = _check(mg, dims, None, 4, "layout")
    assert d <= TOL, (dims, d)


# ---- symmetry and sign of the GPU operator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["bmask-stored", "matrix-free"])
def test_gpu_operator_is_symmetric_and_negative(mg, masked, monkeypatch):
    """A through compute_residual(1) with b = 0, on fields supported on the water-interior set (and zero on land): <x, A y> = <A x, y>
    within 1e-12 relative and <x, A x> < 0, inner products in longdouble.  The eight stored slots are the lower half of a symmetric
    matrix; the boundary rows (own slot against the mirrored halo) are not symmetric, hence the set."""
    dims = (32, 32, 16)
    inp = case_inputs(32, 32, "rndtopo", mask=masked, stretched=True)
    _init(mg, dims, masked, monkeypatch)
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], inp["rmask"], inp["hc"], inp["theta_b"], inp["theta_s"])
    sel = water_interior(inp["rmask"], 32, 32)
    assert_set_is_meaningful(sel, inp["rmask"])
    g = mg.grid(1)

    def apply(x):
        p = np.zeros(g._shape("p")); p[1:-1, 1:-1, :] = x
        g.set("p", p); mg.fill_halo(1, "p"); g.set("b", np.zeros(g._shape("b")))
        mg.compute_residual(1)
        return -g.r[1:-1, 1:-1, :]

    rng = np.random.default_rng(5)
    x, y = (rng.standard_normal(dims) * sel[:, :, None] for _ in range(2))
    Ax, Ay = apply(x), apply(y)
    xAy, Axy = inner(x, Ay), inner(Ax, y)
    print("xAy", xAy, "Axy", Axy, "rel", abs(xAy - Axy) / abs(xAy), "xAx", inner(x, Ax), "yAy", inner(y, Ay))
    assert abs(xAy - Axy) <= SYM_TOL * abs(xAy)
    assert inner(x, Ax) < 0 and inner(y, Ay) < 0


# ---- the proof that the identity can fail --------------------------------------------------------------------------------------------
def test_a_perturbed_slot_is_seen(mg, monkeypatch):
    """One slot of the level-1 cA scaled by 1 + 1e-6 on the whole level (grid(1).set("cA", ...): the smoother and the residual then
    read the stored slots): the matrix no longer matches the divergence of the gradient and the defect must exceed 1000 x TOL --
    for each of the eight slots in turn.  With cA restored the identity holds again.  (On the oracle the eight perturbed defects are
    4.7e-8 ... 1.3e-6, i.e. 1e6 ... 4e7 x TOL.)"""
    dims = (32, 32, 16)
    inp = case_inputs(32, 32, "seamount")
    _init(mg, dims, False, monkeypatch)
    mg.nhydro_matrices(inp["dx"], inp["dy"], inp["zeta"], inp["h"], None, HC, 0.0, 0.0)
    g = mg.grid(1)
    cA = g.get("cA")
    assert _check(mg, dims, None, 6, "untouched") <= TOL
    for slot in range(8):
        bad = cA.copy()
        bad[..., slot] *= 1.0 + 1e-6
        g.set("cA", bad)
        d = _check(mg, dims, None, 6, "slot %d" % (slot + 1))
        assert d > 1000 * TOL, (slot, d)
    g.set("cA", cA)
    assert _check(mg, dims, None, 6, "restored") <= TOL
