"""The three passes of option "krylov" (mgx_krylov.hip: k_kr_apply[_mf] + k_kr_reduce, k_kr_ortho, k_kr_update), each run alone through the
test hook mgx_krylov_op -- the wrappers, buffers, view and stream of solve_p_krylov -- against a plain reference (tests/_krylov_kernel_ref.py:
numpy on the host arrays and the CPU oracle's residual).  Nothing the GPU computed enters an expected value.  Three kinds of comparison:
  exact      q = A z against the oracle's -r (the kernel's stated contract); one-hot inner products; passes 2 and 3 on integer fields, where
             every summation order gives the same bits (the helper asserts the 2^53 condition per case);
  derived    dense inner products against math.fsum within Higham's bound for the kernel's own summation tree (apply_chain / stream_chain);
  eps_ref    nowhere in this file (tests/test_gpu_krylov.py holds the solver-level comparisons).
pytest -s prints, per shape and variant, the launch taken: matrix-free or stored operator, cmatrix real or simple, stream, gy & 7, gx.
The shapes and the paths they are there for: the comment above SHAPES in tests/_krylov_kernel_ref.py."""
import math

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import gpu_problem, oracle_twin
from tests import _krylov_kernel_ref as K

pytestmark = pytest.mark.gpu

# coefficient variants: (name, shapes).  'simple' -> k_kr_apply<false> at nz = 2 and k_kr_apply_mf<false> above; 'bmask' and 'userA' -> the stored
# operator at nz >= 3; 'stretched' -> the matrix-free operator on a stretched grid with a moving free surface
VARIANTS = [("real", K.SMALL_SHAPES), ("simple", [(4, 4, 2), (24, 40, 8), (32, 32, 24)]), ("bmask", [(64, 64, 16)]),
            ("userA", [(32, 32, 16)]), ("stretched", [(32, 32, 16)])]
CASES = [pytest.param(sh, v, id=f"{sh[0]}x{sh[1]}x{sh[2]}-{v}") for v, shapes in VARIANTS for sh in shapes]
SMALL = [pytest.param(sh, id=f"{sh[0]}x{sh[1]}x{sh[2]}") for sh in K.SMALL_SHAPES]


mg = gpu_module()


_now = {}


def _setup(mg, shape, variant="real"):
    """level 1 of `shape` on the GPU and in the oracle with the same coefficients -> the oracle (kept while shape and variant stay)"""
    if _now.get("key") == (shape, variant):
        return _now["o"]
    _now.clear()
    nx, ny, nz = shape
    kw = dict(relax_method="FC", cmatrix="simple" if variant == "simple" else "real")
    if variant == "stretched":
        kw.update(zeta=0.3 * np.cos(np.arange(nx + 2))[:, None] * np.ones((1, ny + 2)), sigma=(250.0, 0.4, 6.0))
    o = oracle_twin(gpu_problem(mg, shape, bmask=variant == "bmask", **kw))
    g = mg.grid(1)
    if variant == "stretched":
        # device cosh / exp differ from the host's in the last bit (test_stretched_sigma_coordinates): the operator is checked on the
        # coefficients the GPU built, which the oracle takes over
        o.field("cA")[...] = g.get("cA")
    if variant == "userA":   # a user matrix through set_field: the library falls back to the stored slots
        cA = g.get("cA")
        cA[..., 2] *= 1.5; cA[..., 5] *= 1.5
        g.set("cA", cA); o.field("cA")[...] = cA
    _now.update(key=(shape, variant), o=o)
    return o


def _z(o, shape, seed):
    """a random z whose physical halo is the oracle's fill_halo of its interior"""
    nx, ny, nz = shape
    o.field("p")[...] = np.random.default_rng(seed).standard_normal((nx + 2, ny + 2, nz))
    o.fill_halo(1, "p")
    return o.field("p").copy()


def _show(shape, variant, path):
    print(f"\n  {shape} {variant}: operator {'matrix-free' if path['mf'] else 'stored'}, REAL {path['real']}, stream {path['stream']}, "
          f"gy & 7 = {path['gy'] & 7} (gy {path['gy']}), gx {path['gx']}")


def _check_path(shape, variant, path):
    """the launch the shape list promises"""
    nx, ny, nz = shape
    st, gx, gy = K.expected_path(nx, ny, nz)
    assert (path["stream"], path["gx"], path["gy"]) == (st, gx, gy), (path, shape)
    assert path["real"] == (0 if variant == "simple" else 1), path
    assert path["mf"] == (1 if variant in ("real", "simple", "stretched") and nz >= 3 else 0), path


def check_apply(mg, o, shape, variant):
    """q = A z of pass 1 on interior cells: bit for bit the negative of the oracle's residual(1) for b = 0, and of the library's own"""
    z = _z(o, shape, 11)
    q = np.full_like(z, np.nan)
    _, path = mg.nhydro.krylov_op("apply", [z, q], nd=0)
    _show(shape, variant, path)
    _check_path(shape, variant, path)
    qref = K.ref_apply(o, z)
    assert np.array_equal(K.interior(q), K.interior(qref)), float(np.nanmax(np.abs(K.interior(q) - K.interior(qref))))
    g = mg.grid(1)
    g.set("p", z); g.set("b", np.zeros_like(z))
    mg.compute_residual(1)
    assert np.array_equal(K.interior(q), -K.interior(g.get("r")))
    return z, qref


def check_onehot(mg, shape, z, qref, chunks=None):
    """(q, q_n) for one-hot q_n = 2^n at a listed cell is q[cell] 2^n exactly: every other product is a zero.  A one-hot in the halo gives 0."""
    nx, ny, nz = shape
    cells = K.onehot_cells(nx, ny, nz)
    assert all(K.is_interior(c, nx, ny, nz) for c in cells)
    groups = [cells[a:a + 8] for a in range(0, len(cells), 8)][:chunks]
    for grp in groups:
        fs, ws = K.onehot_fields(grp, shape)
        q = np.empty_like(z)
        sc, _ = mg.nhydro.krylov_op("apply", [z, q] + fs, nd=len(grp), nout=len(grp))
        want = np.array([qref[i, j, k - 1] * w for (i, j, k), w in zip(grp, ws)])
        assert np.all(want != 0.0)
        assert np.array_equal(sc, want), (grp, sc, want)
    probes = K.halo_probes(nx, ny, nz)
    assert not any(K.is_interior(c, nx, ny, nz) for c in probes)
    fs, _ = K.onehot_fields(probes, shape)
    q = np.empty_like(z)
    sc, _ = mg.nhydro.krylov_op("apply", [z, q] + fs, nd=8, nout=8)
    assert np.array_equal(sc, np.zeros(8)), sc


def check_ortho(mg, shape, nd, rotated):
    slot = K.rotated_slots(nd) if rotated else None
    c = K.ortho_case(shape, nd, seed=100 + nd, slot=slot)
    zr, qr, s, t = K.ref_ortho(c["z"], c["q"], c["r"], c["zi"], c["qi"], c["sc"], c["qq"], c["slot"])
    K.check_exact([zr, qr, c["r"]] + c["zi"] + c["qi"], [(qr, qr), (c["r"], qr)])
    z, q = c["z"].copy(), c["q"].copy()
    fields = [z, q, c["r"]] + [a for pair in zip(c["zi"], c["qi"]) for a in pair]
    out, _ = mg.nhydro.krylov_op("ortho", fields, nd=nd, slot=slot, sin=c["sc"] + c["qq"])
    assert (out[0], out[1]) == (s, t), (out, s, t)
    assert np.array_equal(q, qr) and np.array_equal(z, zr)   # whole arrays, halo included


def check_update(mg, shape, s, t, head=0):
    c = K.update_case(shape, seed=7, s=s, t=t)
    pr, rr, norm, qn = K.ref_update(c["p"], c["r"], c["z"], c["q"], s, t)
    K.check_exact([pr, rr], [(rr, rr)], unit=min(1.0, abs(t / s)))
    p, r = c["p"].copy(), c["r"].copy()
    out, _ = mg.nhydro.krylov_op("update", [p, r, c["z"], c["q"]], nd=head, sin=[s, t])
    assert out[0] == norm and out[1] == qn, (out, norm, qn)
    assert norm > 0
    assert np.array_equal(p, pr) and np.array_equal(r, rr)


# ---- pass 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", CASES)
def test_apply_is_minus_the_residual_and_onehot_products(mg, shape, variant):
    o = _setup(mg, shape, variant)
    z, qref = check_apply(mg, o, shape, variant)
    check_onehot(mg, shape, z, qref)


@pytest.mark.parametrize("nd", [1, 3, 8])
@pytest.mark.parametrize("shape", SMALL)
def test_apply_inner_products_within_the_summation_bound(mg, shape, nd):
    """dense q_n against math.fsum.  Bound (not measured): |computed - exact| <= gamma_n sum |q q_n| (Higham, Accuracy and Stability of
    Numerical Algorithms, (3.5): any summation order, n - 1 = the longest chain of additions an operand goes through, + 1 for the rounding
    of its product).  The chain of pass 1, from mgx_krylov.hip: nz sequential additions per lane (PUT_ROW, one column per lane), 6 shuffle
    steps and 3 additions across the 4 waves (kr_block_sums), ceil(nblk / 256) sequential and 8 tree steps in k_kr_reduce, nblk = 2 gx gy
    (apply_chain).  q itself is exact (the previous test), so the products are those of the reference."""
    o = _setup(mg, shape, "real")
    z = _z(o, shape, 12)
    qref = K.ref_apply(o, z)
    rng = np.random.default_rng(13)
    qi = [rng.standard_normal(z.shape) for _ in range(nd)]   # halo cells filled too: they must not enter
    q = np.empty_like(z)
    sc, _ = mg.nhydro.krylov_op("apply", [z, q] + qi, nd=nd, nout=nd)
    n = K.apply_chain(*shape) + 1
    for k in range(nd):
        exact, w = K.dot_fsum(qref, qi[k]), K.abs_dot(qref, qi[k])
        print(f"\n  {shape} nd={nd} (q, q_{k}): error {abs(sc[k] - exact):.3e}, bound {K.gamma(n) * w:.3e} (n = {n})", end="")
        assert abs(sc[k] - exact) <= K.gamma(n) * w, (k, sc[k], exact, K.gamma(n) * w)


# ---- pass 2 ------------------------------------------------------------------------------------------------------------------
ORTHO = [pytest.param(sh, nd, rot, id=f"{sh[0]}x{sh[1]}x{sh[2]}-nd{nd}-{'rotated' if rot else 'in-order'}")
         for sh in K.SMALL_SHAPES for nd in K.NDS + (5,) for rot in ((False, True) if nd else (False,))]


@pytest.mark.parametrize("shape,nd,rotated", ORTHO)
def test_ortho_exact_on_integer_fields(mg, shape, nd, rotated):
    """integer fields, integer betas: z, q (whole arrays), (q, q) and (r, q) equal the numpy result bit for bit.  Halo cells of r, q, q_n hold
    +-2^40: one of them entering a sum shows.  rotated: slot[] as after the head of the ring of nd + 1 has wrapped (nd = 8 included: the
    ring of m + 1 = 9), every ring slot with another (q_n, q_n): a wrong slot gives another beta (a power of two times the right one)"""
    _setup(mg, shape, "real")
    check_ortho(mg, shape, nd, rotated)


# ---- pass 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", [(4.0, 2.0), (2.0, 8.0), (8.0, -8.0)], ids=["alpha=1/2", "alpha=4", "alpha=-1"])
@pytest.mark.parametrize("shape", SMALL)
def test_update_exact_on_integer_fields(mg, shape, st):
    _setup(mg, shape, "real")
    check_update(mg, shape, *st, head=(0 if st[0] == 4.0 else 3))


GUARD = [(0.0, 1.0), (-4.0, 1.0), (math.inf, 1.0), (4.0, math.nan), (4.0, math.inf)]


@pytest.mark.parametrize("shape", [(24, 40, 8), (30, 18, 2)], ids=["24x40x8", "30x18x2"])
def test_update_guard(mg, shape):
    """scalars that allow no step: p and r bitwise untouched, out = -1, s still filed under the new pair's slot; with {4, 2} the step is taken"""
    _setup(mg, shape, "real")
    for s, t in GUARD:
        c = K.update_case(shape, seed=8, s=s, t=t)
        p, r = c["p"].copy(), c["r"].copy()
        out, _ = mg.nhydro.krylov_op("update", [p, r, c["z"], c["q"]], nd=2, sin=[s, t])
        assert out[0] == -1.0, (s, t, out)
        assert out[1] == s or (math.isnan(s) and math.isnan(out[1])), (s, t, out)
        assert np.array_equal(p, c["p"]) and np.array_equal(r, c["r"]), (s, t)
    check_update(mg, shape, 4.0, 2.0, head=2)


# ---- the streaming variants: everything above at the two sizes beyond the cache threshold ----------------------------------------------------
@pytest.mark.parametrize("shape", [pytest.param(sh, id=f"{sh[0]}x{sh[1]}x{sh[2]}") for sh in K.BIG_SHAPES])
def test_streaming_sizes(mg, shape):
    """stream = 1 (non-temporal loads and stores in all three passes): apply against the oracle and the library's residual, one launch of
    one-hot products and the halo probes, the integer cases of passes 2 and 3 for every nd, the guard"""
    o = _setup(mg, shape, "real")
    z, qref = check_apply(mg, o, shape, "real")
    check_onehot(mg, shape, z, qref, chunks=1)
    del z, qref
    for nd in K.NDS:
        check_ortho(mg, shape, nd, rotated=nd in (3, 8))
    check_update(mg, shape, 4.0, 2.0, head=4)
    c = K.update_case(shape, seed=8)
    for s, t in ((0.0, 1.0), (4.0, math.nan)):
        p, r = c["p"].copy(), c["r"].copy()
        out, _ = mg.nhydro.krylov_op("update", [p, r, c["z"], c["q"]], nd=1, sin=[s, t])
        assert out[0] == -1.0 and out[1] == s
        assert np.array_equal(p, c["p"]) and np.array_equal(r, c["r"])
    _now.clear()


# ---- the passes put together ---------------------------------------------------------------------------------------------------------
def test_one_gcr_iteration_from_the_three_passes(mg):
    """64x64x16 four colours: the first iteration of tests/_krylov_ref.gcr on the seamount right-hand side, its inner products summed with
    math.fsum and recorded, against the same iteration put together from the three hook calls: z = the oracle's preconditioner
    (bit-identical to the GPU's for four colours), apply, ortho (no pair yet), update.
    Bounds (derived, g = gamma_n of passes 2 and 3, stream_chain: 8 additions per lane, 6 + 3 in the workgroup, ceil(nblk / 256) + 8 in
    k_kr_reduce, + 1 for the product): |s - s_ref| <= g S, |t - t_ref| <= g T with S, T the sums of absolute products (+ one rounding of
    fsum's result).  alpha = t / s then differs from the reference's by at most d = (ds + dt) / (1 - ds) relatively (+ one rounding), and
    r' = r - alpha q moves by |d alpha| q, whose norm is at most d ||r|| (alpha q is the projection of r on q): ||r'||^2 differs by at
    most 2 d ||r'|| ||r|| + d^2 ||r||^2, plus the summation bound g ||r'||^2; p = alpha z differs by d relatively."""
    from oracle.mgoracle import make_seamount
    from tests._krylov_ref import gcr, dot_fsum
    shape = (64, 64, 16)
    o = _setup(mg, shape, "real")
    rec = []

    def dot(x, y):
        rec.append((dot_fsum(x, y), math.fsum(np.abs(x * y).ravel())))
        return rec[-1][0]
    o2 = make_seamount(*shape, relax_method="FC"); o2.compute_rhs()
    b0 = o2.field("b").copy()
    n, href, _ = gcr(o2, 4, 1e-30, 1, dot=dot)
    assert n == 1
    (bb, _), (r0, _), (s_ref, S), (t_ref, T), (rr_ref, _) = rec[:5]
    p_ref = o2.field("p").copy()
    # the same iteration from the passes: residual and preconditioner by the oracle, as gcr() forms them
    o.field("b")[...] = b0; o.field("p")[...] = 0.0; o.residual(1)
    res = o.field("r").copy()
    o.field("b")[...] = res; o.field("p")[...] = 0.0; o.residual(1); o.fcycle()
    z = o.field("p").copy()
    q = np.empty_like(z)
    mg.nhydro.krylov_op("apply", [z, q], nd=0)
    qref = K.ref_apply(o, z)
    assert np.array_equal(K.interior(q), K.interior(qref))
    q = qref   # (pass 1 leaves the halo of q alone; the reference's goes on)
    z2, q2 = z.copy(), q.copy()
    (s, t), _ = mg.nhydro.krylov_op("ortho", [z2, q2, res], nd=0, sin=[0.0] * 17)
    assert np.array_equal(z2, z) and np.array_equal(q2, q)
    g = K.gamma(K.stream_chain(*shape) + 1)
    print(f"\n  s {s:.16e}: off the reference's by {abs(s - s_ref):.3e} (bound {g * S + K.U * s_ref:.3e}); "
          f"t {t:.16e}: off by {abs(t - t_ref):.3e} (bound {g * T + K.U * abs(t_ref):.3e})")
    assert abs(s - s_ref) <= g * S + K.U * s_ref
    assert abs(t - t_ref) <= g * T + K.U * abs(t_ref)
    p, r = np.zeros_like(z), res.copy()
    (rr, qn), _ = mg.nhydro.krylov_op("update", [p, r, z, q], nd=0, sin=[s, t])
    assert qn == s
    ds, dt = g * S / s_ref + K.U, g * T / abs(t_ref) + K.U
    d = (ds + dt) / (1.0 - ds) + 2 * K.U
    tol = 2 * d * math.sqrt(rr_ref * r0) + d * d * r0 + (g + 4 * K.U) * rr_ref
    print(f"  ||r'||^2 {rr:.16e}: off the reference's by {abs(rr - rr_ref):.3e} (bound {tol:.3e}); "
          f"history entry {math.sqrt(rr / bb):.6e}, reference {math.sqrt(rr_ref / bb):.6e}")
    assert abs(rr - rr_ref) <= tol
    assert np.abs(p - p_ref).max() <= (d + 2 * K.U) * np.abs(p_ref).max()


def test_refusals(mg):
    from mgroms_amd._lib import MgxError
    from mgroms_amd.testcases import seamount_geometry
    nx, ny, nz = 8, 8, 4
    a = np.zeros((nx + 2, ny + 2, nz))
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, mg.nhydro.default_params(relax_method="FC"))
    _now.clear()
    with pytest.raises(MgxError, match="mgx_matrices"):
        mg.nhydro.krylov_op("apply", [a, a.copy()], nd=0)
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    with pytest.raises(MgxError, match="unknown pass"):
        mg.nhydro.krylov_op("axpy", [a, a.copy()], nd=0)
    for bad in (-1, 9):
        with pytest.raises(MgxError, match="nd = "):
            mg.nhydro.krylov_op("apply", [a, a.copy()], nd=bad)
    with pytest.raises(MgxError, match="slot"):
        mg.nhydro.krylov_op("ortho", [a.copy() for _ in range(7)], nd=2, slot=[1, 1], sin=[1.0] * 17)
    mg.nhydro.krylov_op("apply", [a, a.copy()], nd=0)
    # a process grid larger than 1 x 1: refused on sight (no transport, no matrix is needed to ask)
    mg.nhydro_init(nx, ny, nz, 2, 1, 0, mg.nhydro.default_params(relax_method="FC"))
    with pytest.raises(MgxError, match="single rank"):
        mg.nhydro.krylov_op("apply", [a, a.copy()], nd=0)
    mg.nhydro_clean()
