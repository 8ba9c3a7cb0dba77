"""Option "krylov_precision" = 32: the Krylov loop of option "krylov" (truncated GCR, solve_p_krylov) around the fp32 F-cycle of option
"cycle_precision" = 32, with the two conversions folded into passes the loop runs anyway (mgx_krylov.hip: k_kr_apply32[_mf], k_kr_update32).

Kernel by kernel through the hook mgx_krylov_op ("apply32", "update32"): the expected values are numpy's (one fp32 -> fp64 promotion and one
multiplication; one multiplication and one rounding to fp32) and the results of the fp64 passes "apply" / "update" on the same input, all
bit for bit.  Solver level: the returned residual against the CPU oracle's fp64 residual of the returned p (the tolerance of
tests/test_gpu_mixed_precision.py), the iteration count against the reference GCR over the oracle (tests/_krylov_ref.py) + 2 (the margin
that file gives fp32 refinement over fp64), the counters, and the launches of a steady-state iteration against a hand count."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, on_gpu, oracle_relative_residual, oracle_twin, problem, rhs, uvw
from tests import _krylov_kernel_ref as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OPTIONS = ("krylov", "krylov_precision", "cycle_precision", "warm_start", "rb_exact")


mg = gpu_module(krylov=0, krylov_precision=64)


_restore_options = restore_options(*OPTIONS)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
# The shapes of tests/_krylov_kernel_ref.py (every launch path of pass 1 and of the streaming passes), and two where the fp32 layout differs
# from the fp64 one in kind: ny = 24 (half-rows of 12 columns: the fp32 odd half-row starts at 64, the fp64 one at 32) and ny = 72 (the
# fp32 half-row offset rounds 68 up to 96, the fp64 one 52 up to 64; rows of 160 floats against 112 doubles)
LAYOUT_SHAPES = [(16, 24, 4), (8, 72, 4)]
VARIANTS = [("real", K.SMALL_SHAPES + LAYOUT_SHAPES), ("simple", [(4, 4, 2), (24, 40, 8), (32, 32, 24)]), ("bmask", [(64, 64, 16)]),
            ("userA", [(32, 32, 16)])]
CASES = [pytest.param(sh, v, id=f"{sh[0]}x{sh[1]}x{sh[2]}-{v}") for v, shapes in VARIANTS for sh in shapes]
UPDATE_SHAPES = [pytest.param(sh, id=f"{sh[0]}x{sh[1]}x{sh[2]}") for sh in K.SMALL_SHAPES + LAYOUT_SHAPES + [(256, 256, 64)]]
_now = {}


def _setup(mg, shape, variant="real"):
    """level 1 of `shape` on the GPU (kept while shape and variant stay); no oracle: the references here are numpy and the fp64 passes"""
    if _now.get("key") == (shape, variant):
        return
    gpu_problem(mg, shape, bmask=variant == "bmask", relax_method="FC", cmatrix="simple" if variant == "simple" else "real")
    if variant == "userA":   # a user matrix through set_field: the stored-slot operator at nz >= 3
        g = mg.grid(1)
        cA = g.get("cA")
        cA[..., 2] *= 1.5; cA[..., 5] *= 1.5
        g.set("cA", cA)
    _now.clear()
    _now["key"] = (shape, variant)


def _fp32_field(rng, shape, halo=None):
    """random values fp32 holds exactly, halo cells included (halo: +-halo there instead)"""
    nx, ny, nz = shape
    a = rng.standard_normal((nx + 2, ny + 2, nz)).astype(np.float32).astype(np.float64)
    if halo is not None:
        keep = K.interior(a).copy()
        a[...] = np.where(rng.integers(0, 2, size=a.shape) > 0, halo, -halo)
        K.interior(a)[...] = keep
    return a


def check_apply32(mg, shape, variant, nd, inv_sigma, halo=None, seed=21):
    rng = np.random.default_rng(seed)
    e = _fp32_field(rng, shape, halo)
    qi = [K.int_field(rng, shape, K.HALO) for _ in range(nd)]   # +-2^40 in the halo cells: one of them entering a product shows
    z, q = np.zeros_like(e), np.full_like(e, np.nan)
    sc, path = mg.nhydro.krylov_op("apply32", [e, z, q] + qi, nd=nd, sin=[inv_sigma], nout=nd)
    zref = np.float32(e).astype(np.float64) * inv_sigma
    assert np.array_equal(z, zref), int((z != zref).sum())          # the whole array, halo images included
    q64 = np.full_like(e, np.nan)
    sc64, path64 = mg.nhydro.krylov_op("apply", [zref, q64] + qi, nd=nd, nout=nd)
    assert path == path64
    assert np.isfinite(K.interior(q64)).all() and np.abs(K.interior(q64)).max() > 0
    assert np.array_equal(K.interior(q), K.interior(q64)), float(np.abs(K.interior(q) - K.interior(q64)).max())
    assert np.array_equal(sc, sc64), (sc, sc64)
    return path


@pytest.mark.parametrize("shape,variant", CASES)
def test_apply32_is_the_promotion_followed_by_apply(mg, shape, variant):
    """z = (double)e / sigma over the whole array and q = A z, (q, q_n) as the fp64 pass gives them for that z, bit for bit; with no
    retained pair, with three, and with 2^40 in the halo cells of e (and of the q_n) for eight"""
    _setup(mg, shape, variant)
    nx, ny, nz = shape
    path = check_apply32(mg, shape, variant, 0, 1.0 / 3.0)
    print(f"\n  {shape} {variant}: operator {'matrix-free' if path['mf'] else 'stored'}, REAL {path['real']}, stream {path['stream']}, gx {path['gx']}, gy {path['gy']}")
    assert path["mf"] == (1 if variant in ("real", "simple") and nz >= 3 else 0) and path["real"] == (0 if variant == "simple" else 1)
    assert (path["stream"], path["gx"], path["gy"]) == K.expected_path(nx, ny, nz)
    check_apply32(mg, shape, variant, 3, 7.25e-3, seed=22)
    check_apply32(mg, shape, variant, 8, 1.0 / 3.0, halo=K.HALO, seed=23)


def test_apply32_streaming(mg):
    """256x256x64: the non-temporal variant, gx = 2, gy = 64 (first branch of the block map)"""
    shape = (256, 256, 64)
    _setup(mg, shape)
    path = check_apply32(mg, shape, "real", 1, 1.0 / 3.0, halo=K.HALO)
    assert path["stream"] == 1 and path["mf"] == 1
    _now.clear()


def check_update32(mg, shape, s, t, sigma, head=0, seed=7):
    c = K.update_case(shape, seed=seed, s=s, t=t)
    f0 = _fp32_field(np.random.default_rng(seed + 1), shape)
    p64, r64 = c["p"].copy(), c["r"].copy()
    out64, _ = mg.nhydro.krylov_op("update", [p64, r64, c["z"], c["q"]], nd=head, sin=[s, t])
    p, r, f = c["p"].copy(), c["r"].copy(), f0.copy()
    out, _ = mg.nhydro.krylov_op("update32", [p, r, c["z"], c["q"], f], nd=head, sin=[s, t, sigma])
    assert np.array_equal(out, out64) or (math.isnan(out[1]) and math.isnan(out64[1]) and out[0] == out64[0]), (out, out64)
    assert np.array_equal(p, p64) and np.array_equal(r, r64)
    if K.step_ok(s, t):
        pr, rr, norm, _ = K.ref_update(c["p"], c["r"], c["z"], c["q"], s, t)
        K.check_exact([pr, rr], [(rr, rr)], unit=min(1.0, abs(t / s)))
        assert out[0] == norm and np.array_equal(r, rr)
        want = np.float32(rr * sigma).astype(np.float64)
        assert np.array_equal(K.interior(f), K.interior(want)), int((K.interior(f) != K.interior(want)).sum())
    else:
        assert out[0] == -1.0
        assert np.array_equal(p, c["p"]) and np.array_equal(r, c["r"]) and np.array_equal(f, f0), (s, t)


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_update32_is_update_and_the_demotion(mg, shape):
    """integer fields (every summation order gives the same bits): p, r and sout as the fp64 pass on the same input, f = (float)(sigma r_new)
    on every interior cell; s = 0: p, r and f untouched, sout[0] = -1.  sigma = 1/3: sigma r needs a rounding in fp64 and another to fp32."""
    _setup(mg, shape)
    check_update32(mg, shape, 4.0, 2.0, 1.0 / 3.0)
    check_update32(mg, shape, 2.0, 8.0, 0.0123, head=3)
    check_update32(mg, shape, 0.0, 1.0, 1.0 / 3.0, head=2)
    if shape == (24, 40, 8):
        for s, t in ((-4.0, 1.0), (math.inf, 1.0), (4.0, math.nan)):
            check_update32(mg, shape, s, t, 0.5, head=1)
    if shape[0] == 256:
        _now.clear()


def test_update32_dense(mg):
    """dense random fields: r against numpy's r - (t / s) q (one multiplication, one subtraction per cell: no summation), f against its demotion"""
    shape = (24, 40, 8)
    _setup(mg, shape)
    rng = np.random.default_rng(31)
    p, r, z, q = (rng.standard_normal((shape[0] + 2, shape[1] + 2, shape[2])) for _ in range(4))
    f = np.zeros_like(p)
    s, t, sigma = 3.0, 1.7, 1.0 / 0.83
    want_r = r - (t / s) * q
    mg.nhydro.krylov_op("update32", [p, r, z, q, f], nd=0, sin=[s, t, sigma])
    assert np.array_equal(r, want_r)
    assert np.array_equal(K.interior(f), K.interior(np.float32(want_r * sigma).astype(np.float64)))


# ---- solves ------------------------------------------------------------------------------------------------------------------------
def _case(nx, ny, nz, meth, bmask=False, **par):
    """the record of a seamount case (bmask: with the island mask): what _gpu() hands to the GPU and the reference's oracle is made from"""
    return problem((nx, ny, nz), bmask=bmask, **dict(dict(relax_method=meth, solver_prec=1e-8, solver_maxiter=50), **par))


def _gpu(mg, pr):
    on_gpu(mg, pr)
    rhs(mg, None, uvw(pr.dims))
    _now.clear()


_refs = {}


def _reference(dims, meth, bmask, cmatrix, tol):
    """iterations of the reference GCR (fp64, over the oracle, m = 4), the oracle and the record it was made from, computed once per case"""
    from tests._krylov_ref import gcr
    key = (dims, meth, bmask, cmatrix, tol)
    if key not in _refs:
        pr = _case(*dims, meth, bmask=bmask, **({"cmatrix": cmatrix} if cmatrix else {}))
        o = oracle_twin(pr)
        rhs(None, o, uvw(dims))
        nref, href, _ = gcr(o, 4, tol, 50)
        _refs[key] = (nref, href, o, pr)
    return _refs[key]


SOLVES = [((64, 64, 16), "FC", False, None, 1e-8), ((64, 64, 16), "RB", False, None, 1e-8), ((128, 128, 32), "RB", False, None, 1e-8),
          ((64, 64, 16), "FC", True, None, 1e-8), ((64, 64, 16), "FC", False, "simple", 1e-8), ((32, 32, 48), "FC", False, None, 1e-8),
          ((64, 64, 16), "FC", False, None, 1e-12)]


def _solve_id(c):
    dims, meth, bmask, cm, tol = c
    return f"{dims[0]}x{dims[1]}x{dims[2]}-{meth}" + ("-bmask" if bmask else "") + (f"-{cm}" if cm else "") + f"-{tol:g}"


@pytest.mark.parametrize("case", SOLVES, ids=_solve_id)
def test_solve(mg, case):
    """one rank, the seamount, cold start, m = 4 with fp32 cycles: (a) the returned residual is below tol and is the oracle's fp64 residual of
    the returned p (1e-9 relative, the comparison of tests/test_gpu_mixed_precision.py); (b) at most the reference GCR's count + 2;
    (c) every iteration counted under krylov_mixed_iterations, none under mixed_iterations"""
    dims, meth, bmask, cm, tol = case
    nref, href, o, pr = _reference(dims, meth, bmask, cm, tol)
    _gpu(mg, pr)
    assert np.array_equal(mg.grid(1).b, o.field("b"))
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("krylov_precision", 32)
    before = mg.nhydro.get_option("krylov_mixed_iterations"), mg.nhydro.get_option("mixed_iterations")
    n, hist = mg.solve_p(tol, 50)
    ro = oracle_relative_residual(o, mg.grid(1).p)
    print(f"\n{_solve_id(case)}: fp32-cycle GCR {n} it -> {hist[-1]:.3e} (oracle's residual of p {ro:.3e}), reference GCR {nref} it -> {href[-1]:.3e}, "
          f"restarts {mg.nhydro.get_option('krylov_restarts')}\n  " + " ".join(f"{v:.2e}" for v in hist))
    assert hist[-1] <= tol, hist
    assert abs(ro - hist[-1]) <= 1e-9 * hist[-1], (ro, hist[-1])
    assert n <= nref + 2, (n, nref)
    assert mg.nhydro.get_option("krylov_mixed_iterations") == before[0] + n
    assert mg.nhydro.get_option("mixed_iterations") == before[1]
    assert mg.nhydro.get_option("cycle_precision") == 64


def _cycle32_launches(mg, meth):
    """launches of one fp32 F-cycle, from fcycle32 / vcycle32 / relax32 of mgx_cycle.cpp: a sweep is 4 colour launches (four colours) or 2
    colours with a snapshot each (red-black, cmatrix = 'real'); a V-cycle from level l over d = nlevs - l levels is the leading
    prolongation, d x (ns_pre sweeps + the fused residual-restriction), ns_coarsest sweeps, d x (prolongation + ns_post sweeps); the
    F-cycle is nlevs - 1 restrictions, ns_coarsest sweeps and the V-cycles from nlevs - 1 down to 1"""
    nl = mg.nlevs()
    pre, post, nc = (mg.nhydro.get_option(k) for k in ("ns_pre", "ns_post", "ns_coarsest"))
    sweep = 4   # four colours: 4 colour launches; red-black with cmatrix = 'real': 2 x (snapshot + colour)
    assert meth in ("FC", "RB")
    v = lambda d: 1 + d * (sweep * pre + 1) + sweep * nc + d * (1 + sweep * post)
    return (nl - 1) + sweep * nc + sum(v(nl - l) for l in range(1, nl))


@pytest.mark.parametrize("meth", ["FC", "RB"])
def test_steady_state_iteration_has_no_conversion_launch(mg, meth):
    """64x64x16: the launches of iteration 4 (three retained pairs, no restart) = a solve of 4 iterations minus one of 3.  Hand count: the
    cycle + pass 1 and the reduction of its inner products (2) + pass 2 and its reduction (2) + pass 3 and its reduction (2); e = 0 is a
    memset, not a launch.  fp32: the cycle as counted above and nothing else -- no k_to32, no k_to64.  fp64: the fp64 F-cycle, measured as
    the launches of one mgx_fcycle."""
    _gpu(mg, _case(64, 64, 16, meth))
    mg.nhydro.set_option("krylov", 4)
    cnt = lambda: mg.nhydro.counters()["launches"]
    diff = {}
    for prec in (32, 64):
        mg.nhydro.set_option("krylov_precision", prec)
        mg.solve_p(1e-30, 1)   # allocations and the coefficient conversion happen here
        per = []
        for maxite in (3, 4):
            c0 = cnt(); n, _ = mg.solve_p(1e-30, maxite); per.append(cnt() - c0)
            assert n == maxite and mg.nhydro.get_option("krylov_restarts") == 0
        diff[prec] = per[1] - per[0]
    c0 = cnt(); mg.Fcycle(); fcycle64 = cnt() - c0
    hand32 = _cycle32_launches(mg, meth)
    print(f"\n64x64x16 {meth}: launches of a steady-state iteration: fp32 cycles {diff[32]} (cycle by hand {hand32} + 6), fp64 cycles {diff[64]} (cycle {fcycle64} + 6)")
    assert diff[32] == hand32 + 6, (diff, hand32)
    assert diff[64] == fcycle64 + 6, (diff, fcycle64)


def test_restart_refills_f(mg):
    """64x64x16 four colours, m = 8, tol 1e-14, 20 iterations: the recurrence drifts, the loop restarts from the true residual.  The returned
    residual is an independent compute_residual(1); after the first restart the history goes on falling (f of the shadow refilled from the
    new r: with the old f the cycle would answer a residual the loop no longer has)"""
    import ctypes as C
    from mgroms_amd._lib import lib
    _gpu(mg, _case(64, 64, 16, "FC"))
    mg.nhydro.set_option("krylov", 8)
    mg.nhydro.set_option("krylov_precision", 32)
    n, res, hist = C.c_int(), C.c_double(), (C.c_double * 21)()
    assert lib().mgx_solve_p(1e-14, 20, C.byref(n), C.byref(res), hist) == 0
    h = np.array(hist[:n.value + 1])
    b = mg.grid(1).b
    true = mg.compute_residual(1) / np.sqrt(np.sum(b[1:-1, 1:-1, :] ** 2))
    restarts = mg.nhydro.get_option("krylov_restarts")
    print(f"\n64x64x16 FC m=8 fp32 cycles: {n.value} it, res {res.value:.3e}, independent {true:.3e}, restarts {restarts}\n  " + " ".join(f"{v:.2e}" for v in h))
    assert abs(res.value - true) <= 1e-12 * true and abs(h[-1] - true) <= 1e-12 * true
    assert restarts >= 1
    assert n.value == 20 or res.value <= 1e-14
    # A restart shows in the history as its only kind of rise: the entry where the true residual replaced the drifted recurrence's word (GCR's
    # own norms never rise).  The iteration after the FIRST restart must fall below that true residual.  (Later ones sit at the round-off
    # floor of b - A p in fp64, about 5e-14 ||b|| here, where another restart follows each iteration and nothing can fall further.)
    up = np.nonzero(np.diff(h) > 0)[0]
    assert len(up) >= 1 and up[0] + 2 <= n.value, h
    k = up[0] + 1
    assert np.all(np.diff(h[:k]) < 0) and h[k + 1] < h[k], h


# ---- refusals, the inert case ------------------------------------------------------------------------------------------------------------
def test_other_values_refused(mg):
    from mgroms_amd._lib import MgxError
    for bad in (48, 0, 16, -32):
        with pytest.raises(MgxError, match="krylov_precision"):
            mg.nhydro.set_option("krylov_precision", bad)
    assert mg.nhydro.get_option("krylov_precision") == 64
    with pytest.raises(MgxError, match="unknown option"):
        mg.nhydro.set_option("krylov_mixed_iterations", 1)


@pytest.mark.parametrize("how", ["GS", "rb_exact"])
def test_unsupported_combinations_refused(mg, how):
    from mgroms_amd._lib import MgxError
    _gpu(mg, _case(32, 32, 8, "GS" if how == "GS" else "RB"))
    if how == "rb_exact":
        mg.nhydro.set_option("rb_exact", 1)
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("krylov_precision", 32)
    with pytest.raises(MgxError, match="relax_method = 'GS'" if how == "GS" else "rb_exact"):
        mg.solve_p(1e-8, 10)
    mg.nhydro.set_option("krylov_precision", 64)
    n, hist = mg.solve_p(1e-8, 20)
    assert hist[-1] <= 1e-8


def test_refused_on_a_process_grid():
    """2x2 thread-ranks (the set-up of tests/_gpu_thread_ranks.py): every rank refuses in the words of mixed_check, before any collective"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_krylov_mixed_ranks.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(out) == 4 and all("single rank" in e and "2 x 2" in e for e in out), out


@pytest.mark.parametrize("meth", ["FC", "RB"])
def test_inert_without_krylov(mg, meth):
    """krylov = 0: solve_p with krylov_precision = 32 gives the history and p of the default, bit for bit, and counts nothing"""
    _gpu(mg, _case(64, 64, 16, meth))
    n0, h0 = mg.solve_p(1e-8, 50)
    p0 = mg.grid(1).p
    mg.nhydro.set_option("krylov_precision", 32)
    n1, h1 = mg.solve_p(1e-8, 50)
    assert n1 == n0 and np.array_equal(h1, h0) and np.array_equal(mg.grid(1).p, p0)
    assert mg.nhydro.get_option("krylov_mixed_iterations") == 0 and mg.nhydro.get_option("mixed_iterations") == 0


def test_option_survives_clean_init_and_the_old_refusal_stays(mg):
    from mgroms_amd._lib import MgxError
    _gpu(mg, _case(32, 32, 8, "FC"))
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("krylov_precision", 32)
    n, hist = mg.solve_p(1e-8, 20)
    assert hist[-1] <= 1e-8 and mg.nhydro.get_option("krylov_mixed_iterations") == n
    mg.nhydro_clean()
    _gpu(mg, _case(32, 32, 8, "FC"))
    assert mg.nhydro.get_option("krylov_precision") == 32
    assert mg.nhydro.get_option("krylov_mixed_iterations") == 0
    mg.nhydro.set_option("cycle_precision", 32)
    with pytest.raises(MgxError, match=r"krylov.*cycle_precision"):
        mg.solve_p(1e-8, 10)
