"""Option "krylov" = m: solve_p as truncated GCR / Orthomin(m) around the F-cycle (mgx_krylov.hip, solve_p_krylov).

The reference is the numpy GCR over the CPU oracle (tests/_krylov_ref.py).  Histories are compared within 10 x eps_ref, eps_ref being
the reference's own sensitivity to the order of its sums on the SAME case, measured in the test (the margin of 10 covers the GPU's
other reduction tree).  Iteration counts must equal the reference's (four colours: the cycle is bit-identical) or lie within one of it
(red-black default: the cycle matches the oracle to 1e-10), and must beat plain solve_p's count on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import on_gpu, oracle_twin, problem, rhs, uvw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
mg = gpu_module(krylov=0)


_restore_options = restore_options("krylov", "cycle_precision", "warm_start")


def _case(nx, ny, nz, meth, bmask=False, **par):
    """the record of a seamount case (bmask: with the island mask): what _gpu() hands to the GPU and _oracle() to the oracle"""
    return problem((nx, ny, nz), bmask=bmask, **dict(dict(relax_method=meth, solver_prec=1e-10, solver_maxiter=50), **par))


def _gpu(mg, pr):
    on_gpu(mg, pr)
    rhs(mg, None, uvw(pr.dims))


def _oracle(pr):
    o = oracle_twin(pr)
    rhs(None, o, uvw(pr.dims))
    return o


def _solve(mg, m, tol, maxite=50):
    mg.nhydro.set_option("krylov", m)
    n, hist = mg.solve_p(tol, maxite)
    return n, hist


def _ratio(hist, href, floor):
    from tests._krylov_ref import history_noise
    return history_noise(hist, href, floor)


def test_history_follows_the_reference_gcr(mg):
    """64x64x16 four colours, m = 8, to 1e-10: entry by entry within 10 x eps_ref of the reference GCR, same count"""
    from tests._krylov_ref import eps_ref
    pr = _case(64, 64, 16, "FC")
    e, nref, href = eps_ref(lambda: _oracle(pr), 8, 1e-10)
    _gpu(mg, pr)
    n, hist = _solve(mg, 8, 1e-10)
    d = _ratio(hist, href, 1e-10)
    print(f"\n64x64x16 FC m=8: GPU {n} it, reference {nref} it, eps_ref {e:.3e}, max rel. history difference {d:.3e} = {d / e:.2f} x eps_ref")
    print(" gpu " + " ".join(f"{v:.3e}" for v in hist))
    assert n == nref, (n, nref)
    assert d <= 10 * e, (d, e)
    assert mg.nhydro.get_option("krylov_restarts") == 0


@pytest.mark.parametrize("what", ["simple", "bmask"])
def test_history_follows_the_reference_gcr_simple_and_masked(mg, what):
    """64x64x16 four colours, m = 4, to 1e-10 with cmatrix = 'simple' (k_kr_apply_mf<false>) and with the island mask (the stored-slot operator
    k_kr_apply): entry by entry within 10 x eps_ref of the reference GCR on the same case, same count"""
    from tests._krylov_ref import eps_ref
    pr = _case(64, 64, 16, "FC", cmatrix="simple") if what == "simple" else _case(64, 64, 16, "FC", bmask=True)
    e, nref, href = eps_ref(lambda: _oracle(pr), 4, 1e-10)
    _gpu(mg, pr)
    if what == "bmask":
        assert np.array_equal(mg.grid(1).b, _oracle(pr).field("b"))
    n, hist = _solve(mg, 4, 1e-10)
    d = _ratio(hist, href, 1e-10)
    print(f"\n64x64x16 FC m=4 {what}: GPU {n} it, reference {nref} it, eps_ref {e:.3e}, max rel. history difference {d:.3e} = {d / e:.2f} x eps_ref")
    assert n == nref, (n, nref)
    assert d <= 10 * e, (d, e)
    assert mg.nhydro.get_option("krylov_restarts") == 0


def test_history_follows_the_reference_gcr_above_the_streaming_threshold(mg):
    """256x256x64 four colours, m = 4, tol 1e-8: 4.2 M cells, above the 3.56 M from which all three passes run their non-temporal variant.
    Same count as the reference GCR, history within 10 x eps_ref.  eps_ref is measured on this very case at tol 1e-8, not on a cheaper one
    (three oracle solves of 10 iterations: 77 s on 16 CPU threads, 21 s each for the plain order; the test prints its own time)."""
    from tests._krylov_ref import eps_ref
    import time
    t0 = time.time()
    pr = _case(256, 256, 64, "FC")
    e, nref, href = eps_ref(lambda: _oracle(pr), 4, 1e-8)
    t1 = time.time() - t0
    _gpu(mg, pr)
    n, hist = _solve(mg, 4, 1e-8)
    d = _ratio(hist, href, 1e-8)
    print(f"\n256x256x64 FC m=4: GPU {n} it, reference {nref} it ({t1:.0f} s for eps_ref), eps_ref {e:.3e}, max rel. history difference {d:.3e} = {d / e:.2f} x eps_ref")
    assert n == nref, (n, nref)
    assert d <= 10 * e, (d, e)
    assert mg.nhydro.get_option("krylov_restarts") == 0


@pytest.mark.parametrize("dims,meth,slack", [((128, 128, 16), "FC", 0), ((256, 256, 32), "RB", 1)])
def test_fewer_iterations_than_plain(mg, dims, meth, slack):
    from tests._krylov_ref import gcr
    pr = _case(*dims, meth)
    nref, href, _ = gcr(_oracle(pr), 4, 1e-6, 50)
    _gpu(mg, pr)
    npl, hpl = _solve(mg, 0, 1e-6)
    n, hist = _solve(mg, 4, 1e-6)
    print(f"\n{dims} {meth}: plain {npl} it -> {hpl[-1]:.3e}; krylov(4) {n} it -> {hist[-1]:.3e}; reference GCR {nref} it -> {href[-1]:.3e}")
    assert abs(n - nref) <= slack, (n, nref)
    assert n < npl, (n, npl)
    assert hist[-1] <= 1e-6


@pytest.mark.parametrize("dims,meth,bmask", [((32, 32, 24), "FC", False), ((32, 32, 24), "RB", False), ((32, 32, 24), "GS", False),
                                             ((64, 64, 16), "FC", True), ((64, 64, 16), "RB", True)])
def test_monotone_and_not_slower(mg, dims, meth, bmask):
    """an odd coarsest nz, the island mask, Gauss-Seidel once: monotone history, no more iterations than plain solve_p"""
    _gpu(mg, _case(*dims, meth, bmask=bmask))
    npl, hpl = _solve(mg, 0, 1e-10)
    n, hist = _solve(mg, 4, 1e-10)
    print(f"\n{dims} {meth} bmask={bmask}: plain {npl}, krylov(4) {n}: " + " ".join(f"{v:.2e}" for v in hist))
    assert np.all(np.diff(hist) < 0), hist
    assert n <= npl and hist[-1] <= 1e-10, (n, npl, hist)


def test_reported_residual_is_the_true_one(mg):
    """128x128x32 red-black, m = 8, tol 1e-14, 20 iterations: the recurrence drifts below the true residual there"""
    _gpu(mg, _case(128, 128, 32, "RB"))
    mg.nhydro.set_option("krylov", 8)
    from mgroms_amd._lib import lib
    import ctypes as C
    n, res, hist = C.c_int(), C.c_double(), (C.c_double * 21)()
    assert lib().mgx_solve_p(1e-14, 20, C.byref(n), C.byref(res), hist) == 0
    r_left = mg.grid(1).r
    b = mg.grid(1).b
    bn = np.sqrt(np.sum(b[1:-1, 1:-1, :] ** 2))
    true = mg.compute_residual(1) / bn          # independent: b - A p of the returned p
    r_true = mg.grid(1).r
    restarts = mg.nhydro.get_option("krylov_restarts")
    print(f"\n128x128x32 RB m=8: {n.value} it, res {res.value:.3e}, hist[-1] {hist[n.value]:.3e}, independent {true:.3e}, restarts {restarts}")
    assert abs(res.value - true) <= 1e-12 * true and abs(hist[n.value] - true) <= 1e-12 * true
    assert np.array_equal(r_left[1:-1, 1:-1, :], r_true[1:-1, 1:-1, :])
    assert n.value == 20 or res.value <= 1e-14
    assert restarts >= 1


@pytest.mark.parametrize("meth", ["FC", "RB"])
def test_off_means_off(meth):
    """option set to 4 and back to 0: p and hist bitwise those of a process that never set it"""
    out = []
    for touch in (0, 1):
        r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_krylov_off_worker.py"), meth, str(touch)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert out[0] == out[1]


def test_ranks_2x2(mg):
    """2x2 thread-ranks on one GPU, four colours, m = 4: the one-rank history within 10 x eps_ref, same count, one all-reduce per pass"""
    from tests._krylov_ref import eps_ref
    tol = 1e-8
    pr = _case(128, 128, 16, "FC")
    e, nref, href = eps_ref(lambda: _oracle(pr), 4, tol)
    _gpu(mg, pr)
    n1, h1 = _solve(mg, 4, tol)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_krylov_ranks.py"), "64", "64", "16", "4", str(tol), "50"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    d = _ratio(res["hist"], h1, tol)
    print(f"\n2x2 ranks: {res['n']} it (one rank {n1}, reference {nref}), eps_ref {e:.3e}, max rel. difference {d:.3e} = {d / e:.2f} x eps_ref, all-reduces {res['allreduces']}")
    assert res["same_on_all_ranks"]
    assert res["n"] == n1, (res["n"], n1)
    assert d <= 10 * e, (d, e)
    # ||b||, the first residual and the closing true residual: one each; per iteration one per pass (the first iteration and the first
    # after a restart have no retained pair, hence no inner product in pass 1: two)
    assert res["restarts"] == 0
    assert res["allreduces"] == 3 + 3 * res["n"] - 1, res


@pytest.mark.parametrize("device", [False, True])
def test_nhydro_solve_against_the_oracle(mg, device):
    """u, v, w of nhydro_solve[_device] with m = 4 at 1e-10 against the oracle's plain nhydro_solve at the same tolerance; bound: ten
    times the distance between the oracle's plain solution and the reference GCR's (both stop below the same tolerance)"""
    import torch
    from tests._krylov_ref import gcr
    nx, ny, nz = 64, 64, 16
    u, v, w = uvw((nx, ny, nz))
    pr = _case(nx, ny, nz, "FC")
    o = _oracle(pr)
    o.field("u")[...] = u; o.field("v")[...] = v; o.field("w")[...] = w
    o.nhydro_solve()
    plain = [o.field(k).copy() for k in "uvw"]
    o2 = _oracle(pr)
    o2.field("u")[...] = u; o2.field("v")[...] = v; o2.field("w")[...] = w
    o2.compute_rhs()
    gcr(o2, 4, 1e-10, 50)
    o2.correct_uvw()
    bound = [10 * np.abs(o2.field(k) - a).max() for k, a in zip("uvw", plain)]
    _gpu(mg, pr)
    mg.nhydro.set_option("krylov", 4)
    if device:
        d = [torch.from_numpy(a).cuda() for a in (u, v, w)]
        mg.nhydro.nhydro_solve_device(*d)
        got = [a.cpu().numpy() for a in d]
    else:
        mg.nhydro_solve(u, v, w)
        got = [u, v, w]
    err = [np.abs(g - a).max() for g, a in zip(got, plain)]
    print(f"\nnhydro_solve{'_device' if device else ''} m=4: |u,v,w - oracle| {err}, bound {bound}")
    assert all(b > 0 for b in bound)
    assert all(e <= b for e, b in zip(err, bound)), (err, bound)


def test_refusals(mg):
    from mgroms_amd._lib import MgxError
    for bad in (9, -1):
        with pytest.raises(MgxError, match="krylov"):
            mg.nhydro.set_option("krylov", bad)
    assert mg.nhydro.get_option("krylov") == 0
    _gpu(mg, _case(32, 32, 8, "FC"))
    mg.nhydro.set_option("krylov", 4)
    mg.nhydro.set_option("cycle_precision", 32)
    with pytest.raises(MgxError, match=r"krylov.*cycle_precision"):
        mg.solve_p(1e-8, 10)
    mg.nhydro.set_option("cycle_precision", 64)
    n, hist = mg.solve_p(1e-8, 10)
    assert hist[-1] <= 1e-8
    mg.nhydro_clean()
    assert mg.nhydro.get_option("krylov") == 4   # kept across mgx_clean like the other options


def test_warm_start(mg):
    """warm_start: the second solve starts from the p found"""
    _gpu(mg, _case(64, 64, 16, "FC"))
    n, hist = _solve(mg, 4, 1e-8)
    mg.nhydro.set_option("warm_start", 1)
    n2, hist2 = mg.solve_p(1e-8, 50)
    assert n2 == 0 and abs(hist2[0] - hist[-1]) <= 1e-10 * hist[-1], (n2, hist2, hist)


def test_tictoc_rows():
    """the new kernels have tic/toc rows of their own, called once per iteration"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_krylov_off_worker.py"), "FC", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    lines = out["tictoc"].splitlines()
    for name in ("krylov_apply", "krylov_ortho", "krylov_update", "Fcycle"):
        q = [k for k, l in enumerate(lines) if l.split() and l.split()[0] == name]
        assert q, (name, out["tictoc"])
        assert int(lines[q[0] + 1].split()[0]) == out["n"], (name, lines[q[0] + 1])
