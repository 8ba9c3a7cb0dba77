"""The yardstick of option "krylov": the numpy GCR over the CPU oracle (tests/_krylov_ref.py).  Pins that it is monotone, that it does
what the option is for (128x128x16 four colours, m = 4: 1e-6 within 15 iterations where plain solve_p has not got there after 20), and
measures its own noise eps_ref (the same solve with its inner products summed in another order), which bounds how closely any other
implementation can be asked to follow its history.  Measured here: see the printed figures (pytest -s) and DESIGN.md 4.8."""
import numpy as np

from oracle.mgoracle import make_seamount
from tests._krylov_ref import gcr, eps_ref


def _make(nx, ny, nz, meth):
    o = make_seamount(nx, ny, nz, relax_method=meth)
    o.compute_rhs()
    return o


def test_reference_gcr_beats_plain_on_the_hard_grid():
    o = _make(128, 128, 16, "FC")
    npl, hpl, _ = o.solve_p(1e-6, 20)
    n, h, restarts = gcr(_make(128, 128, 16, "FC"), 4, 1e-6, 20)
    print(f"\n128x128x16 FC: plain {npl} it -> {hpl[-1]:.3e}; GCR(4) {n} it -> {h[-1]:.3e}, restarts {restarts}")
    assert np.all(np.diff(h) < 0), h
    assert h[-1] <= 1e-6 and n <= 15, (n, h)
    assert hpl[-1] > 1e-6 and npl == 20, (npl, hpl)


def test_reference_gcr_monotone_and_its_own_noise():
    e, n, h = eps_ref(lambda: _make(64, 64, 16, "FC"), 8, 1e-10)
    print(f"\n64x64x16 FC GCR(8) to 1e-10: {n} iterations, eps_ref = {e:.3e}")
    print(" history " + " ".join(f"{v:.3e}" for v in h))
    assert np.all(np.diff(h) < 0), h
    assert h[-1] <= 1e-10
    # round-off of sums over 64k cells amplified through ~10 iterations: far below the residual reduction per step, far above one ulp
    assert 0.0 < e < 1e-6, e
