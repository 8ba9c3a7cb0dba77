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


# ---- the per-pass references of tests/_krylov_kernel_ref.py (what tests/test_gpu_krylov_kernels.py holds the three HIP passes to) ----
import pytest

from tests import _krylov_kernel_ref as K

# the two streaming sizes take a minute of numpy each: once, with the largest nd
_EXACT = [(sh, nd) for sh in K.SMALL_SHAPES for nd in K.NDS] + [(sh, 8) for sh in K.BIG_SHAPES]


@pytest.mark.parametrize("shape,nd", _EXACT, ids=[f"{s[0]}x{s[1]}x{s[2]}-nd{n}" for s, n in _EXACT])
def test_integer_cases_stay_exact_and_order_independent(shape, nd):
    """the integer fields of passes 2 and 3 on every shape of the list: every sum below 2^53 (check_exact), and plain, reversed and
    fsum orders give the same bits -- the premise of the exact comparisons on the GPU"""
    big = shape in K.BIG_SHAPES
    c = K.ortho_case(shape, nd, seed=100 + nd, slot=K.rotated_slots(nd))
    out = [K.ref_ortho(c["z"], c["q"], c["r"], c["zi"], c["qi"], c["sc"], c["qq"], c["slot"], dot=d)
           for d in ((K.dot_plain, K.dot_reversed) if big else (K.dot_plain, K.dot_reversed, K.dot_fsum))]
    z, q, s, t = out[0]
    K.check_exact([z, q, c["r"]] + c["zi"] + c["qi"], [(q, q), (c["r"], q)])
    assert all((o[2], o[3]) == (s, t) for o in out), [(o[2], o[3]) for o in out]
    assert s == int(s) and t == int(t) and s > 0
    # the halo cells (2^40) are in the arrays the pass reads and outside every sum
    assert abs(t) < 2.0 ** 40 and all(np.abs(a[0]).min() == K.HALO and np.abs(a[:, -1]).min() == K.HALO for a in [c["q"], c["r"]] + c["qi"])
    del out, c
    for st in ((4.0, 2.0), (2.0, 8.0)):
        u = K.update_case(shape, seed=7, s=st[0], t=st[1])
        res = [K.ref_update(u["p"], u["r"], u["z"], u["q"], *st, dot=d) for d in ((K.dot_plain, K.dot_reversed) if big else (K.dot_plain, K.dot_reversed, K.dot_fsum))]
        K.check_exact([res[0][0], res[0][1]], [(res[0][1], res[0][1])], unit=min(1.0, st[1] / st[0]))
        assert all(r[2] == res[0][2] for r in res) and res[0][3] == st[0]
        if big:
            break


def test_update_reference_guard():
    u = K.update_case((6, 10, 4), seed=8)
    for s, t in ((0.0, 1.0), (-4.0, 1.0), (np.inf, 1.0), (4.0, np.nan), (4.0, np.inf)):
        p, r, norm, qn = K.ref_update(u["p"], u["r"], u["z"], u["q"], s, t)
        assert norm == -1.0 and qn == s and np.array_equal(p, u["p"]) and np.array_equal(r, u["r"])


@pytest.mark.parametrize("shape", K.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in K.SHAPES])
def test_probe_cells_are_what_they_claim(shape):
    """every listed one-hot cell is interior, every halo probe is not; the list holds the corners, both ends of either half-row, k = 1 and
    k = nz, the last plane, and the wave boundary where the shape has one"""
    nx, ny, nz = shape
    cells, probes = K.onehot_cells(nx, ny, nz), K.halo_probes(nx, ny, nz)
    assert all(K.is_interior(c, nx, ny, nz) for c in cells) and len(set(cells)) == len(cells)
    assert not any(K.is_interior(c, nx, ny, nz) for c in probes) and len(probes) == 8
    assert {(i, j, k) for i in (1, nx) for j in (1, ny) for k in (1, nz)} <= set(cells)
    js = {j for _, j, _ in cells}
    assert {1, 2, ny - 1, ny} <= js
    assert any(i == nx for i, _, _ in cells) and {1, nz} <= {k for _, _, k in cells}
    if ny // 2 > 64:
        assert {127, 128, 129, 130} & js == {127, 128, 129, 130} if ny >= 130 else True
    for i, j, k in probes:
        assert i in (0, nx + 1) or j in (0, ny + 1)


def test_shape_list_reaches_every_path():
    """the launch paths the shape list is there for, from the dimensions alone"""
    paths = {sh: K.expected_path(*sh) for sh in K.SHAPES}
    assert any(st == 1 for st, _, _ in paths.values()) and paths[(512, 512, 64)][0] == 1 and paths[(256, 256, 64)][0] == 1
    assert any(gy & 7 and gy > 1 for _, _, gy in paths.values()) and any(gy & 7 == 0 for _, _, gy in paths.values())
    assert any(gx >= 2 for (nx, ny, nz), (_, gx, _) in paths.items() if nx * ny * nz < 1e6)
    assert any(nx % 4 for nx, _, _ in K.SHAPES) and any((ny // 2) % 2 for _, ny, _ in K.SHAPES) and any(nz == 2 for _, _, nz in K.SHAPES)
    assert paths[(4, 130, 4)][1] == 2 and 130 // 2 - 64 == 1        # gx = 2 with one live lane


def test_gcr_from_the_reference_passes_reproduces_gcr():
    """32x32x8 four colours, m = 4: the loop built from ref_apply / ref_ortho / ref_update (the ring of m + 1 slots, all (q, q_n) taken
    from q before it is changed, as pass 1 does) against gcr() (each beta from the q already orthogonalised): the same count, histories
    within 10 x eps_ref of the same case"""
    from tests._krylov_ref import history_noise
    e, n0, h0 = eps_ref(lambda: _make(32, 32, 8, "FC"), 4, 1e-8)
    n, h = K.gcr_from_passes(_make(32, 32, 8, "FC"), 4, 1e-8, 50)
    d = history_noise(h, h0, 1e-8)
    print(f"\n32x32x8 FC GCR(4): {n0} iterations, from the passes {n}; eps_ref {e:.3e}, difference {d:.3e}")
    assert n == n0 and n > 5
    assert d <= 10 * e, (d, e)
