"""The CSR export on the GPU (include/mgx.h: mgx_operator_csr, mgx_transfer_csr; nhydro.operator_csr, restriction_csr, prolongation_csr):
A, R and P of EVERY level of ten hierarchies against the operators they were read off.  Every check is an identity or a derived bound:

  entries   column j of the matrix is what the library's own operator makes of the unit vector e_j, bit for bit (array_equal): for every
            unknown of a level of at most 512 unknowns, for 64 seeded ones (corners, ring, coast, k = 1 and k = nz among them) above.  This
            is what catches two unit vectors of one probe meeting in a row.
  mat-vec   CSR x against the operator on x ~ N(0, 1), row by row within 2 n 2^-53 (|M| |x|), n = 19 for A (both sides sum the same <= 19
            products in different orders; a product is rounded once and a sum of n terms n - 1 times: (1 + u)^n - 1 <= n u (1 + n u) per side) and
            the row's own entry count for R and P.  |M| |x| comes from the CSR itself.
  shape     rowptr monotone and ending at nnz, columns strictly increasing per row and inside [0, ncols), no +-0 values, at most 15 entries
            per row of A (19 in the bottom row with cmatrix = 'real'), 8 per row of R (4 on a held pair) and of P.
  oracle    level 1 of 16 x 16 x 8, 'real' and 'simple': the dense A equals bit for bit the matrix that the dense cross-check of
            tests/test_oracle.py assembles from the CPU oracle (restated below).
  direct    numpy.linalg.solve on the dense A and the level's b against solve_p converged to 1e-12, within the 1e-11 max|p| that
            tests/test_oracle.py asserts for the oracle's solve_p; and once on the island with bmask, on the water rows, where no oracle
            answer exists.
  state     p, b, r of both levels (halos included) and the history of the next solve_p are the same bits with and without exports between.
  refusals  by message.  (The refusal of a level whose rows or entries do not fit an int is a pure function, pinned in
            tests/test_export_host.py: no quick test can build such a level.)

Measured on the MI355X: 10 464 columns compared over the ten cases, all equal; the largest error of a mat-vec row over its bound is 0.17 for
A, 0.43 for R and 0.99 for P (island P(2), semi-coarsened P(1): a boundary row of P holds one entry where the kernel summed several
products that the halo rule folds onto one coarse cell, so the entry count undercounts the kernel's roundings there); the direct solve
agrees with solve_p to 1.0e-12 of max|p| on the seamount and to 1.7e-13 on the water rows of the island.
"""
import numpy as np
import pytest

from _gpu import gpu_module, restore_options
from _problem import gpu_problem, oracle_twin, rhs, uvw

pytestmark = pytest.mark.gpu

mg = gpu_module(periodic=0, hold_z_levels=0, hold_odd_nz=0, warm_start=0)
_restore_options = restore_options("warm_start")

U = 2.0 ** -53
#        id                          dims           namelist members                               options mgx_init reads
CASES = [("seamount-16x16x8-real",   (16, 16, 8),   dict(cmatrix="real", interp_type="linear"),    {}),
         ("seamount-16x16x8-simple", (16, 16, 8),   dict(cmatrix="simple", interp_type="nearest"), {}),
         ("seamount-32x16x8",        (32, 16, 8),   dict(interp_type="nearest"),                   {}),
         ("seamount-24x16x12",       (24, 16, 12),  dict(),                                        {}),
         ("island-32x32x8-bmask",    (32, 32, 8),   dict(bmask=True),                              {}),
         ("periodic-16x16x8",        (16, 16, 8),   dict(),                                        dict(periodic=3)),
         ("periodic-20x12x4",        (20, 12, 4),   dict(interp_type="nearest"),                   dict(periodic=3)),
         ("semi-32x32x16",           (32, 32, 16),  dict(),                                        dict(hold_z_levels=1)),
         ("oddnz-32x32x10",          (32, 32, 10),  dict(),                                        dict(hold_odd_nz=1)),
         ("user-matrix-16x16x8",     (16, 16, 8),   dict(),                                        {})]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}


class Csr:
    """a CSR matrix on the host, numpy only"""

    def __init__(self, t):
        self.shape = tuple(t.shape)
        self.rowptr = t.crow_indices().cpu().numpy()
        self.col = t.col_indices().cpu().numpy()
        self.val = t.values().cpu().numpy()
        assert self.rowptr.dtype == np.int32 and self.col.dtype == np.int32 and self.val.dtype == np.float64
        assert t.is_cuda and self.rowptr.shape == (self.shape[0] + 1,) and self.col.shape == self.val.shape
        self.count = np.diff(self.rowptr.astype(np.int64))
        self.row = np.repeat(np.arange(self.shape[0]), self.count)

    def column(self, q):
        out = np.zeros(self.shape[0])
        sel = self.col == q
        out[self.row[sel]] = self.val[sel]
        return out

    def times(self, x, absolute=False):
        v = np.abs(self.val) if absolute else self.val
        return np.bincount(self.row, weights=v * x[self.col], minlength=self.shape[0])

    def dense(self):
        a = np.zeros(self.shape)
        a[self.row, self.col] = self.val
        return a


_live = {"id": None}
_exports = {}


def _hier(mg, cid):
    """the case's hierarchy live on the GPU (set up again only when another case was) and its exports, made once per case"""
    _, dims, par, opts = BY_ID[cid]
    if _live["id"] != cid:
        _live["id"] = None
        par = dict(par)
        bmask = par.pop("bmask", False)
        pr = gpu_problem(mg, dims, bmask=bmask, init_options=dict(dict(periodic=0, hold_z_levels=0, hold_odd_nz=0), **opts), relax_method="FC", **par)
        if cid.startswith("user-matrix"):
            g = mg.grid(1)
            g.set("cA", 1.5 * g.get("cA"))
        _live.update(id=cid, pr=pr)
    if cid not in _exports:
        nl = mg.nlevs()
        _exports[cid] = {"A": {lev: Csr(mg.nhydro.operator_csr(lev)) for lev in range(1, nl + 1)},
                         "R": {lev: Csr(mg.nhydro.restriction_csr(lev)) for lev in range(1, nl)},
                         "P": {lev: Csr(mg.nhydro.prolongation_csr(lev)) for lev in range(1, nl)}}
    return _live["pr"], _exports[cid]


def _dims(g):
    return g.nx, g.ny, g.nz


def _pad(x, g):
    a = np.zeros((g.nx + 2, g.ny + 2, g.nz))
    a[1:-1, 1:-1, :] = x.reshape(_dims(g))
    return a


def _inner(a):
    return a[1:-1, 1:-1, :].ravel()


def _apply(mg, what, lev, x):
    """the library's own operator on x (an interior field of the column level, flat in the export's order) from zeroed targets"""
    F = mg.grid(lev)
    if what == "A":
        F.set("p", _pad(x, F)); F.set("b", np.zeros(F._shape("b"))); mg.fill_halo(lev, "p")
        mg.compute_residual(lev)
        return -_inner(F.get("r"))
    C = mg.grid(lev + 1)
    if what == "R":
        F.set("r", _pad(x, F)); C.set("b", np.zeros(C._shape("b")))
        mg.fine2coarse(lev)
        return _inner(C.get("b"))
    C.set("p", _pad(x, C)); mg.fill_halo(lev + 1, "p"); F.set("p", np.zeros(F._shape("p")))
    mg.coarse2fine(lev)
    return _inner(F.get("p"))


def _column_level(mg, what, lev):
    return mg.grid(lev + 1 if what == "P" else lev)


def _unknowns(g, rng):
    """every unknown of a level of at most 512, else 64: the eight corners, ring cells at k = 1 and k = nz, coast cells (water next to land,
    and land) where the level has a mask, seeded ones for the rest"""
    nx, ny, nz = _dims(g)
    n = nx * ny * nz
    if n <= 512:
        return list(range(n))
    idx = lambda i, j, k: (i * ny + j) * nz + k   # noqa: E731  (0-based cell)
    pick = [idx(i, j, k) for i in (0, nx - 1) for j in (0, ny - 1) for k in (0, nz - 1)]
    pick += [idx(i, j, k) for k in (0, nz - 1) for i, j in ((0, ny // 2), (nx - 1, ny // 2 - 1), (nx // 2, 0), (nx // 2 - 1, ny - 1))]
    m = g.get("rmask")
    land = np.argwhere(m[1:-1, 1:-1] == 0)
    for i, j in land[:: max(len(land) // 6, 1)][:6]:
        pick.append(idx(i, j, int(rng.integers(nz))))
        for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            if 0 <= i + di < nx and 0 <= j + dj < ny and m[i + di + 1, j + dj + 1] == 1:
                pick.append(idx(i + di, j + dj, (0, nz - 1)[(i + j) & 1]))
                break
    pick = list(dict.fromkeys(pick))[:48]
    have = set(pick)
    rest = [int(q) for q in rng.permutation(n) if q not in have]
    return pick + rest[:64 - len(pick)]


def _matrices(mg, ex):
    for what in ("A", "R", "P"):
        for lev, m in ex[what].items():
            yield what, lev, m


@pytest.mark.parametrize("cid", IDS)
def test_entries_exact(mg, cid):
    _, ex = _hier(mg, cid)
    rng = np.random.default_rng(11)
    n = 0
    for what, lev, m in _matrices(mg, ex):
        g = _column_level(mg, what, lev)
        assert m.shape[1] == g.nx * g.ny * g.nz
        for q in _unknowns(g, rng):
            e = np.zeros(m.shape[1]); e[q] = 1.0
            got = _apply(mg, what, lev, e)
            assert got.shape == (m.shape[0],)
            assert np.array_equal(got, m.column(q)), (what, lev, q, np.flatnonzero(got != m.column(q))[:8])
            n += 1
    print("%s: %d columns compared" % (cid, n))


@pytest.mark.parametrize("cid", IDS)
def test_matvec(mg, cid):
    _, ex = _hier(mg, cid)
    rng = np.random.default_rng(12)
    worst = 0.0
    for what, lev, m in _matrices(mg, ex):
        x = rng.standard_normal(m.shape[1])
        got, want, scale = _apply(mg, what, lev, x), m.times(x), m.times(np.abs(x), absolute=True)
        terms = 19 if what == "A" else m.count
        bound = 2 * terms * U * scale
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        worst = max(worst, ratio.max())
        print("%s %s(%d): largest error / bound = %.3f" % (cid, what, lev, ratio.max()))
        assert np.all(err <= bound), (what, lev, int(np.argmax(ratio)), ratio.max())
        assert np.abs(want).max() > 0, (what, lev)
    assert worst <= 1.0


@pytest.mark.parametrize("cid", IDS)
def test_shape_of_the_output(mg, cid):
    pr, ex = _hier(mg, cid)
    real = pr.par.get("cmatrix", "real") == "real"
    for what, lev, m in _matrices(mg, ex):
        F = mg.grid(lev)
        rows = mg.grid(lev + 1) if what == "R" else F
        cols = _column_level(mg, what, lev)
        assert m.shape == (rows.nx * rows.ny * rows.nz, cols.nx * cols.ny * cols.nz), (what, lev)
        assert m.rowptr[0] == 0 and np.all(m.count >= 0) and m.rowptr[-1] == m.val.size, (what, lev)   # val was sized by the *_size call
        assert m.col.size == 0 or (m.col.min() >= 0 and m.col.max() < m.shape[1]), (what, lev)
        same_row = m.row[1:] == m.row[:-1]
        assert np.all(np.diff(m.col.astype(np.int64))[same_row] > 0), (what, lev)
        assert np.all(m.val != 0) and np.all(np.isfinite(m.val)), (what, lev)
        k = np.arange(m.shape[0]) % rows.nz
        if what == "A":
            assert m.count[k > 0].max() <= 15 and m.count[k == 0].max() <= (19 if real else 15), (lev, m.count.max())
            assert m.count.max() >= 7, lev
        elif what == "R":
            held = mg.grid(lev + 1).nz == F.nz
            assert m.count.max() == (4 if held else 8), (lev, m.count.max())
        else:
            assert 1 <= m.count.max() <= 8, (lev, m.count.max())


def _oracle_dense(o, nx, ny, nz):
    """the dense cross-check of tests/test_oracle.py (test_multigrid_solution_equals_a_direct_solve), restated: the level-1 operator column by
    column from the oracle's residual routine"""
    n = nx * ny * nz
    a = np.zeros((n, n))
    for q in range(n):
        e = np.zeros(n); e[q] = 1.0
        p = o.field("p"); p[...] = 0; p[1:-1, 1:-1, :] = e.reshape(nx, ny, nz)
        o.fill_halo(1, "p"); o.field("b")[...] = 0; o.residual(1)
        a[:, q] = -o.field("r")[1:-1, 1:-1, :].ravel()
    return a


@pytest.mark.parametrize("cid", IDS[:2])
def test_level_one_equals_the_oracles_dense_matrix(mg, cid):
    pr, ex = _hier(mg, cid)
    o = oracle_twin(pr)
    try:
        want = _oracle_dense(o, *pr.dims)
    finally:
        o.close()
    got = ex["A"][1].dense()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def _direct_against_solve_p(mg, cid, water_only):
    pr, ex = _hier(mg, cid)
    rhs(mg, None, uvw(pr.dims))
    g = mg.grid(1)
    b = _inner(g.get("b"))
    nit, hist = mg.solve_p(1e-12, 60)
    assert hist[-1] < 1e-12, hist
    p = _inner(g.get("p"))
    a = ex["A"][1].dense()
    keep = np.ones(b.size, bool)
    if water_only:
        keep = np.repeat(g.get("rmask")[1:-1, 1:-1].ravel() == 1, g.nz)
        assert not a[keep][:, ~keep].any()   # no water row reaches a land column
    direct = np.linalg.solve(a[np.ix_(keep, keep)], b[keep])
    err = np.abs(p[keep] - direct).max() / np.abs(direct).max()
    print("%s: max |solve_p - direct| / max |direct| = %.3e after %d iterations" % (cid, err, nit))
    return err


def test_direct_solve_on_the_gpu_operator(mg):
    """the bound of tests/test_oracle.py::test_multigrid_solution_equals_a_direct_solve"""
    assert _direct_against_solve_p(mg, "seamount-16x16x8-real", False) <= 1e-11


def test_direct_solve_on_the_masked_gpu_operator(mg):
    """the same on the island with bmask, water rows only: the case the oracle-side test has no answer for.  The same bound."""
    assert _direct_against_solve_p(mg, "island-32x32x8-bmask", True) <= 1e-11


@pytest.mark.parametrize("cid", IDS)
def test_state_untouched(mg, cid):
    pr, _ = _hier(mg, cid)
    mg.nhydro.set_option("warm_start", 1)
    nl = mg.nlevs()
    pairs = sorted({1, nl - 1})

    def run(export):
        rng = np.random.default_rng(13)
        rhs(mg, None, uvw(pr.dims, seed=3))
        for lev in range(1, nl + 1):
            g = mg.grid(lev)
            for name in ("p", "r") + (("b",) if lev > 1 else ()):
                g.set(name, rng.standard_normal(g._shape(name)))
            for name in ("p", "b", "r"):   # valid halos and no deferred fill left over from whatever ran before
                mg.fill_halo(lev, name)
        for lev in pairs:   # a deferred halo of r on the fine and of b on the coarse level
            mg.compute_residual(lev); mg.fine2coarse(lev)
        if export:
            for lev in pairs:
                mg.nhydro.operator_csr(lev); mg.nhydro.operator_csr(lev + 1); mg.nhydro.restriction_csr(lev); mg.nhydro.prolongation_csr(lev)
        fields = {(lev, name): mg.grid(lev).get(name) for lev in sorted({q for lev in pairs for q in (lev, lev + 1)}) for name in ("p", "b", "r")}
        return fields, mg.solve_p(1e-9, 6)

    f0, (n0, h0) = run(False)
    f1, (n1, h1) = run(True)
    for key in f0:
        assert np.array_equal(f0[key], f1[key]), key
    assert n0 == n1 and np.array_equal(h0, h1), (h0, h1)


def test_refusals(mg):
    from mgroms_amd._lib import MgxError
    import ctypes as C
    nh = mg.nhydro
    _live["id"] = None
    mg.nhydro_clean()
    for call in (lambda: nh.operator_csr(1), lambda: nh.restriction_csr(1), lambda: nh.prolongation_csr(1)):
        with pytest.raises(MgxError, match="mgx_init has not been called"):
            call()
    for name in ("periodic", "hold_z_levels", "hold_odd_nz"):
        nh.set_option(name, 0)
    par = nh.default_params(relax_method="FC")
    mg.nhydro_init(16, 16, 8, 1, 1, 0, par)
    for call in (lambda: nh.operator_csr(1), lambda: nh.restriction_csr(1), lambda: nh.prolongation_csr(1)):
        with pytest.raises(MgxError, match="no matrix: call mgx_matrices"):      # before nhydro_matrices
            call()
    gpu_problem(mg, (16, 16, 8), relax_method="FC")
    nl = mg.nlevs()
    for lev in (0, nl + 1, -3):
        for call in (nh.operator_csr, nh.restriction_csr, nh.prolongation_csr):
            with pytest.raises(MgxError, match="level %d out of range 1..%d" % (lev, nl)):
                call(lev)
    for call in (nh.restriction_csr, nh.prolongation_csr):
        with pytest.raises(MgxError, match=r"mgx_transfer_csr\(%d\): no coarser level" % nl):
            call(nl)
    n = C.c_longlong()
    assert nh.lib().mgx_transfer_csr_size(1, 2, C.byref(n), C.byref(n), C.byref(n)) != 0
    assert "which = 2 is neither 0" in nh.lib().mgx_last_error().decode()
    # the *_csr call fills buffers that the *_size call sized: without one for the same matrix it is refused
    import torch
    nh.operator_csr(2)
    buf = torch.empty(1 << 16, dtype=torch.int32, device="cuda"); val = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert nh.lib().mgx_operator_csr(1, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(val.data_ptr())) != 0
    assert "call mgx_operator_csr_size for this matrix first" in nh.lib().mgx_last_error().decode()
    assert nh.lib().mgx_operator_csr(1, None, None, None) != 0
    assert "must all be device pointers" in nh.lib().mgx_last_error().decode()
    nh.operator_csr(nl)    # (the coarsest level has an operator, and no transfer)
    # a process grid: refused before anything else is asked of the level (no hooks are needed to initialise one rank of a closed grid)
    mg.nhydro_clean()
    mg.nhydro_init(16, 16, 8, 2, 1, 0, par)
    for call in (lambda: nh.operator_csr(1), lambda: nh.restriction_csr(1), lambda: nh.prolongation_csr(1)):
        with pytest.raises(MgxError, match=r"a process grid \(2 x 1\) is out of scope"):
            call()
    mg.nhydro_clean()
