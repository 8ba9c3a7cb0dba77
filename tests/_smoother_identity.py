"""The rule of the smoother identities, stated once (tests/test_oracle.py, tests/test_gpu_smoother_identity.py).

Every smoother test but these compares relax() with the CPU oracle's relax().  Here the smoother of a level is held to the level's own
operator, r = b - A p as compute_residual forms it, by what a line smoother satisfies exactly.  T is the in-column tridiagonal part of A,
the RING the columns i = 1, nx, j = 1, ny.  With p* ~ N(0, 1) in every cell (halo filled) and b := A p* (compute_residual with b = 0,
negated):

  1  FIXED POINT (every method, every column, ring included): relax(lev, 2) from p* leaves p*.  Defect max|p - p*| / max|p*| over the
     interior.  The (T, off-column terms) of every colour's text equal the residual's A.  A smoother that does nothing passes: hence 2, 3.
  2  THE FIRST COLOUR IS A COMPLETE SOLVE (four colours, red-black): from p* + delta, delta of size 1 .. 2 (first_colour says how it is
     drawn) on the non-ring columns of the first colour -- four colours (i odd, j odd), red-black i + j even
     (mg_relax.f90:174,216-217) -- relax(lev, 1) gives back p* everywhere, in the units of 1.  Red-black with cmatrix = 'real': delta has a zero row k = 1, because the bottom row couples same-colour diagonals
     (mg_relax.f90:271-276).  Ring columns stay unperturbed: a ring column reads its own mirror image as it was before the pass, so the
     reference itself does not solve them completely.
  3  THE LAST COLOUR HAS NO RESIDUAL (four colours, red-black): from p ~ N(0, 1) (halo filled) and b ~ N(0, 1) times the size of A p of
     the relaxed p (last_colour says how that is found), relax(lev, 1), then compute_residual: r vanishes on the non-ring columns of the last colour -- four colours (i even, j even), red-black i + j odd
     -- in units of max|A p| of the relaxed p over the level.  Red-black 'real': rows k >= 2 only.

Controls, asserted with the checks so that a check which stopped looking fails: 2 with delta on the LAST colour leaves > 1e-3; in 3 the
residual on the non-ring columns of the other colours exceeds 1e-2; in 3 for red-black 'real' row k = 1 of the last colour exceeds 1e-4
(the row is excluded because it has to be).  The set of 2 and 3 is "not in the ring" and nothing narrower -- land and coast columns are
in it --, and a level enters 2 and 3 with nx, ny >= 4, so that every colour has a column in the set.

Gauss-Seidel gets check 1 only: in lexicographic order no interior column is first or last in the sense 2 and 3 need (each reads
neighbours already updated and neighbours still to come).  Its completeness stays with the comparison against the oracle.

The nearest-neighbour transfers are exact adjoints, <R r, q> = <r, P q> (fine2coarse: fine r -> coarse b; coarse2fine with
interp_type = 'nearest': coarse p -> the fine correction, read as the fine p from p = 0), on every level pair whose fine nz is even.
On a pair with an odd fine nz (5 -> 2) the reference's restriction leaves the top fine row out and its prolongation does not write it (the fine r keeps what it held there, and
p = p + r adds it): the identity fails there at O(1), which is asserted on the oracle so that the exclusion is known to matter.

The checks, colour sets and defects are pure numpy over a small backend (set_p_b, relax, residual, p, dims, nlevs, cA); the oracle enters
through OracleBackend only, the library through GpuBackend.

BOUNDS.  Measured on the CPU oracle (tests/test_oracle.py::test_smoother_identities_on_the_oracle prints them): the largest defect over
every level of every case of CASES that the oracle can build and eight seeds, per check; asserted on the GPU: 16 x that, the margin
COUPLING_TOL uses, for other seeds and the GPU's other summation order.  The cases the oracle has no hierarchy for (hold_odd_nz, periodic)
take the same bounds.  One exception, taken from the project: red-black with cmatrix = 'real' in the sequential order at speed (the window,
walk_apply, scan and k_relax_wave's walk) is documented as within 1e-12 of max|p| per relax call (header of tests/test_gpu_parity.py): every level
of a case with rb_seq = 1 and rb_exact = 0 takes 1e-12 for checks 1 and 2, and for check 3 what an error of 1e-12 max|p| in every cell
can leave in r, 1e-12 max|p| ||A||_inf / max|A p| with ||A||_inf bounded from the level's stored slots (norm_bound), or TOL3 if larger.
rb_exact = 1 (the plane loop) and rb_seq = 0 (the parallel sweep on a snapshot) take the 16 x bounds."""
import collections

import numpy as np

from _operator_identity import inner

# ---- bounds: the eight-seed maxima of the oracle over CASES (printed by tests/test_oracle.py) and 16 x each ----
MEASURED = {1: 1.21e-13, 2: 9.54e-14, 3: 5.95e-14}       # check: largest defect on the oracle (all three at island-32x32x96 / 32x32x128,
#                                                          level 1: tall columns beside land; without them 8.1e-15, 6.8e-15, 3.3e-15)
TOL = {1: 1.94e-12, 2: 1.53e-12, 3: 9.52e-13}            # 16 x MEASURED
ADJOINT_MEASURED = 7.3e-18                               # |<R r, q> - <r, P q>| / (||r|| ||P q||), even fine nz, longdouble sums; the held
#                                                          pairs of tests/_hold_ref.py (4x4x5, 8x8x5, 16x16x5 fine): 1.4e-17
ADJOINT_TOL = 2.3e-16                                    # 16 x the larger of the two
RB_SEQ_TOL = 1e-12                                       # the project's bound of the sequential order at speed, per relax call
SEEDS = tuple(range(8))
# conditions, not measurements.  The oracle's minima over CASES, SEEDS and every level: 1.3e-2 (check 2), 0.13 (check 3), a factor 13 above
# each (asserted at a factor 3 in tests/test_oracle.py).  Row k = 1: 1.8e-4, always on a level four columns wide (4x64x2, 4x4x3, 4x4x16)
# -- the bottom row's diagonals carry the bottom slope, which all but vanishes at the seamount's summit, and that is where the inner
# columns i = 2, 3 of such a level lie; the ratio of that row's residual to the other colour's is the ratio of slots 5, 8 to slots 4, 7
# whatever p and b are, so no input of the check moves it (level 1 of every case: >= 1.7e-3)
CONTROL_2, CONTROL_3, CONTROL_ROW1, ODD_PAIR = 1e-3, 1e-2, 1e-4, 1e-2


# ---- the colour sets ----
def ring(nx, ny):
    r = np.zeros((nx, ny), dtype=bool)
    r[0, :] = r[-1, :] = True
    r[:, 0] = r[:, -1] = True
    return r


def colour_sets(method, nx, ny):
    """(first, last, others): boolean (nx, ny) arrays over the columns i = 1..nx, j = 1..ny (entry [i-1, j-1]) that are NOT in the ring"""
    assert method in ("FC", "RB") and nx >= 4 and ny >= 4
    i, j = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), indexing="ij")
    if method == "FC":
        first, last = (i % 2 == 1) & (j % 2 == 1), (i % 2 == 0) & (j % 2 == 0)
    else:
        first, last = (i + j) % 2 == 0, (i + j) % 2 == 1
    inside = ~ring(nx, ny)
    first, last, others = first & inside, last & inside, ~last & inside
    assert first.any() and last.any() and others.any()
    return first, last, others


# ---- the three checks ----
def _with_halo(be, lev, interior):
    nx, ny, nz = be.dims(lev)
    a = np.zeros((nx + 2, ny + 2, nz))
    a[1:-1, 1:-1, :] = interior
    return a


def apply_A(be, lev, x):
    """A x on the interior: compute_residual with b = 0 and the halo of p filled; leaves p = x there"""
    be.set_p_b(lev, _with_halo(be, lev, x), np.zeros(_with_halo(be, lev, x).shape))
    return -be.residual(lev)


def _start(be, lev, rng):
    """p* ~ N(0, 1) in every cell and b = A p*"""
    nx, ny, nz = be.dims(lev)
    ps = rng.standard_normal((nx, ny, nz))
    return ps, _with_halo(be, lev, apply_A(be, lev, ps))


def fixed_point(be, lev, seed):
    """check 1 -> the defect"""
    ps, b = _start(be, lev, np.random.default_rng([1, lev, seed]))
    be.set_p_b(lev, _with_halo(be, lev, ps), b)
    be.relax(lev, 2)
    return float(np.abs(be.p(lev) - ps).max() / np.abs(ps).max())


def first_colour(be, lev, seed, method, real):
    """check 2 -> (the defect, the control: the same with delta on the last colour)"""
    nx, ny, nz = be.dims(lev)
    rng = np.random.default_rng([2, lev, seed])
    ps, b = _start(be, lev, rng)
    first, last, _ = colour_sets(method, nx, ny)
    # delta: per column a constant in k of random sign and size 1 .. 2, plus a tenth of N(0, 1) in every cell.  What the control needs is
    # the part the neighbours feel: a column answers a vertically smooth error of its neighbour (the weak modes of T) and all but ignores
    # a rough one where the cells are thin (delta ~ N(0, 1) per cell: the control fell to 1.3e-3 on the 6x4x3 level of the stretched
    # coordinate); and on a 4x4 level the last colour of the set is ONE column, whose delta must not be small by the luck of a draw
    delta = rng.choice([-1.0, 1.0], (nx, ny, 1)) * rng.uniform(1.0, 2.0, (nx, ny, 1)) + 0.1 * rng.standard_normal((nx, ny, nz))
    if method == "RB" and real:
        delta[:, :, 0] = 0.0
    out = []
    for cols in (first, last):
        be.set_p_b(lev, _with_halo(be, lev, ps + delta * cols[:, :, None]), b)
        be.relax(lev, 1)
        out.append(float(np.abs(be.p(lev) - ps).max() / np.abs(ps).max()))
    return tuple(out)


def last_colour(be, lev, seed, method, real):
    """check 3 -> dict: defect (the last colour's residual), others (control), row1 (control, red-black 'real' only, else None), and
    p_over_Ap = max|p| / max|A p| of the relaxed p (the unit change of the sequential-order bound)"""
    nx, ny, nz = be.dims(lev)
    rng = np.random.default_rng([3, lev, seed])
    p0 = rng.standard_normal((nx, ny, nz))
    # |b| ~ |A p| of the RELAXED p: one pass with b = 0 wipes the rough p0 out of every column, and what A p is left with (the other
    # colours' later changes) is the size b gets.  A b of the size of A p0 would set the unit by the thin top rows of a stretched
    # coordinate and push the control on the other colours to its threshold (8.8e-3 on the 6x4x3 level of the stretched case).
    be.set_p_b(lev, _with_halo(be, lev, p0), np.zeros((nx + 2, ny + 2, nz)))
    be.relax(lev, 1)
    scale = float(np.sqrt((be.residual(lev) ** 2).mean()))
    assert scale > 0.0
    b = _with_halo(be, lev, rng.standard_normal((nx, ny, nz)) * scale)
    be.set_p_b(lev, _with_halo(be, lev, p0), b)
    be.relax(lev, 1)
    p = be.p(lev)
    r = be.residual(lev)
    assert not np.array_equal(p, p0)
    unit = float(np.abs(b[1:-1, 1:-1, :] - r).max())
    _, last, others = colour_sets(method, nx, ny)
    k0 = 1 if (method == "RB" and real) else 0
    return dict(defect=float(np.abs(r[last][:, k0:]).max()) / unit, others=float(np.abs(r[others]).max()) / unit,
                row1=float(np.abs(r[last][:, 0]).max()) / unit if k0 else None, p_over_Ap=float(np.abs(p).max()) / unit)


def norm_bound(cA, real):
    """an upper bound of ||A||_inf from the level's eight stored slots: a row holds slot 1 once and each of the slots 2..8 at most twice
    (the matrix is symmetric, a slot is one of a pair of mirrored couplings); the bottom row of cmatrix = 'real' holds 5 and 8 twice more"""
    m = [float(np.abs(cA[..., s]).max()) for s in range(8)]
    return m[0] + 2.0 * sum(m[1:]) + (2.0 * (m[4] + m[7]) if real else 0.0)


def run_level(be, lev, method, real, seed, rb_seq=False):
    """every check the level takes -> dict of figures (None where the check does not apply) and "tol": the bounds of this level"""
    nx, ny, nz = be.dims(lev)
    f = dict(dims=(nx, ny, nz), c1=fixed_point(be, lev, seed), c2=None, k2=None, c3=None, k3=None, row1=None)
    tol = {1: RB_SEQ_TOL, 2: RB_SEQ_TOL, 3: TOL[3]} if rb_seq else dict(TOL)
    if method != "GS" and nx >= 4 and ny >= 4:
        f["c2"], f["k2"] = first_colour(be, lev, seed, method, real)
        l = last_colour(be, lev, seed, method, real)
        f.update(c3=l["defect"], k3=l["others"], row1=l["row1"])
        if rb_seq:
            tol[3] = max(TOL[3], RB_SEQ_TOL * l["p_over_Ap"] * norm_bound(be.cA(lev), real))
    f["tol"] = tol
    return f


def assert_level(f, what):
    """the bounds and the controls on run_level's figures"""
    tol = f["tol"]
    assert f["c1"] <= tol[1], (what, "check 1: relax moved the fixed point", f)
    if f["c2"] is None:
        return
    assert f["c2"] <= tol[2], (what, "check 2: the first colour did not restore p*", f)
    assert f["k2"] > CONTROL_2, (what, "control of check 2", f)
    assert f["c3"] <= tol[3], (what, "check 3: the last colour kept a residual", f)
    assert f["k3"] > CONTROL_3, (what, "control of check 3", f)
    assert f["row1"] is None or f["row1"] > CONTROL_ROW1, (what, "control of check 3, row k = 1", f)


# ---- the nearest transfers ----
def even_fine_pairs(be):
    return [lev for lev in range(1, be.nlevs()) if be.dims(lev)[2] % 2 == 0]


def adjoint_defect(be, lev, seed):
    """|<R r, q> - <r, P q>| / (||r|| ||P q||) on the pair (lev, lev + 1), r and q ~ N(0, 1) on the interiors, sums in longdouble (the
    scale is the one of Cauchy-Schwarz: <r, P q> itself is a sum of random signs and can be small by luck).  The restriction runs first
    and the prolongation then writes into the fine r that holds r, as in a cycle: what it does not write keeps r."""
    rng = np.random.default_rng([4, lev, seed])
    r = rng.standard_normal(be.dims(lev)); q = rng.standard_normal(be.dims(lev + 1))
    Rr = be.restrict(lev, r)
    Pq = be.prolong(lev, q)
    assert np.abs(Rr).max() > 0 and np.abs(Pq).max() > 0
    return abs(inner(Rr, q) - inner(r, Pq)) / np.sqrt(inner(r, r) * inner(Pq, Pq))


# ---- the backends ----
class OracleBackend:
    """the calls on the CPU oracle: how the bounds asserted on the GPU were measured"""

    def __init__(self, o):
        self.o = o

    def nlevs(self):
        return self.o.nlevs

    def dims(self, lev):
        li = self.o.level_info(lev)
        return li["nx"], li["ny"], li["nz"]

    def set_p_b(self, lev, p, b):
        self.o.field("p", lev)[...] = p; self.o.field("b", lev)[...] = b
        self.o.fill_halo(lev, "p")

    def relax(self, lev, n):
        self.o.relax(lev, n)

    def residual(self, lev):
        self.o.residual(lev)
        return self.o.field("r", lev)[1:-1, 1:-1, :].copy()

    def p(self, lev):
        return self.o.field("p", lev)[1:-1, 1:-1, :].copy()

    def cA(self, lev):
        return self.o.field("cA", lev)

    def restrict(self, lev, r):
        """fine2coarse(lev): the fine r -> the interior of the coarse b"""
        f = self.o.field("r", lev)
        f[...] = 0.0; f[1:-1, 1:-1, :] = r
        self.o.fine2coarse(lev)
        return self.o.field("b", lev + 1)[1:-1, 1:-1, :].copy()

    def prolong(self, lev, q):
        """coarse2fine(lev): the coarse p -> the interior of the fine p, from p = 0 (p = p + r; the fine r is left as restrict() set it)"""
        c = self.o.field("p", lev + 1)
        c[...] = 0.0; c[1:-1, 1:-1, :] = q
        self.o.fill_halo(lev + 1, "p")
        self.o.field("p", lev)[...] = 0.0
        self.o.coarse2fine(lev)
        return self.o.field("p", lev)[1:-1, 1:-1, :].copy()


class GpuBackend:
    """the same calls on the library, through mg.grid(lev), mg.fill_halo, mg.relax, mg.compute_residual, mg.fine2coarse / coarse2fine"""

    def __init__(self, mg):
        self.mg = mg
        self._g = {}

    def g(self, lev):
        if lev not in self._g:
            self._g[lev] = self.mg.grid(lev)
        return self._g[lev]

    def nlevs(self):
        return self.mg.nlevs()

    def dims(self, lev):
        g = self.g(lev)
        return g.nx, g.ny, g.nz

    def set_p_b(self, lev, p, b):
        g = self.g(lev)
        g.set("p", p); g.set("b", b)
        self.mg.fill_halo(lev, "p")

    def relax(self, lev, n):
        self.mg.relax(lev, n)

    def residual(self, lev):
        self.mg.compute_residual(lev)
        return self.g(lev).get("r")[1:-1, 1:-1, :]

    def p(self, lev):
        return self.g(lev).get("p")[1:-1, 1:-1, :]

    def cA(self, lev):
        return self.g(lev).get("cA")

    def restrict(self, lev, r):
        F, C = self.g(lev), self.g(lev + 1)
        f = np.zeros(F._shape("r")); f[1:-1, 1:-1, :] = r
        F.set("r", f)
        self.mg.fine2coarse(lev)
        return C.get("b")[1:-1, 1:-1, :]

    def prolong(self, lev, q):
        F, C = self.g(lev), self.g(lev + 1)
        c = np.zeros(C._shape("p")); c[1:-1, 1:-1, :] = q
        C.set("p", c); self.mg.fill_halo(lev + 1, "p")
        F.set("p", np.zeros(F._shape("p")))
        self.mg.coarse2fine(lev)
        return F.get("p")[1:-1, 1:-1, :]


# ---- the cases: asserted on the GPU (tests/test_gpu_smoother_identity.py), measured on the oracle (tests/test_oracle.py) ----
# options: set_option after the set-up; init: the options mgx_init reads (no oracle has such a hierarchy); stored: run the case again after
# g.set("cA", g.get("cA")), which makes level 1 read the stored slots; moved: {read-only counter: levels on which it must have grown,
# or None = on some level}; still: counters that must not move
# fewer_than: options under which relax(1, 1) must take MORE launches than under the case's own (the evidence of a fused launch)
Case = collections.namedtuple("Case", "name dims method cmatrix geom bmask stretched curvilinear options init stored moved still fewer_than",
                              defaults=("FC", "real", "seamount", False, False, False, None, None, False, None, None, None))


def _fc(dims, what, **kw):
    return [Case("FC-%s-%dx%dx%d%s" % ((c,) + tuple(dims) + (what,)), tuple(dims), "FC", c, **kw) for c in ("real", "simple")]


def _route_name(o):
    return "window" if o["rbseq_window"] else "walk_apply" if o["rbseq_fuse"] else "scan_apply"


def _cases():
    from _switch_cases import WINDOW_ROUTES
    c = []
    # four colours, cmatrix real and simple
    c += _fc((16, 16, 8), "")                      # the one-workgroup kernels at 8x8x4 and 4x4x2
    c += _fc((32, 32, 8), "")                      # k-split nz = 8, colour pair, persistent relax
    c += _fc((32, 32, 64), "")                     # ks 64 / 32 / 16, 4x4x8
    c += _fc((64, 32, 64), "", stored=True)        # matrix-free k_relax_nz<64> with gam in LDS; again on the stored slots
    c += _fc((32, 160, 16), "")                    # ragged half-rows of 80 columns in two j-chunks
    c += _fc((32, 32, 48), "")                     # register instances 48, 24, 12; generic 6, 3
    c += _fc((32, 32, 40), "")                     # register instances 40, 20; generic 10, 5
    c += _fc((16, 160, 80), "")                    # tall matrix-free; 40; 20
    c += _fc((16, 32, 128), "") + _fc((16, 32, 96), "")   # tall
    # four colours, further cases
    c.append(Case("FC-32x32x24-small_any_nz=0", (32, 32, 24), options={"small_any_nz": 0}, still=("small_any_nz_calls",)))
    c.append(Case("FC-32x32x24-small_any_nz=1", (32, 32, 24), options={"small_any_nz": 1}, moved={"small_any_nz_calls": (3, 4)}))
    c.append(Case("FC-island-32x32x8", (32, 32, 8), bmask=True))
    c.append(Case("FC-island-32x32x96", (32, 32, 96), bmask=True, moved={"tall_stored_passes": (1,)}))
    c.append(Case("FC-rndtopo-island-stretched-24x16x12", (24, 16, 12), geom="rndtopo", bmask=True, stretched=True))
    c.append(Case("FC-curvilinear-32x16x8", (32, 16, 8), curvilinear=True))
    # hold_odd_nz: 32x32x40 ends at 4x4x5 (the horizontal bound) with or without the option; the held levels of nz = 5 are those of
    # 32x32x10 > 16x16x5 > 8x8x5 > 4x4x5
    c.append(Case("FC-hold_odd_nz-32x32x40", (32, 32, 40), init={"hold_odd_nz": 1}))
    c.append(Case("FC-hold_odd_nz-32x32x10", (32, 32, 10), init={"hold_odd_nz": 1}))
    c.append(Case("FC-periodic=3-32x32x16", (32, 32, 16), init={"periodic": 3}))           # the ring rule as it is: it excludes more than it must
    # red-black, cmatrix = 'real': every correction route of the sequential order at speed; the plane loop; the parallel sweep
    for dims in ((16, 256, 8), (16, 160, 16), (32, 32, 8)):
        for o in WINDOW_ROUTES:
            c.append(Case("RB-real-%dx%dx%d-%s" % (dims + (_route_name(o),)), dims, "RB", options=dict(o),
                          moved={"rbseq_window_colours": (1,)} if o["rbseq_window"] else None,
                          still=None if o["rbseq_window"] else ("rbseq_window_colours",)))
    c.append(Case("RB-real-32x512x16-fused", (32, 512, 16), "RB", options={"rbseq_fuse_min": 0, "rbseq_window": 0, "rbseq_fuse": 1},
                  still=("rbseq_window_colours",), fewer_than={"rbseq_fuse": 0}))
    c.append(Case("RB-real-32x32x8-rb_exact", (32, 32, 8), "RB", options={"rb_exact": 1}))
    c.append(Case("RB-real-32x32x8-rb_seq=0", (32, 32, 8), "RB", options={"rb_seq": 0}))
    c.append(Case("RB-real-64x64x48", (64, 64, 48), "RB"))                                  # the row-cut cases of test_rb_default_relax_every_level
    c.append(Case("RB-real-island-32x32x128", (32, 32, 128), "RB", bmask=True))
    # red-black, cmatrix = 'simple'
    for dims in ((16, 16, 8), (128, 128, 8), (32, 32, 24)):                                 # 128x128x8: the 1024-thread k_relax_reg<2>
        c.append(Case("RB-simple-%dx%dx%d" % dims, dims, "RB", "simple"))
    # Gauss-Seidel: check 1 only
    c.append(Case("GS-32x16x8", (32, 16, 8), "GS"))                                         # k_relax_gs_front
    c.append(Case("GS-16x16x24", (16, 16, 24), "GS"))                                       # k_relax_gs_front_any
    return c


CASES = _cases()
ADJOINT_DIMS = [(16, 16, 8), (32, 16, 24), (64, 96, 32), (32, 32, 12)]
HELD_DIMS = [(32, 32, 40), (32, 32, 10)]   # under hold_odd_nz: 32x32x40 ends at 4x4x5 and has NO held pair; 32x32x10 > 16x16x5 > 8x8x5 > 4x4x5 has two
ODD_PAIR_DIMS = (64, 64, 20)     # 64x64x20 > 32x32x10 > 16x16x5 > 8x8x2: the pair 5 -> 2


def is_rb_seq(case):
    """the sequential order at speed: red-black, cmatrix = 'real', neither the plane loop nor the parallel sweep"""
    o = case.options or {}
    return case.method == "RB" and case.cmatrix == "real" and not o.get("rb_exact") and o.get("rb_seq", 1) == 1


def case_problem(case, **par):
    """the record (tests/_problem.py) of a case: what gpu_problem hands to the library and oracle_twin to the oracle"""
    from _problem import SIGMA, problem
    nx, ny, _ = case.dims
    zeta, sigma = None, SIGMA
    if case.stretched:    # the stretched coordinate under a rough free surface, as tests/_operator_identity.py::case_inputs
        zeta, sigma = 0.3 * np.random.default_rng(99).standard_normal((nx + 2, ny + 2)), (250.0, 0.4, 6.0)
    return problem(case.dims, geom=case.geom, bmask=case.bmask, zeta=zeta, sigma=sigma, metric="curvilinear" if case.curvilinear else "uniform",
                   relax_method=case.method, cmatrix=case.cmatrix, **par)


def oracle_cases():
    """the cases an oracle exists for, one per problem (the options choose kernels, not another operator)"""
    seen, out = set(), []
    for c in CASES:
        key = (c.dims, c.method, c.cmatrix, c.geom, c.bmask, c.stretched, c.curvilinear)
        if c.init or key in seen:
            continue
        seen.add(key)
        out.append(c)
    return out
