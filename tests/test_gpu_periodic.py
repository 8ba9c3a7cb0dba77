"""Option "periodic" on the GPU (include/mgx.h; DESIGN.md sections 1 and 5): east-west and north-south wrap on a single rank.

A periodic side is an open side whose neighbour is the rank itself, so nothing here is compared with the CPU oracle, which has closed
walls only.  What is asserted instead:

  1  the halo rule, cell by cell, against a numpy construction (np.pad: "wrap" along periodic axes, the closed rule along the others)
  2  shift equivariance, bit for bit: a cyclic roll of every input along a periodic direction rolls every output (moving the seam is a
     shift, and the kernels are decomposition-independent bit for bit already)
  3  the operator identity compute_rhs(correct_uvw(0; p)) = -A p ACROSS the seam, with no exclusion ring in a periodic direction
  4  a converged solve of mirror-symmetric data: the wrap seam is a symmetry plane of the same standing as the interior one
  5  a land wall across the seam ties a periodic solve to a closed one
  6  red-black in the sequential order at speed against the plane loop on every level
  7  the device-resident time step
  8  the refusals, 9 the launch counts with the option off

Geometry of every case: no symmetry, nothing constant along a periodic direction -- a seamount centred at 0.3 Lx, 0.4 Ly in the wrapped
distance, 2 % uniform roughness from a seeded generator on top, dx = dx0 (1 + 0.1 sin(2 pi i / nx)) and dy likewise in j."""
import numpy as np
import pytest

from _gpu import gpu_module
from _operator_identity import COUPLING_TOL, MIN_FRACTION, MIN_LAND, scaled_defect, velocities, inner

pytestmark = pytest.mark.gpu

HC = 4e3
SYM_TOL = 1e-12
HIST_TOL = 1e-13   # residual histories of two runs whose norms are summed in another order


mg = gpu_module(periodic=0, rb_seq=1, rb_exact=0, krylov=0, krylov_precision=64, cycle_precision=64, warm_start=0,
                **{"async": 0})   # (a Python keyword)


def _init(mg, dims, per, monkeypatch=None, stored=False, **par):
    """mgx_init reads the option: clean, set, init"""
    if monkeypatch is not None:
        if stored:
            monkeypatch.setenv("MGX_NO_MF", "1")   # read by every nhydro_init: the stored slots instead of the in-kernel coefficients
        else:
            monkeypatch.delenv("MGX_NO_MF", raising=False)
    mg.nhydro_clean()
    mg.nhydro.set_option("periodic", per)
    par.setdefault("relax_method", "FC")
    mg.nhydro_init(*dims, 1, 1, 0, mg.nhydro.default_params(**par))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _pad(a, per, ax_i, ax_j, n=1, closed="edge", **kw):
    """halo of n cells around the interior a: the periodic axes first ("wrap"), then the closed ones (`closed`), so that a corner between a
    periodic and a closed side is the closed side's image of the wrapped edge"""
    for periodic_pass in (True, False):
        for ax, bit in ((ax_i, 1), (ax_j, 2)):
            if bool(per & bit) != periodic_pass:
                continue
            w = [(0, 0)] * a.ndim
            w[ax] = (n, n)
            a = np.pad(a, w, mode="wrap") if per & bit else np.pad(a, w, mode=closed, **kw)
    return a


def _wrapped(x, c, periodic):
    d = x - c
    return d - np.round(d) if periodic else d


def geometry(nx, ny, per, stretched=False, seed=7, island=False, curvilinear=False):
    """interiors (nx, ny) of dx, dy, zeta, h and, with `island`, of a mask whose island straddles the seam(s).  curvilinear: dx(i,j),
    dy(i,j) -- each varies in both directions, with whole wave numbers over nx and ny, so that it is periodic in whichever direction
    wraps; not separable, and dy is no transpose or shift of dx"""
    rng = np.random.default_rng(seed)
    x = (np.arange(1, nx + 1) - 0.5) / nx
    y = (np.arange(1, ny + 1) - 0.5) / ny
    ex = _wrapped(x, 0.3, per & 1)[:, None] / 0.2
    ey = _wrapped(y, 0.4, per & 2)[None, :] / 0.2
    h = 4e3 * (1.0 - 0.5 * np.exp(-ex ** 2 - ey ** 2)) * (1.0 + 0.02 * (2.0 * rng.random((nx, ny)) - 1.0))
    dx = np.repeat((1e4 / nx * (1.0 + 0.1 * np.sin(2 * np.pi * np.arange(1, nx + 1) / nx)))[:, None], ny, axis=1)
    dy = np.repeat((1e4 / ny * (1.0 + 0.1 * np.sin(2 * np.pi * np.arange(1, ny + 1) / ny)))[None, :], nx, axis=0)
    if curvilinear:
        ti = (2 * np.pi * np.arange(1, nx + 1) / nx)[:, None]
        tj = (2 * np.pi * np.arange(1, ny + 1) / ny)[None, :]
        dx = dx * (1.0 + 0.08 * np.sin(2 * ti + tj + 0.7) + 0.04 * np.cos(3 * tj))
        dy = dy * (1.0 + 0.08 * np.cos(ti - 2 * tj + 0.3) + 0.04 * np.sin(3 * ti))
    zeta = 0.3 * rng.standard_normal((nx, ny)) if stretched else np.zeros((nx, ny))
    g = dict(dx=dx, dy=dy, zeta=zeta, h=h, rmask=None, hc=250.0 if stretched else HC, theta_b=0.4 if stretched else 0.0, theta_s=6.0 if stretched else 0.0)
    if island:
        ci = 0.0 if per & 1 else 0.3   # centred ON a periodic seam (between the last and the first column)
        cj = 0.0 if per & 2 else 0.6
        x0, y0 = np.arange(1, nx + 1) - 0.5, np.arange(1, ny + 1) - 0.5
        di = nx * _wrapped(x0 / nx, ci, per & 1)[:, None]
        dj = ny * _wrapped(y0 / ny, cj, per & 2)[None, :]
        g["rmask"] = np.where(di ** 2 + dj ** 2 <= (0.15 * min(nx, ny)) ** 2, 0.0, 1.0)
    return g


def full2d(g, per, poison=False):
    """the (nx+2, ny+2) arrays nhydro_matrices takes.  poison: not-a-numbers in the halo entries of a periodic direction, which the
    library has to ignore (it replaces them by the wrapped interior)"""
    out = {}
    for name in ("dx", "dy", "zeta", "h", "rmask"):
        if g[name] is None:
            out[name] = None
            continue
        a = _pad(g[name], per, 0, 1) if name != "rmask" else _pad(g[name], per, 0, 1, closed="constant", constant_values=0.0)
        if poison:
            if per & 1:
                a[0, :] = a[-1, :] = np.nan
            if per & 2:
                a[:, 0] = a[:, -1] = np.nan
        out[name] = a
    return out


def matrices(mg, g, per, poison=False):
    f = full2d(g, per, poison)
    mg.nhydro_matrices(f["dx"], f["dy"], f["zeta"], f["h"], f["rmask"], g["hc"], g["theta_b"], g["theta_s"])
    return f


def velocity_bases(nx, ny, nz, per, seed):
    """u, v, w without their duplicates: faces 1..nx of u in a periodic i direction (face nx+1 IS face 1), all nx+1 otherwise; cells only"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nz, ny, nx if per & 1 else nx + 1)), rng.standard_normal((nz, ny if per & 2 else ny + 1, nx)),
            rng.standard_normal((nz + 1, ny, nx)))


def velocities_from(bases, per):
    """u (nz, ny+2, nx+1), v (nz, ny+1, nx+2), w (nz+1, ny+2, nx+2) as a model hands them over after its own exchange: halo columns in a
    periodic direction hold the wrapped values, u(nx+1) = u(1), v(ny+1) = v(1)"""
    ub, vb, wb = bases
    u = np.concatenate([ub, ub[:, :, :1]], axis=2) if per & 1 else ub
    v = np.concatenate([vb, vb[:, :1, :]], axis=1) if per & 2 else vb
    u = np.pad(u, [(0, 0), (1, 1), (0, 0)], mode="wrap" if per & 2 else "edge")       # the j halo of u
    v = np.pad(v, [(0, 0), (0, 0), (1, 1)], mode="wrap" if per & 1 else "edge")       # the i halo of v
    w = _pad(wb, per, 2, 1)
    return np.ascontiguousarray(u), np.ascontiguousarray(v), np.ascontiguousarray(w)


def velocity_base_views(u, v, w, per):
    nx, ny = w.shape[2] - 2, w.shape[1] - 2
    return (u[:, 1:-1, :nx] if per & 1 else u[:, 1:-1, :], v[:, :ny, 1:-1] if per & 2 else v[:, :, 1:-1], w[:, 1:-1, 1:-1])


# ---- 1. the halo rule --------------------------------------------------------------------------------------------------------------
def _coded(shape):
    return np.arange(1.0, np.prod(shape) + 1.0).reshape(shape)


def _fill(mg, lev, name, a):
    g = mg.grid(lev)
    g.set(name, a)
    c0 = mg.nhydro.counters()
    mg.fill_halo(lev, name)
    c1 = mg.nhydro.counters()
    return g.get(name), c1["launches"] - c0["launches"], c1["halo_fills"] - c0["halo_fills"]


@pytest.mark.parametrize("dims", [(32, 16, 8), (64, 32, 64)], ids=["32x16x8", "64x32x64"])
def test_halo_rule(mg, dims):
    """A position-coded field through grid(lev).set, fill_halo(lev, name), read back: every halo cell, corners included, on every level,
    for periodic = 1, 2, 3.  p, b, r, dx, h: np.pad of the interior, "wrap" along the periodic axes, then "edge" along the closed ones.
    zr, zw (two halo columns): the closed rule is the existing extrapolation, taken from the periodic = 0 run of the same field; its rows
    and planes wrap whole, and a corner between a periodic and a closed side is the reference's mixed-corner rule, which rl_fill_halo
    applies from neighb[] as on a process grid: the closed side's MIRROR of the wrapped columns (j = 0 <- 1, j = -1 <- 2).
    cA: fill_halo_4D's rule -- an exchange and nothing else, so a closed direction keeps what was set there ("in a closed direction
    nothing changes": with periodic = 0 the call does nothing) and whole rows and planes wrap.
    One launch per halo fill of a solver field (k_halo_wrap, which also stores the closed sides' images when they are due)."""
    names = ("p", "b", "r", "dx", "h", "zr", "zw", "cA")
    _init(mg, dims, 0)
    matrices(mg, geometry(*dims[:2], 0), 0)
    nlev = mg.nlevs()
    closed = {(lev, name): _fill(mg, lev, name, _coded(mg.grid(lev)._shape(name)))[0] for lev in range(1, nlev + 1) for name in ("zr", "zw")}
    for per in (1, 2, 3):
        _init(mg, dims, per)
        matrices(mg, geometry(*dims[:2], per), per)
        assert mg.nlevs() == nlev
        for lev in range(1, nlev + 1):
            g = mg.grid(lev)
            nx, ny = g.nx, g.ny
            for name in names:
                a = _coded(g._shape(name))
                got, launches, fills = _fill(mg, lev, name, a)
                if name in ("zr", "zw"):
                    want = closed[lev, name].copy()
                    if per & 1:
                        want[:2] = want[nx:nx + 2]; want[nx + 2:] = want[2:4]
                        if not per & 2:   # mixed corners: the mirror of the wrapped columns
                            for sl in (slice(0, 2), slice(nx + 2, nx + 4)):
                                want[sl, 1] = want[sl, 2]; want[sl, 0] = want[sl, 3]; want[sl, ny + 2] = want[sl, ny + 1]; want[sl, ny + 3] = want[sl, ny]
                    if per & 2:
                        want[:, :2] = want[:, ny:ny + 2]; want[:, ny + 2:] = want[:, 2:4]
                        if not per & 1:
                            for sl in (slice(0, 2), slice(ny + 2, ny + 4)):
                                want[1, sl] = want[2, sl]; want[0, sl] = want[3, sl]; want[nx + 2, sl] = want[nx + 1, sl]; want[nx + 3, sl] = want[nx, sl]
                    if per == 3:
                        want = _pad(a[2:-2, 2:-2], 3, 0, 1, n=2)
                elif name == "cA":
                    want = a.copy()
                    if per & 1:
                        want[0] = want[nx]; want[nx + 1] = want[1]
                    if per & 2:
                        want[:, 0] = want[:, ny]; want[:, ny + 1] = want[:, 1]
                else:
                    want = _pad(a[1:-1, 1:-1], per, 0, 1)
                assert np.array_equal(got, want), (per, lev, name, np.argwhere(got != want)[:4])
                if name in ("p", "b", "r"):
                    assert (launches, fills) == (1, 1), (per, lev, name, launches, fills)
                if name == "cA":
                    assert (launches, fills) == (8, 8), (per, lev, launches, fills)


def test_level_info_and_transport(mg):
    from mgroms_amd._lib import lib
    for per, want, word in ((0, [-1] * 8, "none (one rank)"), (1, [-1, 0, -1, 0, -1, -1, -1, -1], "none (one rank; periodic i: local wrap)"),
                            (2, [0, -1, 0, -1, -1, -1, -1, -1], "none (one rank; periodic j: local wrap)"), (3, [0] * 8, "none (one rank; periodic ij: local wrap)")):
        _init(mg, (32, 16, 8), per)
        for lev in range(1, mg.nlevs() + 1):
            assert mg.grid(lev).neighb == want, (per, lev, mg.grid(lev).neighb)
        assert lib().mgx_transport().decode() == word


# ---- 2. shift equivariance ---------------------------------------------------------------------------------------------------------
def _roll_inputs(g, bases, s, axis):
    """every input rolled by s cells along i (axis 0) or j (axis 1)"""
    g2 = dict(g)
    for name in ("dx", "dy", "zeta", "h", "rmask"):
        if g[name] is not None:
            g2[name] = np.roll(g[name], s, axis=axis)
    return g2, tuple(np.roll(b, s, axis=2 - axis) for b in bases)   # model arrays: (k, j, i)


def _outputs(mg, dims, per, g, bases, poison):
    matrices(mg, g, per, poison)
    out = {"cA": [mg.grid(lev).cA[1:-1, 1:-1] for lev in range(1, mg.nlevs() + 1)]}
    u, v, w = velocities_from(bases, per)
    mg.nhydro.compute_rhs(u, v, w)
    out["b"] = mg.grid(1).b[1:-1, 1:-1]
    n, out["hist"] = mg.solve_p(1e-30, 3)
    assert n == 3
    out["p"] = mg.grid(1).p[1:-1, 1:-1]
    mg.nhydro_solve(u, v, w)
    nx, ny = dims[:2]
    if per & 1:
        assert np.array_equal(u[:, :, nx], u[:, :, 0])   # the duplicated faces come back equal bit for bit
    if per & 2:
        assert np.array_equal(v[:, ny, :], v[:, 0, :])
    out["uvw"] = velocity_base_views(u, v, w, per)
    return out


SHIFT_CASES = [
    # dims, periodic, axis of the shift, s, stored, island, stretched, red-black
    ((32, 16, 8), 1, 0, 8, False, False, False, False),
    ((32, 16, 8), 2, 1, 8, False, False, False, False),
    ((32, 16, 8), 3, 0, 8, True, False, False, False),
    ((32, 16, 8), 3, 1, 8, False, True, False, False),
    ((32, 32, 24), 1, 0, 16, True, False, False, False),
    ((32, 32, 24), 2, 1, 16, False, False, True, False),
    ((32, 32, 24), 3, 0, 16, False, True, True, False),
    ((64, 32, 64), 3, 0, 16, False, False, False, False),
    ((64, 32, 64), 1, 0, 16, False, True, False, False),
    ((64, 32, 64), 2, 1, 16, True, False, False, False),
    ((32, 16, 8), 3, 0, 8, False, False, False, True),
    ((32, 32, 24), 2, 1, 16, False, False, False, True),
    ((64, 32, 64), 1, 0, 16, False, False, False, True),
    # a ninth entry: dx(i,j), dy(i,j), periodic in both directions (geometry(curvilinear=True))
    ((32, 16, 8), 3, 1, 8, False, False, False, False, True),
    ((64, 32, 64), 3, 0, 16, False, False, False, False, True),
]


def _shift_id(c):
    d, per, ax, s, stored, island, stretched, rb = c[:8]
    return "%dx%dx%d-per%d-%s%d%s%s%s%s%s" % (*d, per, "ij"[ax], s, "-stored" if stored else "", "-island" if island else "", "-stretched" if stretched else "", "-rb" if rb else "",
                                            "-curvilinear" if c[8:] == (True,) else "")


@pytest.mark.parametrize("case", SHIFT_CASES, ids=[_shift_id(c) for c in SHIFT_CASES])
def test_shift_equivariance(mg, case, monkeypatch):
    """Every input rolled by s along a periodic direction, s / 2^(lev-1) a whole and EVEN number of cells on every level, the coarsest included,
    so that coarse cells and colours keep their place: s = 8 at 32 x 16 x 8 (three levels), s = 16 at 64 x 32 x 64 and at 32 x 32 x 24 (four
    levels each: 24, 12, 6, 3 rows; with s = 8 the coarsest level, 4 x 4 x 3, is shifted by one cell, its colours change places and p, not cA or
    b, differs in the last bits).  The eight cA slots of every level (rolled by s / 2^(lev-1)), b, p after three solve_p iterations and u, v, w after nhydro_solve
    come out rolled, np.array_equal on interiors; the residual histories agree within 1e-13 relative (the norm is summed in another order).
    Four colours, matrix-free and stored slots (MGX_NO_MF, which every nhydro_init reads), bmask with an island that straddles the seam, the
    stretched coordinate, both directions; red-black as the snapshot pass (rb_seq = 0, rb_exact = 0: the sequential order is not shift
    invariant).  The first run's inputs carry not-a-numbers in the halo entries of the periodic directions: they are ignored."""
    dims, per, axis, s, stored, island, stretched, rb = case[:8]
    curvilinear = case[8:] == (True,)
    nx, ny, nz = dims
    mg.nhydro_clean()
    mg.nhydro.set_option("rb_seq", 0 if rb else 1); mg.nhydro.set_option("rb_exact", 0)
    try:
        _init(mg, dims, per, monkeypatch, stored, relax_method="RB" if rb else "FC", solver_prec=1e-30, solver_maxiter=3, bmask=1 if island else 0)
        nlev = mg.nlevs()
        assert s % (1 << nlev) == 0 and per & (1 << axis)
        g = geometry(nx, ny, per, stretched, island=island, curvilinear=curvilinear)
        bases = velocity_bases(nx, ny, nz, per, 11)
        a = _outputs(mg, dims, per, g, bases, poison=True)
        g2, bases2 = _roll_inputs(g, bases, s, axis)
        _init(mg, dims, per, monkeypatch, stored, relax_method="RB" if rb else "FC", solver_prec=1e-30, solver_maxiter=3, bmask=1 if island else 0)
        b = _outputs(mg, dims, per, g2, bases2, poison=False)
    finally:
        mg.nhydro_clean()
        mg.nhydro.set_option("rb_seq", 1)
    assert np.abs(a["p"]).max() > 0 and not np.array_equal(a["p"], b["p"])
    for lev in range(nlev):
        assert np.array_equal(np.roll(a["cA"][lev], s >> lev, axis=axis), b["cA"][lev]), ("cA", lev + 1)
    for name in ("b", "p"):
        assert np.array_equal(np.roll(a[name], s, axis=axis), b[name]), name
    for name, x, y in zip("uvw", a["uvw"], b["uvw"]):
        assert np.array_equal(np.roll(x, s, axis=2 - axis), y), name
    print(_shift_id(case), "hist", a["hist"], "rel", np.abs(a["hist"] - b["hist"]) / a["hist"])
    assert np.all(np.abs(a["hist"] - b["hist"]) <= HIST_TOL * a["hist"])


# ---- 3. the operator identity across the seam ---------------------------------------------------------------------------------------
def periodic_set(rmask, nx, ny, per):
    """water_interior's rule with the wrap: the columns whose wrapped 3 x 3 neighbourhood is water and that are outside the ring of a
    CLOSED direction only.  rmask: (nx+2, ny+2) with its periodic halos wrapped, or None."""
    m = np.ones((nx + 2, ny + 2), dtype=bool) if rmask is None else (np.asarray(rmask) != 0.0)
    sel = np.ones((nx, ny), dtype=bool)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            sel &= m[di:di + nx, dj:dj + ny]
    if not per & 1:
        sel[0, :] = sel[-1, :] = False
    if not per & 2:
        sel[:, 0] = sel[:, -1] = False
    return sel


def assert_periodic_set(sel, rmask, per):
    nx, ny = sel.shape
    assert sel.sum() >= MIN_FRACTION * nx * ny, (sel.sum(), nx * ny)
    if per & 1:
        assert sel[0, :].any() and sel[-1, :].any()     # the seam columns i = 1 and nx
        assert rmask is not None or (sel[0, 1:-1].all() and sel[-1, 1:-1].all())
    if per & 2:
        assert sel[:, 0].any() and sel[:, -1].any()     # j = 1 and ny
        assert rmask is not None or (sel[1:-1, 0].all() and sel[1:-1, -1].all())
    if rmask is not None:
        water = np.asarray(rmask)[1:-1, 1:-1] != 0.0
        ring = np.zeros((nx, ny), dtype=bool)
        if not per & 1:
            ring[0, :] = ring[-1, :] = True
        if not per & 2:
            ring[:, 0] = ring[:, -1] = True
        land, coast = int((~water & ~ring).sum()), int((water & ~ring & ~sel).sum())
        assert land >= MIN_LAND and coast >= 1, (land, coast)
        seam = np.concatenate([~water[0, :], ~water[-1, :]] if per & 1 else [~water[:, 0], ~water[:, -1]])
        assert seam.any()   # the island straddles the seam


def _direct_defect(mg, dims, sel, water, seed):
    """compute_rhs(correct_uvw(0; p)) against -A p = compute_residual(1) with b = 0, for a random p (zero on land).  The solver was
    initialised with solver_maxiter = 0 and "warm_start": nhydro_solve then is compute_rhs, no iteration, correct_uvw with the p given."""
    nx, ny, nz = dims
    g = mg.grid(1)
    p = np.zeros(g._shape("p"))
    p[1:-1, 1:-1] = np.random.default_rng(seed).standard_normal(dims) * water[:, :, None]
    g.set("p", p); mg.fill_halo(1, "p")
    u, v, w = (np.zeros(s) for s in ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2)))
    mg.nhydro_solve(u, v, w)
    assert np.abs(u).max() > 0 and np.abs(w).max() > 0 and np.array_equal(mg.grid(1).p[1:-1, 1:-1], p[1:-1, 1:-1])
    g.set("b", np.zeros(g._shape("b")))
    mg.compute_residual(1)
    mAp = g.r[1:-1, 1:-1]
    mg.nhydro.compute_rhs(u, v, w)
    return scaled_defect(g.b[1:-1, 1:-1], mAp, sel)


def _sequence_defect(mg, dims, per, sel, seed):
    """coupling_defect's sequence (tests/_operator_identity.py) through nhydro_solve, on the periodic set, the velocities as a model hands
    them over after its exchange"""
    nx, ny, nz = dims
    u0, v0, w0 = velocities(nx, ny, nz, seed)
    u0, v0, w0 = velocities_from(velocity_base_views(u0, v0, w0, per), per)   # wrapped halos, u(nx+1) = u(1); the closed halos: edge images
    u, v, w = u0.copy(), v0.copy(), w0.copy()
    mg.nhydro_solve(u, v, w)
    assert not np.array_equal(u, u0) and not np.array_equal(w, w0)
    mg.nhydro.compute_rhs(u0, v0, w0)
    b = mg.grid(1).b[1:-1, 1:-1]
    mg.compute_residual(1)
    r = mg.grid(1).r[1:-1, 1:-1]
    mg.nhydro.compute_rhs(u, v, w)
    b2 = mg.grid(1).b[1:-1, 1:-1]
    Ap = b - r
    assert np.abs(Ap[sel]).max() > 1e-3 * np.abs(b[sel]).max()
    return scaled_defect(b2, r, sel, b, Ap)


IDENTITY_CASES = [
    # dims, periodic, island, stretched, stored
    ((32, 16, 8), 1, False, False, False),
    ((32, 16, 8), 2, False, False, True),
    ((32, 16, 8), 3, True, False, False),
    ((32, 32, 24), 3, False, True, False),
    ((32, 32, 24), 1, True, True, False),
    ((64, 32, 64), 1, False, False, False),
    ((64, 32, 64), 2, True, False, False),
    ((64, 32, 64), 3, False, False, True),
    # a sixth entry: dx(i,j), dy(i,j), periodic in both directions (geometry(curvilinear=True))
    ((32, 16, 8), 3, False, False, True, True),
    ((64, 32, 64), 3, False, False, False, True),
    ((32, 32, 24), 1, True, True, False, True),
]


def _identity_id(c):
    d, per, island, stretched, stored = c[:5]
    return "%dx%dx%d-per%d%s%s%s%s" % (*d, per, "-island" if island else "", "-stretched" if stretched else "", "-stored" if stored else "",
                                       "-curvilinear" if c[5:] == (True,) else "")


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=[_identity_id(c) for c in IDENTITY_CASES])
def test_identity_across_the_seam(mg, case, monkeypatch):
    """No oracle call and no ring in a periodic direction: the set holds the seam columns.  The direct form and the sequence through
    nhydro_solve, both within COUPLING_TOL = 3.5e-14 (the CPU oracle keeps the identity to 4.5e-16 at an open seam of a 2 x 1
    decomposition on these geometries, as on the interior)."""
    dims, per, island, stretched, stored = case[:5]
    nx, ny, nz = dims
    g = geometry(nx, ny, per, stretched, island=island, curvilinear=case[5:] == (True,))
    if case[5:] == (True,):   # the metric varies along every row and every column
        assert all(np.ptp(g[n], axis=a).min() > 0 for n in ("dx", "dy") for a in (0, 1))
    rmask = full2d(g, per)["rmask"]
    sel = periodic_set(rmask, nx, ny, per)
    assert_periodic_set(sel, rmask, per)
    water = np.ones((nx, ny)) if rmask is None else rmask[1:-1, 1:-1]
    mg.nhydro_clean(); mg.nhydro.set_option("warm_start", 1)
    try:
        _init(mg, dims, per, monkeypatch, stored, solver_prec=1e-30, solver_maxiter=0, bmask=1 if island else 0)
        matrices(mg, g, per)
        d1 = _direct_defect(mg, dims, sel, water, 3)
    finally:
        mg.nhydro_clean(); mg.nhydro.set_option("warm_start", 0)
    _init(mg, dims, per, monkeypatch, stored, solver_prec=1e-30, solver_maxiter=2, bmask=1 if island else 0)
    matrices(mg, g, per)
    d2 = _sequence_defect(mg, dims, per, sel, 1)
    print(_identity_id(case), "direct", d1, "sequence", d2, "set", sel.mean())
    assert d1 <= COUPLING_TOL, ("direct", d1)
    assert d2 <= COUPLING_TOL, ("sequence", d2)


@pytest.mark.parametrize("per", [1, 2], ids=["i", "j"])
def test_a_perturbed_slot_on_a_seam_column_is_seen(mg, per, monkeypatch):
    """One slot of the level-1 cA scaled by 1 + 1e-6 on the seam columns i = 1 (j = 1) alone: the defect of the direct form exceeds
    1000 x the bound, for each of the eight slots in turn; with cA restored the identity holds again."""
    dims = (32, 32, 16)
    g = geometry(32, 32, per)
    sel = periodic_set(None, 32, 32, per)
    assert_periodic_set(sel, None, per)
    water = np.ones((32, 32))
    mg.nhydro_clean(); mg.nhydro.set_option("warm_start", 1)
    try:
        _init(mg, dims, per, monkeypatch, solver_prec=1e-30, solver_maxiter=0)
        matrices(mg, g, per)
        gr = mg.grid(1)
        cA = gr.get("cA")
        assert _direct_defect(mg, dims, sel, water, 6) <= COUPLING_TOL
        for slot in range(8):
            bad = cA.copy()
            if per == 1:
                bad[1, :, :, slot] *= 1.0 + 1e-6
            else:
                bad[:, 1, :, slot] *= 1.0 + 1e-6
            gr.set("cA", bad); mg.fill_halo(1, "cA")   # the wrapped image of the perturbed columns
            d = _direct_defect(mg, dims, sel, water, 6)
            print("periodic", per, "slot", slot + 1, d)
            assert d > 1000 * COUPLING_TOL, (slot, d)
        gr.set("cA", cA)
        assert _direct_defect(mg, dims, sel, water, 6) <= COUPLING_TOL
    finally:
        mg.nhydro_clean(); mg.nhydro.set_option("warm_start", 0)


@pytest.mark.parametrize("per,island", [(1, True), (3, False)], ids=["i-island-stored", "ij-matrix-free"])
def test_operator_is_symmetric_and_negative_across_the_seam(mg, per, island, monkeypatch):
    """A through compute_residual(1) with b = 0 on fields supported on the periodic set, seam columns included: <x, A y> = <A x, y> within
    1e-12 relative, <x, A x> < 0, sums in longdouble"""
    dims = (32, 32, 16)
    g = geometry(32, 32, per, stretched=True, island=island)
    rmask = full2d(g, per)["rmask"]
    sel = periodic_set(rmask, 32, 32, per)
    assert_periodic_set(sel, rmask, per)
    _init(mg, dims, per, monkeypatch, bmask=1 if island else 0)
    matrices(mg, g, per)
    gr = mg.grid(1)

    def apply(x):
        p = np.zeros(gr._shape("p")); p[1:-1, 1:-1, :] = x
        gr.set("p", p); mg.fill_halo(1, "p"); gr.set("b", np.zeros(gr._shape("b")))
        mg.compute_residual(1)
        return -gr.r[1:-1, 1:-1, :]

    rng = np.random.default_rng(5)
    x, y = (rng.standard_normal(dims) * sel[:, :, None] for _ in range(2))
    Ax, Ay = apply(x), apply(y)
    xAy, Axy = inner(x, Ay), inner(Ax, y)
    print("xAy", xAy, "Axy", Axy, "rel", abs(xAy - Axy) / abs(xAy), "xAx", inner(x, Ax), "yAy", inner(y, Ay))
    assert abs(xAy - Axy) <= SYM_TOL * abs(xAy)
    assert inner(x, Ax) < 0 and inner(y, Ay) < 0


# ---- 4. a converged solve of mirror-symmetric data ----------------------------------------------------------------------------------
def _true_residual(mg):
    b = mg.grid(1).b[1:-1, 1:-1]
    return mg.compute_residual(1) / np.sqrt(inner(b, b))


def test_converged_solve_and_mirror_symmetry(mg, monkeypatch):
    """periodic = 1, 64 x 32 x 8: a 32-wide block followed by its mirror image, u odd and the rest even, so the interior seam 32|33 and
    the wrap seam 64|1 are symmetry planes of equal standing.  Four colours to tol = 1e-11 in at most 300 iterations; compute_residual(1)
    / ||b|| confirms the reported residual; p(i) = p(65 - i) within 16 x 8.3e-13 = 1.3e-11 of max|p| (8.3e-13 is what the CPU oracle's
    closed, mirrored 64 x 32 x 8 solve shows at that tolerance: the sweep order is not mirror symmetric, the solution is).  The same
    solve with "krylov" = 4 reaches tol on the true residual.
    Measured on the MI355X: 21 iterations to 9.7e-12, asymmetry 1.12e-11 of max|p|; with "krylov" = 4: 12 iterations to 1.5e-12 (asymmetry 1.23e-11)."""
    nx, ny, nz, tol = 64, 32, 8, 1e-11
    blk = geometry(32, ny, 0)
    g = dict(blk)
    for name in ("dx", "dy", "zeta", "h"):
        g[name] = np.concatenate([blk[name], blk[name][::-1]], axis=0)
    rng = np.random.default_rng(21)
    ub = np.zeros((nz, ny, nx))                      # faces 1..64; faces 1 (= 65) and 33 are the symmetry planes: u = 0 there
    ub[:, :, 1:32] = rng.standard_normal((nz, ny, 31))
    ub[:, :, 33:64] = -ub[:, :, 31:0:-1]             # u(33 + m) = -u(33 - m)
    vb, wb = rng.standard_normal((nz, ny + 1, 32)), rng.standard_normal((nz + 1, ny, 32))
    vb, wb = np.concatenate([vb, vb[:, :, ::-1]], axis=2), np.concatenate([wb, wb[:, :, ::-1]], axis=2)
    u, v, w = velocities_from((ub, vb, wb), 1)
    try:
        for krylov in (0, 4):
            mg.nhydro_clean(); mg.nhydro.set_option("krylov", krylov)
            _init(mg, (nx, ny, nz), 1, monkeypatch)
            matrices(mg, g, 1)
            mg.nhydro.compute_rhs(u, v, w)
            n, hist = mg.solve_p(tol, 300)
            true = _true_residual(mg)
            P = mg.grid(1).p[1:-1, 1:-1]
            asym = np.abs(P - P[::-1]).max() / np.abs(P).max()
            print("krylov", krylov, "iterations", n, "reported", hist[-1], "true", true, "asymmetry", asym)
            assert n < 300 and hist[-1] <= tol, (n, hist[-1])
            assert abs(true - hist[-1]) <= 1e-10 * hist[-1] and true <= tol * (1 + 1e-9), (true, hist[-1])   # (the norm is summed in another order)
            if krylov == 0:
                assert asym <= 16 * 8.3e-13, asym
    finally:
        mg.nhydro_clean(); mg.nhydro.set_option("krylov", 0)


# ---- 5. a land wall across the seam ---------------------------------------------------------------------------------------------------
def test_land_wall_ties_periodic_to_closed(mg, monkeypatch):
    """bmask, 64 x 32 x 8, land on i = 1..8 and 57..64, the rest water.  Water rows have no coupling to land, so the level-1 operator on the
    water columns is the same with periodic = 0 and periodic = 1; the coarse masks are all water, so the iterates differ.  Solved to
    tol = 1e-11 three times: closed four colours, closed red-black, periodic four colours.  The yardstick is formed here, from code the
    option does not touch: d0 = max|p_FC - p_RB| on the water columns of the two closed solves in units of max|p| (the CPU oracle gives
    4.6e-13 for four colours against red-black on a similar closed case), and the periodic solve lies within 16 x d0 of the closed one.
    Measured on the MI355X: 46, 45 and 46 iterations; d0 = 5.9e-11, the periodic solve 6.0e-12 away from the closed one."""
    nx, ny, nz, tol = 64, 32, 8, 1e-11
    g = geometry(nx, ny, 0)
    g["rmask"] = np.ones((nx, ny)); g["rmask"][:8] = 0.0; g["rmask"][56:] = 0.0
    water = g["rmask"] != 0.0
    u, v, w = velocities_from(velocity_bases(nx, ny, nz, 1, 23), 1)   # u(nx+1) = u(1): both on land
    sol = {}
    for key, per, method in (("closed-FC", 0, "FC"), ("closed-RB", 0, "RB"), ("periodic-FC", 1, "FC")):
        _init(mg, (nx, ny, nz), per, monkeypatch, relax_method=method, bmask=1)
        f = full2d(g, 1)   # the same arrays for all three: the i halo is land either way
        mg.nhydro_matrices(f["dx"], f["dy"], f["zeta"], f["h"], f["rmask"], HC, 0.0, 0.0)
        mg.nhydro.compute_rhs(u, v, w)
        n, hist = mg.solve_p(tol, 300)
        print(key, "iterations", n, "residual", hist[-1])
        assert n < 300 and hist[-1] <= tol, (key, n, hist[-1])
        sol[key] = mg.grid(1).p[1:-1, 1:-1]
    pmax = np.abs(sol["closed-FC"][water]).max()
    d0 = np.abs(sol["closed-FC"] - sol["closed-RB"])[water].max() / pmax
    d = np.abs(sol["periodic-FC"] - sol["closed-FC"])[water].max() / pmax
    print("d0", d0, "periodic against closed", d)
    assert d0 > 0
    assert d <= 16 * d0, (d, d0)


# ---- 6. red-black, the default order -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 8), (64, 32, 64)], ids=["32x32x8", "64x32x64"])
def test_red_black_sequential_order_at_speed(mg, dims, monkeypatch):
    """periodic = 3, every level: one relax call of three sweeps from a rough random state with "rb_seq" (the default: the walk starts at
    plane 1 and reads the wrapped image of plane nx as it was before the pass) against "rb_exact" (the plane loop), within 1e-12 of max|p|,
    the bound of test_relax_rb_sequential_order_at_speed"""
    mg.nhydro_clean(); mg.nhydro.set_option("rb_seq", 1); mg.nhydro.set_option("rb_exact", 0)
    _init(mg, dims, 3, monkeypatch, relax_method="RB")
    matrices(mg, geometry(*dims[:2], 3), 3)
    rng = np.random.default_rng(31)
    start = {lev: (rng.standard_normal(mg.grid(lev)._shape("p")), rng.standard_normal(mg.grid(lev)._shape("b"))) for lev in range(1, mg.nlevs() + 1)}

    def run():
        out = {}
        for lev, (p, b) in start.items():
            g = mg.grid(lev)
            g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
            mg.relax(lev, 3)
            out[lev] = g.get("p")
        return out

    try:
        seq = run()
        mg.nhydro.set_option("rb_exact", 1)
        exact = run()
    finally:
        mg.nhydro.set_option("rb_exact", 0)
    for lev in start:
        d = np.abs(seq[lev] - exact[lev]).max() / np.abs(exact[lev]).max()
        print(dims, "level", lev, d)
        assert not np.array_equal(exact[lev], start[lev][0])
        assert d <= 1e-12, (lev, d)


# ---- 7. the resident time step -------------------------------------------------------------------------------------------------------
def test_resident_step(mg, monkeypatch):
    """periodic = 1, 32 x 32 x 16.  After nhydro_update_zeta_device with a new zeta every level's cA, zr, zw equal bit for bit what a fresh
    nhydro_matrices with that zeta leaves (the call's contract); nhydro_solve_device gives the p, u, v, w of nhydro_solve bit for bit;
    "zeta_chain_launches" stays 0 (the hierarchy is not closed)."""
    import torch
    dims, per = (32, 32, 16), 1
    nx, ny, nz = dims
    g = geometry(nx, ny, per, stretched=True)
    f = full2d(g, per)
    zeta2 = _pad(0.3 * np.random.default_rng(100).standard_normal((nx, ny)), per, 0, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    par = dict(solver_prec=1e-30, solver_maxiter=3)

    def fields():
        return {(lev, name): mg.grid(lev).get(name) for lev in range(1, mg.nlevs() + 1) for name in ("cA", "zr", "zw", "zeta")}

    _init(mg, dims, per, monkeypatch, **par)
    mg.nhydro_matrices_device(*(dev(f[n]) for n in ("dx", "dy", "zeta", "h")), None, g["hc"], g["theta_b"], g["theta_s"])
    mg.nhydro_update_zeta_device(dev(zeta2))
    assert mg.nhydro.get_option("zeta_refreshes") == 1 and mg.nhydro.get_option("zeta_chain_launches") == 0
    refreshed = fields()
    u, v, w = velocities_from(velocity_bases(nx, ny, nz, per, 29), per)
    du, dv, dw = dev(u), dev(v), dev(w)
    mg.nhydro.nhydro_solve_device(du, dv, dw)
    p_dev = mg.grid(1).p
    _init(mg, dims, per, monkeypatch, **par)
    mg.nhydro_matrices(f["dx"], f["dy"], zeta2, f["h"], None, g["hc"], g["theta_b"], g["theta_s"])
    rebuilt = fields()
    for key in refreshed:
        assert np.array_equal(refreshed[key], rebuilt[key]), key
    assert not np.array_equal(rebuilt[1, "zeta"][1:-1, 1:-1], f["zeta"][1:-1, 1:-1])
    mg.nhydro_solve(u, v, w)
    assert np.array_equal(p_dev, mg.grid(1).p) and np.abs(p_dev).max() > 0
    for a, b in ((du, u), (dv, v), (dw, w)):
        assert np.array_equal(a.cpu().numpy(), b)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(mg, monkeypatch):
    """each in words that name the option, and the solver is usable afterwards"""
    from mgroms_amd._lib import MgxError
    dims = (32, 16, 8)
    g = geometry(32, 16, 1)

    def solves():
        u, v, w = velocities_from(velocity_bases(*dims, 1, 3), 1)
        mg.nhydro.compute_rhs(u, v, w)
        n, hist = mg.solve_p(1e-8, 50)
        assert hist[-1] <= 1e-8, hist

    mg.nhydro_clean(); mg.nhydro.set_option("periodic", 1)
    with pytest.raises(MgxError, match=r'"periodic" = 1 needs a single rank \(process grid 2 x 1\)'):
        mg.nhydro_init(16, 16, 8, 2, 1, 0, mg.nhydro.default_params(relax_method="FC"))
    _init(mg, dims, 1, monkeypatch)
    matrices(mg, g, 1)
    solves()
    try:
        mg.nhydro.set_option("cycle_precision", 32)
        with pytest.raises(MgxError, match=r'"periodic" = 1 is not served by the fp32 cycles \(cycle_precision = 32'):
            mg.solve_p(1e-8, 50)
        mg.nhydro.set_option("cycle_precision", 64)
        solves()
        mg.nhydro.set_option("krylov", 2); mg.nhydro.set_option("krylov_precision", 32)
        with pytest.raises(MgxError, match=r'"periodic" = 1 is not served by the fp32 cycles .*krylov_precision = 32'):
            mg.solve_p(1e-8, 50)
        mg.nhydro.set_option("krylov_precision", 64)
        solves()   # Krylov with fp64 cycles is served
        mg.nhydro.set_option("krylov", 0)
        for value in (0, 2, 3):
            with pytest.raises(MgxError, match=r"periodic = %d: the hierarchy in use was built with periodic = 1 and the option takes effect at mgx_init" % value):
                mg.nhydro.set_option("periodic", value)
        mg.nhydro.set_option("periodic", 1)   # the value in use is taken
        assert mg.nhydro.get_option("periodic") == 1
        solves()
    finally:
        for name, value in (("cycle_precision", 64), ("krylov", 0), ("krylov_precision", 64)):
            mg.nhydro.set_option(name, value)


def test_gauss_seidel_is_served(mg, monkeypatch):
    """relax_method = 'GS' on a periodic level is the hyperplane sweep of a level with neighbours, the wrapped images those of the sweep
    before (include/mgx.h): it converges, and to the solution four colours find"""
    dims, per, tol = (32, 16, 8), 3, 1e-10
    g = geometry(32, 16, per)
    u, v, w = velocities_from(velocity_bases(*dims, per, 5), per)
    sol = {}
    for method in ("FC", "GS"):
        _init(mg, dims, per, monkeypatch, relax_method=method)
        matrices(mg, g, per)
        mg.nhydro.compute_rhs(u, v, w)
        n, hist = mg.solve_p(tol, 100)
        true = _true_residual(mg)
        print(method, n, hist[-1], true)
        assert hist[-1] <= tol and true <= tol * (1 + 1e-6), (method, n, hist[-1], true)
        sol[method] = mg.grid(1).p[1:-1, 1:-1]
    assert np.abs(sol["GS"] - sol["FC"]).max() <= 1e-7 * np.abs(sol["FC"]).max()


# ---- 9. nothing moves with the option off ---------------------------------------------------------------------------------------------
PARENT_COUNTERS = {"launches": 374, "halo_fills": 231, "exchanges": 0, "allreduces": 0, "p2p_exchanges": 0}


def test_counters_with_the_option_off(mg, monkeypatch):
    """periodic = 0, 64 x 32 x 64, four colours: mgx_counters after nhydro_matrices, compute_rhs and three solve_p iterations equal the
    counts of the parent commit ea2d9bf for this case (recorded from that commit's library with this sequence)."""
    dims = (64, 32, 64)
    _init(mg, dims, 0, monkeypatch, solver_prec=1e-30, solver_maxiter=3)
    matrices(mg, geometry(64, 32, 0), 0)
    u, v, w = velocities_from(velocity_bases(*dims, 0, 11), 0)
    mg.nhydro.compute_rhs(u, v, w)
    n, hist = mg.solve_p(1e-30, 3)
    c = mg.nhydro.counters()
    print("counters", c)
    assert n == 3
    assert c == PARENT_COUNTERS, c
