"""Where a test problem is made: the set-up the GPU is given, and the CPU oracle's twin of exactly that set-up.

gpu_problem() initialises the library and returns a record of what it handed over; oracle_twin() builds an Oracle from that record and from
nothing else, so the two sides of a bit-for-bit comparison cannot be given different problems.  Geometry and mask come from
mgroms_amd.testcases only (tests/test_problem_host.py holds the oracle's own text of the generators to it, and this module to its contract)."""
import inspect
from types import SimpleNamespace

import numpy as np

SIGMA = (4e3, 0.0, 0.0)


def _geometry(geom, nx, ny, npx=1, npy=1, rank=0, metric="uniform"):
    """dx, dy, zeta, h of one rank; metric="curvilinear": dx, dy times that rank's block of testcases.curvilinear_metric"""
    from mgroms_amd import testcases
    dx, dy, zeta, h = {"seamount": testcases.seamount_geometry, "rndtopo": testcases.rndtopo_geometry}[geom](nx, ny, npx, npy, rank)
    assert metric in ("uniform", "curvilinear"), metric
    if metric == "curvilinear":
        fx, fy = testcases.curvilinear_metric(nx, ny, npx, npy, rank)
        dx, dy = dx * fx, dy * fy
    return dx, dy, zeta, h


def problem(dims, geom="seamount", bmask=False, rmask=None, zeta=None, sigma=SIGMA, metric="uniform", **par):
    """The record of a one-rank problem: dims, the namelist members, (dx, dy, zeta, h), the mask and the sigma triple.  bmask: the masked
    system, with `rmask` or the island mask; zeta: instead of the generator's; metric: "uniform", the generator's constant dx, dy, or
    "curvilinear", those times testcases.curvilinear_metric (dx(i,j), dy(i,j))."""
    from mgroms_amd.testcases import island_mask
    nx, ny, nz = dims
    if bmask:
        par["bmask"] = 1
        rmask = island_mask(nx, ny) if rmask is None else rmask
    else:
        assert rmask is None
    dx, dy, z0, h = _geometry(geom, nx, ny, metric=metric)
    if zeta is not None:
        z0 = zeta
    return SimpleNamespace(dims=(nx, ny, nz), geom=geom, metric=metric, par=par, fields=(dx, dy, z0, h), rmask=rmask, sigma=tuple(sigma))


def on_gpu(mg, pr, init_options=None):
    """nhydro_init + nhydro_matrices of the record.  init_options: options that mgx_init reads (hold_odd_nz, periodic) -- clean, set, init in
    that order."""
    if init_options:
        mg.nhydro_clean()
        for name, value in init_options.items():
            mg.nhydro.set_option(name, value)
    mg.nhydro_init(*pr.dims, 1, 1, 0, mg.nhydro.default_params(**pr.par))
    mg.nhydro_matrices(*pr.fields, pr.rmask, *pr.sigma)
    return pr


def gpu_problem(mg, dims, init_options=None, **kw):
    """problem(dims, ...) handed to the GPU; returns the record, i.e. exactly what the GPU was given"""
    return on_gpu(mg, problem(dims, **kw), init_options)


def oracle_twin(problem, npx=1, npy=1, only=None):
    """The Oracle of `problem`: every parameter of the record that Oracle.__init__ accepts (only=: just these names -- for a file whose oracle
    deliberately keeps its defaults for the rest), the record's fields, mask and sigma.  npx x npy: the same global problem on emulated ranks,
    each with its block of the generators' geometry under the metric the record names."""
    from oracle.mgoracle import Oracle
    nx, ny, nz = problem.dims
    accepted = set(inspect.signature(Oracle.__init__).parameters) - {"self", "nx", "ny", "nz", "npx", "npy"}
    par = {k: v for k, v in problem.par.items() if k in accepted and (only is None or k in only)}
    o = Oracle(nx // npx, ny // npy, nz, npx, npy, **par)
    load(o, problem)
    return o


def load(o, problem):
    """the record's fields, mask and sigma into the oracle, and its matrices (again after a test changed the record's fields)"""
    from mgroms_amd.testcases import island_mask
    nx, ny, _ = problem.dims
    one = o.nranks == 1
    if not one:    # every rank makes its own block: the record must hold the generators' fields, not the caller's own
        assert all(np.array_equal(a, c) for a, c in zip(problem.fields, _geometry(problem.geom, nx, ny, metric=problem.metric)))
        assert problem.rmask is None or np.array_equal(problem.rmask, island_mask(nx, ny))
    for r in range(o.nranks):
        dx, dy, zeta, h = problem.fields if one else _geometry(problem.geom, o.nx, o.ny, o.npx, o.npy, r, problem.metric)
        for name, a in (("dx", dx), ("dy", dy), ("zeta", zeta), ("h", h)):
            o.field(name, 1, r)[...] = a
        if problem.rmask is not None:
            o.field("rmask", 1, r)[...] = problem.rmask if one else island_mask(o.nx, o.ny, o.npx, o.npy, r)
    o.matrices(*problem.sigma)


def uvw(dims, seed=None):
    """the model state: the resting column of the reference's driver, or with a seed uniform in (-1, 1), drawn in the order u, v, w"""
    nx, ny, nz = dims
    if seed is None:
        from mgroms_amd.testcases import resting_column_state
        return resting_column_state(nx, ny, nz)
    r = np.random.default_rng(seed)
    u = r.uniform(-1, 1, (nz, ny + 2, nx + 1)); v = r.uniform(-1, 1, (nz, ny + 1, nx + 2)); w = r.uniform(-1, 1, (nz + 1, ny + 2, nx + 2))
    return u, v, w


def load_uvw(o, state):
    """u, v, w of the whole domain into the oracle's rank blocks (numpy layout [k][j][i]; neighbours share their halo rows and the face between them)"""
    lx, ly = o.nx, o.ny
    for r in range(o.nranks):
        pi, pj = r % o.npx, r // o.npx
        for name, a, ex, ey in zip("uvw", state, (1, 2, 2), (2, 1, 2)):
            o.field(name, 1, r)[...] = a[:, pj * ly:pj * ly + ly + ey, pi * lx:pi * lx + lx + ex]


def rhs(mg, o, state):
    """compute_rhs of u, v, w on the GPU and on the oracle (either may be None)"""
    if o is not None:
        load_uvw(o, state)
        o.compute_rhs()
    if mg is not None:
        mg.nhydro.compute_rhs(*state)


def random_level(mg, o, lev, rng):
    """p, then b, drawn for level `lev`, set on the GPU and on the oracle (o=None: the GPU only), p's halo filled on both; returns the GPU's grid"""
    g = mg.grid(lev)
    p = rng.standard_normal(g._shape("p")); b = rng.standard_normal(g._shape("b"))
    g.set("p", p); g.set("b", b); mg.fill_halo(lev, "p")
    if o is not None:
        o.field("p", lev)[...] = p; o.field("b", lev)[...] = b; o.fill_halo(lev, "p")
    return g


def hist_close(h, ho, rtol, atol, same_length):
    """every entry of a residual history within atol + rtol * |ho| of the other's; same_length: and as many entries"""
    if same_length and len(h) != len(ho):
        return False
    return bool(np.all(np.abs(h - ho) <= atol + rtol * np.abs(ho)))


def oracle_relative_residual(o, p):
    """the oracle's fp64 ||b - A p|| / ||b|| of p"""
    bn = np.sqrt(np.sum(o.field("b")[1:-1, 1:-1, :] ** 2))
    o.field("p")[...] = p
    o.fill_halo(1, "p")
    return o.residual(1) / bn


def regions(a):
    """rows k = 2..nz-1, k = 1 and k = nz of the interior columns, and the halo cells"""
    inner = a[1:-1, 1:-1]
    out = {"k=1": inner[:, :, 0], "k=nz": inner[:, :, -1],
           "halo": np.concatenate([a[0].ravel(), a[-1].ravel(), a[1:-1, 0].ravel(), a[1:-1, -1].ravel()])}
    if a.shape[2] > 2:
        out["interior"] = inner[:, :, 1:-1]
    return out
