"""tests/_problem.py without a GPU: a stand-in for the package records what gpu_problem() hands over, and a real Oracle shows what
oracle_twin() made of the same record.  Pinned: both sides get the same arrays, parameters and sigma; options that mgx_init reads are set
between the clean and the init; the seeded state is drawn in the order u, v, w; and the two texts of the geometry generators
(oracle.mgoracle for the oracle's own drivers, mgroms_amd.testcases for everything fed to the GPU) agree on every rank."""
import functools
import inspect

import numpy as np
import pytest

import _problem
from mgroms_amd import testcases
from oracle import mgoracle

ORACLE_PARAMETERS = set(inspect.signature(mgoracle.Oracle.__init__).parameters) - {"self", "nx", "ny", "nz", "npx", "npy"}


class Recorder:
    """stands for `mgroms_amd` and for `mgroms_amd.nhydro`: every call the builder makes, in order, with its arguments"""

    def __init__(self):
        self.calls = []
        self.nhydro = self
        for name in ("default_params", "nhydro_clean", "set_option", "nhydro_init", "nhydro_matrices", "compute_rhs"):
            setattr(self, name, self._note(name))

    def _note(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return ("params", kw) if name == "default_params" else None
        return call

    def named(self, name):
        return [(args, kw) for n, args, kw in self.calls if n == name]

    def order(self):
        return [n for n, _, _ in self.calls]


@pytest.fixture
def oracle_calls(monkeypatch):
    """the keyword arguments of every Oracle(...), and the arguments of every matrices(...) with the fields it found on every rank (it fills
    their halos), noted on the instance"""
    init, matrices = mgoracle.Oracle.__init__, mgoracle.Oracle.matrices

    @functools.wraps(init)     # (the builder reads the parameter names from the signature)
    def noting_init(self, *args, **kw):
        self.init_kw = kw
        init(self, *args, **kw)

    def noting_matrices(self, *sigma):
        self.sigma = sigma
        self.found = {name: [self.field(name, 1, r).copy() for r in range(self.nranks)] for name in ("dx", "dy", "zeta", "h", "rmask")}
        matrices(self, *sigma)

    monkeypatch.setattr(mgoracle.Oracle, "__init__", noting_init)
    monkeypatch.setattr(mgoracle.Oracle, "matrices", noting_matrices)


def _given(mg):
    """what the GPU call received: the namelist members, the init arguments, (dx, dy, zeta, h), rmask and sigma"""
    (_, par), = mg.named("default_params")
    (init, _), = mg.named("nhydro_init")
    (mat, _), = mg.named("nhydro_matrices")
    assert init[-1] == ("params", par)       # the Params that went to nhydro_init are the ones default_params made
    return par, init[:-1], mat[:4], mat[4], mat[5:]


CASES = [dict(), dict(geom="rndtopo"), dict(bmask=True), dict(geom="rndtopo", bmask=True),
         dict(zeta="rough", sigma=(250.0, 0.4, 6.0)), dict(bmask=True, rmask="basin", zeta="rough", sigma=(250.0, 0.4, 6.0))]
PAR = dict(relax_method="FC", solver_prec=1e-10, solver_maxiter=7, ns_pre=1, ns_post=4, cmatrix="simple", interp_type="nearest")


def _case(dims, case):
    nx, ny, _ = dims
    case = dict(case)
    if case.get("zeta") == "rough":
        case["zeta"] = 0.3 * np.random.default_rng(1).standard_normal((nx + 2, ny + 2))
    if case.get("rmask") == "basin":
        m = np.ones((nx + 2, ny + 2)); m[0, :] = m[-1, :] = 0.0; m[:, 0] = m[:, -1] = 0.0; m[3, 2] = 0.0
        case["rmask"] = m
    return case


@pytest.mark.parametrize("only", [None, ("relax_method", "cmatrix", "bmask")], ids=["all", "only"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()) or "plain")
@pytest.mark.parametrize("dims", [(16, 16, 8), (8, 16, 2)], ids=lambda d: "%dx%dx%d" % d)
def test_gpu_and_oracle_are_given_the_same_problem(oracle_calls, dims, case, only):
    mg = Recorder()
    kw = _case(dims, case)
    pr = _problem.gpu_problem(mg, dims, **kw, **PAR)
    o = _problem.oracle_twin(pr, only=only)
    assert mg.order() == ["default_params", "nhydro_init", "nhydro_matrices"]
    par, init, fields, rmask, sigma = _given(mg)
    assert init == dims + (1, 1, 0)
    assert par == dict(PAR, **({"bmask": 1} if kw.get("bmask") else {}))
    # the record is what the GPU was given
    assert pr.dims == dims and pr.par == par and pr.sigma == sigma and pr.rmask is rmask and all(a is c for a, c in zip(pr.fields, fields))
    # the oracle holds the same arrays ...
    for name, a in zip(("dx", "dy", "zeta", "h"), fields):
        assert a.shape == (dims[0] + 2, dims[1] + 2) and np.array_equal(o.found[name][0], a), name
    if "zeta" in kw:
        assert fields[2] is kw["zeta"]
    assert (rmask is not None) == bool(kw.get("bmask"))
    if rmask is not None:
        assert np.array_equal(o.found["rmask"][0], rmask)
        assert np.array_equal(rmask, kw["rmask"] if "rmask" in kw else testcases.island_mask(dims[0], dims[1]))
    # ... the same parameters, or none for those that only= leaves out ...
    want = {k: v for k, v in par.items() if k in ORACLE_PARAMETERS and (only is None or k in only)}
    assert o.init_kw == want and (only is not None or set(want) == set(par))
    assert o.par.bmask == (1 if kw.get("bmask") else 0) and o.par.relax_method == mgoracle.METHOD["FC"] and o.par.cmatrix_real == 0
    assert (o.par.ns_pre, o.par.ns_post, o.par.interp_linear) == ((1, 4, 0) if only is None else (3, 2, 1))
    # ... and the same sigma
    assert o.sigma == sigma == tuple(kw.get("sigma", (4e3, 0.0, 0.0)))


@pytest.mark.parametrize("geom,bmask", [("seamount", False), ("rndtopo", False), ("seamount", True), ("rndtopo", True)])
def test_emulated_ranks_hold_the_blocks_of_the_same_problem(oracle_calls, geom, bmask):
    """2 x 2 emulated ranks of 8 x 8 x 8: every rank's fields are its block (with halo) of what the one GPU rank was given"""
    _emulated_ranks_hold_the_blocks(geom, bmask, "uniform")


@pytest.mark.parametrize("geom,bmask", [("seamount", False), ("rndtopo", False), ("seamount", True), ("rndtopo", True)])
def test_emulated_ranks_hold_the_blocks_of_the_curvilinear_problem(oracle_calls, geom, bmask):
    """the same with metric="curvilinear": every rank holds its block of the one global dx(i,j), dy(i,j), the halo columns it shares
    with its neighbours included"""
    _emulated_ranks_hold_the_blocks(geom, bmask, "curvilinear")


def _emulated_ranks_hold_the_blocks(geom, bmask, metric):
    mg = Recorder()
    pr = _problem.gpu_problem(mg, (16, 16, 8), geom=geom, bmask=bmask, metric=metric, **PAR)
    assert pr.metric == metric
    o = _problem.oracle_twin(pr, 2, 2)
    par, _, fields, rmask, sigma = _given(mg)
    assert (np.ptp(fields[0]) > 0 and np.ptp(fields[1]) > 0) == (metric == "curvilinear")
    assert (o.nx, o.ny, o.nz, o.npx, o.npy) == (8, 8, 8, 2, 2) and o.sigma == sigma
    assert o.init_kw == {k: v for k, v in par.items() if k in ORACLE_PARAMETERS}
    for r in range(4):
        pi, pj = r % 2, r // 2
        block = (slice(8 * pi, 8 * pi + 10), slice(8 * pj, 8 * pj + 10))
        for name, a in zip(("dx", "dy", "zeta", "h"), fields):
            assert np.array_equal(o.found[name][r], a[block]), (r, name)
        if bmask:
            assert np.array_equal(o.found["rmask"][r], rmask[block]), r
    # a record that holds fields of the caller's own has no per-rank blocks: refused, not guessed
    pr.fields = (pr.fields[0], pr.fields[1], pr.fields[2] + 1.0, pr.fields[3])
    with pytest.raises(AssertionError):
        _problem.oracle_twin(pr, 2, 2)
    # nor has a record whose fields are another metric's than the one it names
    other = "uniform" if metric == "curvilinear" else "curvilinear"
    wrong = _problem.problem((16, 16, 8), geom=geom, bmask=bmask, metric=metric, **PAR)
    wrong.metric = other
    with pytest.raises(AssertionError):
        _problem.oracle_twin(wrong, 2, 2)


@pytest.mark.parametrize("dims", [(16, 16, 8), (8, 16, 2)], ids=lambda d: "%dx%dx%d" % d)
@pytest.mark.parametrize("geom", ["seamount", "rndtopo"])
def test_the_curvilinear_problem_is_the_generators_times_the_metric(oracle_calls, dims, geom):
    """metric="curvilinear" multiplies the generator's dx, dy by testcases.curvilinear_metric and leaves zeta, h alone; both sides get it"""
    nx, ny, _ = dims
    mg = Recorder()
    pr = _problem.gpu_problem(mg, dims, geom=geom, metric="curvilinear", **PAR)
    o = _problem.oracle_twin(pr)
    plain = _problem.problem(dims, geom=geom, **PAR)
    assert plain.metric == "uniform" and pr.metric == "curvilinear"
    fx, fy = testcases.curvilinear_metric(nx, ny)
    _, _, fields, _, _ = _given(mg)
    assert np.array_equal(fields[0], plain.fields[0] * fx) and np.array_equal(fields[1], plain.fields[1] * fy)
    assert np.array_equal(fields[2], plain.fields[2]) and np.array_equal(fields[3], plain.fields[3])
    for name, a in zip(("dx", "dy", "zeta", "h"), fields):
        assert np.array_equal(o.found[name][0], a), name
    with pytest.raises(AssertionError):
        _problem.problem(dims, geom=geom, metric="stretched", **PAR)


def test_curvilinear_metric_varies_in_both_directions_on_every_rank():
    """fx, fy are defined on global indices: within [0.75, 1.25]; each varies along both axes, is neither symmetric nor separable, and
    neither is the other or a one-cell shift of it; a rank of a process grid holds its block of the one-rank arrays, the halo columns
    it shares with its neighbours included"""
    for nxg, nyg in ((32, 32), (32, 16), (48, 96)):
        fx, fy = testcases.curvilinear_metric(nxg, nyg)
        for f in (fx, fy):
            assert f.shape == (nxg + 2, nyg + 2) and f.dtype == np.float64
            assert 0.75 <= f.min() and f.max() <= 1.25
            assert np.all(np.ptp(f, axis=0) > 1e-3) and np.all(np.ptp(f, axis=1) > 1e-3)      # every row and every column varies
            assert np.linalg.matrix_rank(f - f.mean(), tol=1e-6) >= 2                       # not a(i) + b(j), so not a(i) * b(j) either
            assert np.abs(np.diff(f, axis=0)).min() > 0 and np.abs(np.diff(f, axis=1)).min() > 0   # no two neighbours are equal
        if nxg == nyg:
            assert np.abs(fx - fx.T).max() > 1e-2 and np.abs(fy - fy.T).max() > 1e-2
            assert np.abs(fx - fy.T).max() > 1e-2
        assert np.abs(fx - fy).max() > 1e-2
        for a, c in ((fx[1:], fy[:-1]), (fx[:-1], fy[1:]), (fx[:, 1:], fy[:, :-1]), (fx[:, :-1], fy[:, 1:])):
            assert np.abs(a - c).max() > 1e-2
    fx, fy = testcases.curvilinear_metric(32, 32)
    assert not np.array_equal(fx, fx.T)
    for npx, npy in ((2, 2), (2, 1), (1, 2), (4, 2)):
        nx, ny = 32 // npx, 32 // npy
        for rank in range(npx * npy):
            pi, pj = rank % npx, rank // npx
            block = (slice(nx * pi, nx * pi + nx + 2), slice(ny * pj, ny * pj + ny + 2))
            bx, by = testcases.curvilinear_metric(nx, ny, npx, npy, rank)
            assert np.array_equal(bx, fx[block]) and np.array_equal(by, fy[block]), (npx, npy, rank)
            dx = _problem._geometry("seamount", nx, ny, npx, npy, rank, "curvilinear")[0]
            assert np.array_equal(dx, _problem._geometry("seamount", 32, 32, metric="curvilinear")[0][block])


def test_init_options_are_set_between_clean_and_init():
    mg = Recorder()
    _problem.gpu_problem(mg, (16, 16, 8), init_options=dict(hold_odd_nz=1, periodic=3), relax_method="FC")
    assert mg.order() == ["nhydro_clean", "set_option", "set_option", "default_params", "nhydro_init", "nhydro_matrices"]
    assert [args for args, _ in mg.named("set_option")] == [("hold_odd_nz", 1), ("periodic", 3)]
    mg = Recorder()
    _problem.gpu_problem(mg, (16, 16, 8), relax_method="FC")
    assert "nhydro_clean" not in mg.order() and "set_option" not in mg.order()


def test_model_state_and_right_hand_side(oracle_calls):
    dims = nx, ny, nz = 8, 16, 2
    r = np.random.default_rng(5)
    want = (r.uniform(-1, 1, (nz, ny + 2, nx + 1)), r.uniform(-1, 1, (nz, ny + 1, nx + 2)), r.uniform(-1, 1, (nz + 1, ny + 2, nx + 2)))
    got = _problem.uvw(dims, seed=5)
    assert all(np.array_equal(a, c) for a, c in zip(got, want))      # one generator, drawn in the order u, v, w
    rest = _problem.uvw(dims)
    assert all(np.array_equal(a, c) for a, c in zip(rest, testcases.resting_column_state(nx, ny, nz)))
    mg = Recorder()
    o = _problem.oracle_twin(_problem.gpu_problem(mg, dims, relax_method="FC"))
    _problem.rhs(mg, o, got)
    (args, kw), = mg.named("compute_rhs")
    assert len(args) == 3 and not kw and all(a is c for a, c in zip(args, got))
    for name, a in zip("uvw", got):
        assert np.array_equal(o.field(name), a), name
    # on emulated ranks every rank holds its block of the same state, the shared faces and halo rows included
    o4 = _problem.oracle_twin(_problem.problem((16, 16, 8), relax_method="FC"), 2, 2)
    state = _problem.uvw((16, 16, 8), seed=6)
    _problem.load_uvw(o4, state)
    for rank in range(4):
        pi, pj = rank % 2, rank // 2
        assert np.array_equal(o4.field("u", 1, rank), state[0][:, 8 * pj:8 * pj + 10, 8 * pi:8 * pi + 9])
        assert np.array_equal(o4.field("v", 1, rank), state[1][:, 8 * pj:8 * pj + 9, 8 * pi:8 * pi + 10])
        assert np.array_equal(o4.field("w", 1, rank), state[2][:, 8 * pj:8 * pj + 10, 8 * pi:8 * pi + 10])


def test_hist_close_has_no_defaults():
    h = np.array([1.0, 1e-3, 1e-6])
    assert _problem.hist_close(h, h * (1 + 5e-13), rtol=1e-12, atol=0.0, same_length=True)
    assert not _problem.hist_close(h, h * (1 + 5e-12), rtol=1e-12, atol=0.0, same_length=True)
    assert _problem.hist_close(h, h + 5e-14, rtol=0.0, atol=1e-13, same_length=True)
    assert not _problem.hist_close(h, h[:2], rtol=1.0, atol=1.0, same_length=True)
    with pytest.raises(TypeError):
        _problem.hist_close(h, h)


@pytest.mark.parametrize("npx,npy", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("name", ["seamount_geometry", "rndtopo_geometry"])
def test_the_two_texts_of_the_generators_agree(name, npx, npy):
    """oracle/mgoracle.py must import without the package, so it keeps its own text of the generators: equal on every rank"""
    for nx, ny in ((16, 16), (8, 16)):
        for rank in range(npx * npy):
            a, c = getattr(mgoracle, name)(nx, ny, npx, npy, rank), getattr(testcases, name)(nx, ny, npx, npy, rank)
            assert len(a) == len(c) == 4
            for x, y in zip(a, c):
                assert x.shape == y.shape == (nx + 2, ny + 2) and np.array_equal(x, y), (rank, nx, ny)
