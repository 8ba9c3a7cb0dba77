"""The tall-column colour pass on STORED coefficients (nz = 80, 96, 128 with bmask, a user matrix or MGX_NO_MF: k_relax_tall_st,
mgx_relax_tall.hip), which before ran the generic column plus a physical-halo launch per colour.

Against the CPU oracle: four colours and rb_exact bit for bit (interior, k = 1, k = nz and every physical mirror -- the whole array
with its halo); the default red-black order within 1e-12 of max|p| per relax call of rb_exact (the project's bound for that mode,
test_gpu_vertical_sizes.py); solve_p histories to 1e-12 relative (norms are reduced in another order).  The two-wave blocks and
the streaming variant need nx * ny >= 524 288, too large for the oracle in seconds: there the pass is compared word for word with
the generic column of a child process under MGX_NO_TALL=1 (tests/_gpu_tall_stored_worker.py).

Shapes: 16 x 32 is a half-row of 16 columns (one partial wave), 8 x 256 a half-row of 128 (two j-chunks), 4 x 30 an odd half-row
of 15.  (The odd half-row was asked for at 16 x 30 x 128, which mgx_init refuses, as the reference's assumptions do: its second level
would be 8 x 15 x 64.  ny = 30 is only possible where level 1 is the only level, i.e. nx = 4: the same half-row, two planes per colour,
and Vcycle(1) is then the coarsest-level solve by ns_coarsest sweeps of the same pass.)
nz = 80 is only relaxed and V-cycled, never solved: its 5 -> 2 restriction diverges in the reference too.

The oracle runs are collected without a GPU too (the tests without the gpu mark): the masked oracle is finite and its
three-iteration solves at nz = 96 and 128 contract."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import on_gpu, oracle_twin, problem, rhs, uvw

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# (nx, ny, nz, cmatrix, coefficients): "bmask" = island mask on both sides, "user" = the oracle's own matrix perturbed per slot
FC_CASES = [(16, 32, 80, "real", "bmask"), (16, 32, 96, "real", "bmask"), (16, 32, 128, "real", "bmask"), (8, 256, 96, "real", "bmask"),
            (4, 30, 128, "real", "bmask"), (16, 32, 128, "simple", "bmask"), (16, 32, 128, "real", "user")]
SOLVE_CASES = [(32, 32, 96), (32, 32, 128)]
BIG = (1024, 512, 80)   # gx0 * nplanes = 4 * 512 = 2048: two waves per block; 3.0 GB of coefficients: the streaming variant


def _ids(cases):
    return ["x".join(str(d) for d in c[:3]) + "".join("-" + s for s in c[3:]) for c in cases]


@functools.lru_cache(maxsize=None)
def _case(nx, ny, nz, method="FC", cmatrix="real", bmask=True):
    """the record of a seamount case: what _gpu_setup() hands to the GPU and _oracle() to the oracle"""
    return problem((nx, ny, nz), bmask=bmask, relax_method=method, cmatrix=cmatrix, solver_prec=1e-10)


def _oracle(*case, **kw):
    return oracle_twin(_case(*case, **kw))


def _user_matrix(cA):
    """the oracle's own level-1 matrix, each slot scaled by a factor of its own (fixed seed): the couplings shrink by up to 10 %, the
    diagonal grows by up to 10 %, so the columns stay diagonally dominant"""
    f = np.random.default_rng(96128).uniform(0.0, 0.1, 8)
    out = cA.copy()
    out[..., 0] *= 1.0 + f[0]
    for s in range(1, 8):
        out[..., s] *= 1.0 - f[s]
    return out


def _random_pb(shape, seed):
    r = np.random.default_rng(seed)
    return r.standard_normal(shape), r.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def _fc_reference(case):
    """the oracle's p after relax(1, 1), after relax(1, ns_pre) and after one Vcycle(1), from a random level-1 state; computed once
    per case and read only"""
    nx, ny, nz, cmatrix, coef = case
    o = _oracle(nx, ny, nz, "FC", cmatrix, bmask=coef == "bmask")
    cA = None
    if coef == "user":
        cA = _user_matrix(o.field("cA"))
        o.field("cA")[...] = cA
    p0, b0 = _random_pb(o.field("p").shape, nz + nx)
    o.field("p")[...] = p0; o.field("b")[...] = b0; o.fill_halo(1, "p")
    out = []
    o.relax(1, 1); out.append(o.field("p").copy())
    o.relax(1, o.par.ns_pre); out.append(o.field("p").copy())
    o.vcycle(1); out.append(o.field("p").copy())
    for a in out:
        a.setflags(write=False)
    return dict(p0=p0, b0=b0, cA=cA, steps=out, ns_pre=int(o.par.ns_pre))


@functools.lru_cache(maxsize=None)
def _solve_reference(dims):
    nx, ny, nz = dims
    o = _oracle(nx, ny, nz, "FC", "real", bmask=True)
    rhs(None, o, uvw(dims))
    n, hist, _ = o.solve_p(1e-30, 3)
    p = o.field("p").copy(); p.setflags(write=False)
    return dict(n=n, hist=hist, p=p)


# ---- without a GPU: the references themselves ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC_CASES, ids=_ids(FC_CASES))
def test_oracle_masked_tall_columns_finite(case):
    ref = _fc_reference(case)
    for a in ref["steps"]:
        assert np.isfinite(a).all() and np.abs(a).max() > 0


@pytest.mark.parametrize("dims", SOLVE_CASES, ids=_ids(SOLVE_CASES))
def test_oracle_masked_tall_solve_contracts(dims):
    ref = _solve_reference(dims)
    h = ref["hist"]
    assert ref["n"] == 3 and np.isfinite(h).all() and np.isfinite(ref["p"]).all()
    assert all(h[k + 1] < h[k] for k in range(3)), h


# ---- on the GPU --------------------------------------------------------------------------------------------------------------
mg = gpu_module(rb_exact=0)


def _gpu_setup(mg, *case, **kw):
    on_gpu(mg, _case(*case, **kw))


def _passes(mg):
    return mg.nhydro.get_option("tall_stored_passes")


def _set_pb(mg, p, b):
    g = mg.grid(1)
    g.set("p", p); g.set("b", b); mg.fill_halo(1, "p")
    return g


def _same(a, c, what):
    """bit for bit, and where not: which part of p differs (interior, bottom row, top row, physical mirrors)"""
    if np.array_equal(a, c):
        return
    d = np.abs(a - c)
    inner = d[1:-1, 1:-1]
    halo = d.copy(); halo[1:-1, 1:-1] = 0
    raise AssertionError(f"{what}: interior {inner.max():.3e} (k=1 {inner[..., 0].max():.3e}, k=nz {inner[..., -1].max():.3e}), "
                         f"mirrors {halo.max():.3e}, {np.count_nonzero(d)} cells differ")


@gpu
def test_stored_tall_pass_is_taken(mg):
    """masked domain and user matrix: four colour passes by the stored tall kernel, four launches per relax call (the generic column
    needs a physical-halo launch per colour: eight); the unmasked define_matrices matrix keeps the matrix-free tall kernel"""
    nx, ny, nz = 16, 32, 96

    def call():
        n0, c0 = _passes(mg), mg.nhydro.counters()["launches"]
        mg.relax(1, 1)
        return _passes(mg) - n0, mg.nhydro.counters()["launches"] - c0

    _gpu_setup(mg, nx, ny, nz, bmask=True)
    _set_pb(mg, *_random_pb(mg.grid(1)._shape("p"), 1))
    assert call() == (4, 4)
    _gpu_setup(mg, nx, ny, nz, bmask=False)
    g = _set_pb(mg, *_random_pb(mg.grid(1)._shape("p"), 1))
    assert call() == (0, 4) and _passes(mg) == 0
    g.set("cA", g.get("cA"))
    assert call() == (4, 4)


@gpu
@pytest.mark.parametrize("case", FC_CASES, ids=_ids(FC_CASES))
def test_fc_bitwise(mg, case):
    """p with its halo after relax(1, 1), relax(1, ns_pre) and one Vcycle(1), bit for bit"""
    nx, ny, nz, cmatrix, coef = case
    ref = _fc_reference(case)
    _gpu_setup(mg, nx, ny, nz, "FC", cmatrix, bmask=coef == "bmask")
    g = mg.grid(1)
    if coef == "user":
        g.set("cA", ref["cA"])
    _set_pb(mg, ref["p0"], ref["b0"])
    n0 = _passes(mg)
    mg.relax(1, 1); _same(g.get("p"), ref["steps"][0], "relax(1, 1)")
    mg.relax(1, ref["ns_pre"]); _same(g.get("p"), ref["steps"][1], "relax(1, ns_pre)")
    assert _passes(mg) - n0 == 4 * (1 + ref["ns_pre"])
    mg.Vcycle(1); _same(g.get("p"), ref["steps"][2], "Vcycle(1)")


@gpu
def test_rb_exact_bitwise(mg):
    """the reference's sequential red-black order (one launch per plane) at 16 x 32 x 128 with bmask, bit for bit"""
    nx, ny, nz = 16, 32, 128
    o = _oracle(nx, ny, nz, "RB", "real", bmask=True)
    p0, b0 = _random_pb(o.field("p").shape, 43)
    o.field("p")[...] = p0; o.field("b")[...] = b0; o.fill_halo(1, "p")
    mg.nhydro.set_option("rb_exact", 1)
    try:
        _gpu_setup(mg, nx, ny, nz, "RB", "real", bmask=True)
        g = _set_pb(mg, p0, b0)
        n0 = _passes(mg)
        for call in (1, 2):
            mg.relax(1, 1); o.relax(1, 1)
            _same(g.get("p"), o.field("p"), f"relax call {call}")
        assert _passes(mg) - n0 == 4
    finally:
        mg.nhydro.set_option("rb_exact", 0)


@gpu
@pytest.mark.parametrize("dims", [(32, 32, 128), (32, 32, 96)], ids=_ids([(32, 32, 128), (32, 32, 96)]))
def test_rb_default_order_close_to_exact(mg, dims):
    """the default red-black order (rb_seq, windowed walk, row cut on) on level 1 with bmask: each relax call within 1e-12 of max|p|
    of rb_exact from the same state, mirrors included -- the rows above the cut take their physical images from the colour pass"""
    nx, ny, nz = dims
    p0, b0 = _random_pb((nx + 2, ny + 2, nz), 41)
    mg.nhydro.set_option("rb_exact", 1)
    try:
        _gpu_setup(mg, nx, ny, nz, "RB", "real", bmask=True)
        g = _set_pb(mg, p0, b0)
        exact = []
        for _ in range(2):
            mg.relax(1, 1); exact.append(g.get("p"))
    finally:
        mg.nhydro.set_option("rb_exact", 0)
    _gpu_setup(mg, nx, ny, nz, "RB", "real", bmask=True)
    assert mg.nhydro.get_option("rb_seq") == 1 and mg.nhydro.get_option("rb_exact") == 0 and mg.nhydro.get_option("rbseq_rowcut") == 1
    start = p0
    for call, pe in enumerate(exact):
        g = _set_pb(mg, start, b0)
        n0 = _passes(mg)
        mg.relax(1, 1)
        assert _passes(mg) - n0 == 2
        a = g.get("p")
        err = np.abs(a - pe).max() / np.abs(pe).max()
        print(f"rb default vs rb_exact {dims} call {call}: {err:.3e}")
        assert err <= 1e-12, (call, err)
        start = pe


@gpu
@pytest.mark.parametrize("dims", SOLVE_CASES, ids=_ids(SOLVE_CASES))
def test_fc_solve_bitwise(mg, dims):
    """three solve_p iterations with bmask: p bit for bit, the history to 1e-12, and the stored tall kernel did the level-1 passes"""
    nx, ny, nz = dims
    ref = _solve_reference(dims)
    _gpu_setup(mg, nx, ny, nz, "FC", "real", bmask=True)
    w = -np.ones((nz + 1, ny + 2, nx + 2)); w[0] = 0
    mg.nhydro.compute_rhs(np.zeros((nz, ny + 2, nx + 1)), np.zeros((nz, ny + 1, nx + 2)), w)
    n0 = _passes(mg)
    n, hist = mg.solve_p(1e-30, 3)
    assert n == ref["n"] == 3
    assert np.all(np.abs(hist - ref["hist"]) <= 1e-13 + 1e-12 * np.abs(ref["hist"])), (hist, ref["hist"])
    _same(mg.grid(1).get("p"), ref["p"], "solve_p")
    assert _passes(mg) - n0 > 0


@gpu
def test_two_wave_blocks_and_streaming_same_words_as_generic_column(mg):
    """1024 x 512 x 80 with bmask, four colours: blocks of two waves and the non-temporal variant.  p after relax(1, 1) word for word
    the generic column's (a child process under MGX_NO_TALL=1, run first: if it fails nothing more is started here)"""
    nx, ny, nz = BIG
    out = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "_gpu_tall_stored_worker.py")] + [str(d) for d in BIG],
                         env=dict(os.environ, MGX_NO_TALL="1"), capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    rec = dict(l.split()[:2] for l in out.stdout.splitlines() if l.startswith(("DIGEST", "PASSES", "LAUNCHES")))
    assert rec["PASSES"] == "0" and rec["LAUNCHES"] == "8", rec   # the child ran the generic column
    from _gpu_tall_stored_worker import big_state
    _gpu_setup(mg, nx, ny, nz, "FC", "real", bmask=True)
    g = _set_pb(mg, *big_state(nx, ny, nz))
    n0, c0 = _passes(mg), mg.nhydro.counters()["launches"]
    mg.relax(1, 1)
    assert (_passes(mg) - n0, mg.nhydro.counters()["launches"] - c0) == (4, 4)
    p = g.get("p")
    mg.nhydro_clean()
    assert np.isfinite(p).all()
    assert hashlib.sha256(p.tobytes()).hexdigest() == rec["DIGEST"]
