"""The model coupling of nhydro_solve -- compute_rhs and correct_uvw on the model's own u, v, w (mgx_model.hip, mgx_define.cpp) --
against the CPU oracle, bit for bit, at the shapes and run layouts a model uses.

The model kernels run one lane per (i,j) column and climb a run of rows in k, carrying row k+1 to the next step in registers; each
run starts by reloading what the run below would have carried.  How many rows a run has depends on the plane's wave count
(`_runs`, restated from igrid_run in mgx_model.hip): 8 on small grids, 12..64 on production grids.  So the velocities here are random
in every index (halos and the bottom w included) on geometries with slopes, and the shapes are chosen so that between them they cover
every run layout and lane / row tail the kernels have (test_shape_list_covers_every_run_layout).  Everything is compared with
np.array_equal: the model kernels keep the reference's operation order and are compiled without FMA contraction.

correct_uvw is pinned on its own with a pressure given to both sides: p is set, its halo filled, then nhydro_solve runs with
warm_start and solver_maxiter = 0, i.e. compute_rhs, no iteration, correct_uvw -- and p must come out unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _gpu import gpu_module
from _problem import gpu_problem, load, load_uvw, oracle_twin, problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
mg = gpu_module()


# ---- run layouts (igrid_run / igrid_k of mgx_model.hip) -------------------------------------------------------------------------
def _runs(ni, nj, klast, kr_env=0):
    """row counts of the runs igrid_run launches for ni x nj lanes over rows 1..klast (kr_env: MGX_MODEL_KR)"""
    waves = -(-ni // 64) * nj
    nrun = -(-klast // kr_env) if kr_env > 0 else -(-16384 // waves)
    nrun = max(nrun, 1)
    if kr_env <= 0:
        nrun = min(nrun, -(-klast // 8))  # at least eight rows per run (the heuristic's floor)
    kr = -(-klast // nrun)
    nb = -(-klast // kr)
    return [kr] * (nb - 1) + [klast - kr * (nb - 1)]


def _layout(nx, ny, nz, kr_env=0):
    return {"uf": _runs(nx + 1, ny, nz, kr_env), "vf": _runs(nx, ny + 1, nz, kr_env), "wf": _runs(nx, ny, nz + 1, kr_env),
            "correct_uvw": _runs(nx + 2, ny + 2, nz, kr_env), "accum_kr": 8 if nz >= 16 else nz}


# (nx, ny, nz), geometry, velocities
SHAPES = [
    ((512, 512, 64), "seamount", "random"),  # the bench: runs of 16 (wf 17, last 14); i tails of 1 and 2 lanes
    ((512, 512, 48), "rndtopo", "random"),   # runs of 12 (wf 13, last 10), nz not a power of two
    ((256, 512, 96), "seamount", "random"),  # uf runs of 14 with a last of 12, vf 12, wf 13 with a last of 6
    ((64, 64, 16), "rndtopo", "random"),     # two runs of 8; j tail of 1 row (v: ny+1 = 65)
    ((62, 6, 24), "seamount", "random"),     # j tails of 2 and 3 rows, nx+1 = 63 lanes (one level: 62x30 would coarsen to odd sizes)
    ((16, 32, 128), "rndtopo", "random"),    # sixteen runs of 8, wf's last run a single row
    ((8, 16, 2), "seamount", "random"),      # nz = 2: one run everywhere, igrid_k takes KR = klast
    ((128, 64, 40), "seamount", "smooth"),   # a flow-like field (u ~ 0.1 m/s, w ~ 1e-3 m/s) plus noise
]


def test_shape_list_covers_every_run_layout():
    """The shapes above must keep covering, under the current run heuristic: one run; several equal runs; runs longer than 8 of at
    least three lengths; a ragged last run of wf; nz = 2; nz not a power of two; i-block tails of 1 and 2 lanes; j tails of 1, 2, 3 rows."""
    lay = {s: _layout(*s) for s, _, _ in SHAPES}
    for s, l in lay.items():
        print(s, l)
    every = [r for l in lay.values() for key in ("uf", "vf", "wf", "correct_uvw") for r in [l[key]]]
    assert any(len(r) == 1 for r in every), "one run"
    assert any(len(r) > 1 and len(set(r)) == 1 for r in every), "several equal runs"
    assert len({x for r in every for x in r if x > 8}) >= 3 and {12, 16} <= {x for r in every for x in r}, "runs longer than 8"
    assert any(l["wf"][-1] < l["wf"][0] for l in lay.values()), "ragged last run of wf"
    assert any(s[2] == 2 and l["accum_kr"] == 2 for s, l in lay.items()), "nz = 2"
    assert {24, 48, 96} <= {s[2] for s in lay}, "nz not a power of two"
    itails = {n % 64 for (nx, ny, nz) in lay for n in (nx, nx + 1, nx + 2)}
    assert {1, 2} <= itails, "i-block tails of 1 and 2 lanes"
    jtails = {n % 4 for (nx, ny, nz) in lay for n in (ny, ny + 1, ny + 2)}
    assert {1, 2, 3} <= jtails, "j tails of 1, 2 and 3 rows"


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _setup(mg, nx, ny, nz, geom="seamount", bmask=False, **par):
    """one GPU instance and a one-rank oracle with the same geometry and namelist (FC; bmask: the island mask on both)"""
    return oracle_twin(gpu_problem(mg, (nx, ny, nz), geom=geom, bmask=bmask,
                                   **dict(dict(relax_method="FC", solver_prec=1e-10, solver_maxiter=0), **par)))


def _velocities(nx, ny, nz, seed, kind="random"):
    """u (nz, ny+2, nx+1), v (nz, ny+1, nx+2), w (nz+1, ny+2, nx+2): every entry different, halos and the bottom w included"""
    rng = np.random.default_rng(seed)
    shapes = ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2))
    if kind == "random":
        return tuple(rng.standard_normal(s) for s in shapes)
    # a smooth flow scaled like a real one: u, v ~ 0.1 m/s varying in i, j and k; w ~ 1e-3 m/s; plus 1 % noise
    out = []
    for s, amp in zip(shapes, (0.1, 0.1, 1e-3)):
        k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in s), indexing="ij")
        f = amp * np.sin(2 * np.pi * i / s[2] + 0.3) * np.cos(2 * np.pi * j / s[1]) * (1.0 + 0.5 * k / s[0])
        out.append(f + 0.01 * amp * rng.standard_normal(s))
    return tuple(out)


def _assert_uvw(u, v, w, o, what=""):
    for name, a in (("u", u), ("v", v), ("w", w)):
        b = o.field(name)
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:5].tolist(), np.abs(a - b).max())


def _same_pressure(mg, o, seed):
    """the same random p on both sides, halo filled on both sides; returns the GPU's p (must equal the oracle's, halo included)"""
    g1 = mg.grid(1)
    p = np.random.default_rng(seed).standard_normal(g1._shape("p"))
    g1.set("p", p)
    mg.fill_halo(1, "p")
    o.field("p")[...] = p
    o.fill_halo(1, "p")
    p1 = g1.p
    assert np.array_equal(p1, o.field("p"))
    return p1


def _correct_only(mg, u, v, w, rmask=None, device=False):
    """nhydro_solve with no iteration (solver_maxiter = 0, warm start): compute_rhs, then correct_uvw with the p that is there"""
    assert mg.nhydro.get_option("solver_maxiter") == 0
    mg.nhydro.set_option("warm_start", 1)
    try:
        if device:
            mg.nhydro.nhydro_solve_device(u, v, w, rmask)
        else:
            mg.nhydro_solve(u, v, w, rmask)
    finally:
        mg.nhydro.set_option("warm_start", 0)


# ---- 1 + 2: compute_rhs and correct_uvw across run layouts and lane tails -----------------------------------------------------
@pytest.mark.parametrize("dims,geom,kind", SHAPES, ids=["%dx%dx%d" % s for s, _, _ in SHAPES])
def test_compute_rhs_and_correct_uvw_run_layouts(mg, dims, geom, kind):
    nx, ny, nz = dims
    print(dims, _layout(nx, ny, nz))
    o = _setup(mg, nx, ny, nz, geom)
    u, v, w = _velocities(nx, ny, nz, seed=nz + nx, kind=kind)
    load_uvw(o, (u, v, w))
    mg.nhydro.compute_rhs(u, v, w)
    o.compute_rhs()
    b = mg.grid(1).b
    assert np.array_equal(b, o.field("b")), np.argwhere(b != o.field("b"))[:5].tolist()
    # correct_uvw on its own, from the same p
    p = _same_pressure(mg, o, seed=ny)
    _correct_only(mg, u, v, w)
    assert np.array_equal(mg.grid(1).p, p)  # no iteration ran
    assert np.array_equal(mg.grid(1).b, b)
    o.correct_uvw()
    _assert_uvw(u, v, w, o, dims)


# ---- 3: end to end at the bench size -----------------------------------------------------------------------------------------
def test_nhydro_solve_end_to_end_bench_size(mg):
    """FC nhydro_solve with one iteration at 512x512x64 (compute_rhs, F-cycle, correct_uvw): p, u, v, w bit for bit; then
    nhydro_check_nondivergence on the corrected fields against the oracle's; then the device path on torch tensors, same bits."""
    import torch
    nx, ny, nz = 512, 512, 64
    o = _setup(mg, nx, ny, nz, "seamount", solver_maxiter=1)
    u, v, w = _velocities(nx, ny, nz, seed=3)
    du, dv, dw = (torch.from_numpy(a).cuda() for a in (u, v, w))
    load_uvw(o, (u, v, w))
    mg.nhydro_solve(u, v, w)
    p = mg.grid(1).p
    n, hist, _ = o.nhydro_solve()
    assert n == 1
    assert np.array_equal(p, o.field("p"))
    _assert_uvw(u, v, w, o, "host")
    mg.nhydro_check_nondivergence(u, v, w)
    o.check_nondivergence()
    assert np.array_equal(mg.grid(1).b, o.field("b"))
    mg.nhydro.nhydro_solve_device(du, dv, dw)
    assert np.array_equal(mg.grid(1).p, p)
    for d, a in ((du, u), (dv, v), (dw, w)):
        assert np.array_equal(d.cpu().numpy(), a)


# ---- 4: masks at a shape with runs of 12 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bmask", "call_mask"])
def test_masks_multi_run_shape(mg, case):
    """512x512x48 (runs of 12).  "bmask": bmask = .true. with the island mask, passed to the call as the reference's drivers do.
    "call_mask": bmask = .true. and a per-call mask with land the matrices have not seen (the oracle reads it with use_call_mask).
    b, u, v, w bit for bit; the same call once more with u, v, w and the mask as device tensors (nhydro_solve_device): same bits."""
    import torch
    from mgroms_amd.testcases import island_mask
    nx, ny, nz = 512, 512, 48
    m0 = island_mask(nx, ny)
    o = _setup(mg, nx, ny, nz, "rndtopo", bmask=True)
    mcall = m0
    if case == "call_mask":
        mcall = m0.copy()
        mcall[40:90, ny - 150:ny - 70] = 0.0  # not symmetric under i <-> j
        o.field("rmaska")[...] = mcall
        o.use_call_mask(True)
    u, v, w = _velocities(nx, ny, nz, seed=17)
    dev = [torch.from_numpy(a).cuda() for a in (u, v, w)]
    load_uvw(o, (u, v, w))
    mg.nhydro.compute_rhs(u, v, w, mcall)
    o.compute_rhs()
    b = mg.grid(1).b
    assert np.array_equal(b, o.field("b"))
    p = _same_pressure(mg, o, seed=5)
    _correct_only(mg, u, v, w, mcall)
    assert np.array_equal(mg.grid(1).p, p) and np.array_equal(mg.grid(1).b, b)
    o.correct_uvw()
    _assert_uvw(u, v, w, o, case)
    _correct_only(mg, *dev, rmask=torch.from_numpy(np.ascontiguousarray(mcall)).cuda(), device=True)
    assert np.array_equal(mg.grid(1).b, b), "device path: b"
    assert np.array_equal(mg.grid(1).p, p)
    for d, a in zip(dev, (u, v, w)):
        assert np.array_equal(d.cpu().numpy(), a), "device path: u, v, w"


# ---- 5: forced run lengths ---------------------------------------------------------------------------------------------------
def test_forced_run_lengths_against_the_oracle(mg, tmp_path):
    """MGX_MODEL_KR is read once per process: each run length is a child process (tests/_gpu_model_kr_worker.py, one at a time) that
    writes b and the corrected u, v, w; each is compared with the oracle.  128x64x40: 3, 7 and 13 divide neither nz nor nz + 1, and
    KR = 1 makes every row a run start."""
    nx, ny, nz = 128, 64, 40
    o = oracle_twin(problem((nx, ny, nz), geom="rndtopo", relax_method="FC", solver_prec=1e-10, solver_maxiter=0))   # (the worker's call)
    u0, v0, w0 = _velocities(nx, ny, nz, seed=23)
    layouts = set()
    for kr in (None, 1, 3, 7, 13, 1000):
        env = {k: v for k, v in os.environ.items() if k != "MGX_MODEL_KR"}
        if kr is not None:
            env["MGX_MODEL_KR"] = str(kr)
        lay = _layout(nx, ny, nz, kr or 0)
        layouts.add(str(lay))
        print("MGX_MODEL_KR", kr, lay)
        out_dir = tmp_path / ("kr%s" % kr)
        out_dir.mkdir()
        r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_model_kr_worker.py"), str(nx), str(ny), str(nz), str(out_dir)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (kr, r.stdout[-2000:], r.stderr[-2000:])
        got = {n: np.load(out_dir / (n + ".npy")) for n in ("b", "p", "u", "v", "w", "u0")}
        assert np.array_equal(got["u0"], u0)  # the worker drew the same velocities
        load_uvw(o, (u0, v0, w0))
        o.compute_rhs()
        assert np.array_equal(got["b"], o.field("b")), ("b", kr)
        o.field("p")[...] = got["p"]
        o.fill_halo(1, "p")
        assert np.array_equal(got["p"], o.field("p")), ("p", kr)
        o.correct_uvw()
        for name in ("u", "v", "w"):
            assert np.array_equal(got[name], o.field(name)), (name, kr)
    assert len(layouts) == 6  # every KR gave a layout of its own


# ---- 6: two time steps with a moving free surface --------------------------------------------------------------------------
def test_two_time_steps_with_a_moving_free_surface(mg):
    """One nhydro_init, then twice: nhydro_matrices with a new zeta and h, nhydro_solve (FC, two iterations) on the velocities the
    previous step corrected.  theta_s = theta_b = 0: setup_zr_zw has no transcendental function, so the coefficients are bitwise
    even with zeta /= 0, and so are b, p, u, v, w after each step -- which needs the model-space copies of zw, dzw, cw, zxdy, zydx
    rebuilt by every nhydro_matrices."""
    nx, ny, nz = 96, 64, 24
    pr = problem((nx, ny, nz), relax_method="FC", solver_prec=1e-12, solver_maxiter=2)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, mg.nhydro.default_params(**pr.par))
    o = oracle_twin(pr)
    dx, dy, _, h0 = pr.fields
    rng = np.random.default_rng(31)
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    u, v, w = _velocities(nx, ny, nz, seed=37)
    load_uvw(o, (u, v, w))
    for step, ph in enumerate((0.0, 1.3)):
        zeta = 0.8 * np.sin(2 * np.pi * i / nx + ph) * np.cos(2 * np.pi * j / ny - ph) + 0.05 * rng.standard_normal((nx + 2, ny + 2))
        h = h0 + 20.0 * rng.standard_normal((nx + 2, ny + 2))
        pr.fields = (dx, dy, zeta, h)
        mg.nhydro_matrices(*pr.fields, None, *pr.sigma)
        load(o, pr)
        for name in ("zw", "cw", "cA"):
            assert np.array_equal(mg.grid(1).get(name), o.field(name)), (step, name)
        mg.nhydro_solve(u, v, w)
        n, hist, _ = o.nhydro_solve()
        assert n == 2
        assert np.array_equal(mg.grid(1).b, o.field("b")), step
        assert np.array_equal(mg.grid(1).p, o.field("p")), step
        _assert_uvw(u, v, w, o, "step %d" % step)
