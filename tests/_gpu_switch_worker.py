"""Worker of tests/test_gpu_switches.py: the A/B switches are read from the environment once per process, so every arm of a case runs in a
process of its own.  Arguments: the case of tests/_switch_cases.py, the file the arrays go to (np.savez).  It runs the probes of the
case's list one after another, each on a fresh hierarchy with the CPU oracle beside it on the same inputs, and stores per probe (key
"<index>/<what>") the GPU fields, the launches of every call, and the error against the oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

import mgroms_amd as mg  # noqa: E402
from mgroms_amd import nhydro  # noqa: E402
from _problem import gpu_problem, oracle_twin  # noqa: E402
from _switch_cases import CASES, PROBE_SETS  # noqa: E402

case, dest = sys.argv[1], sys.argv[2]
probes = PROBE_SETS[CASES[case]["probes"]]
torch.cuda.set_device(0)
nhydro.set_verbose(0)
out = {}


def rel(a, c):
    """max|a - c| / max|c|"""
    return float(np.abs(a - c).max() / np.abs(c).max())


def launches():
    return nhydro.counters()["launches"]


def setup(p):
    o = oracle_twin(gpu_problem(mg, p["dims"], relax_method=p["method"], cmatrix=p["cmatrix"]))
    assert mg.nlevs() == o.nlevs
    return o


def relax_probe(n, p, o):
    rng = np.random.default_rng(100 + n)
    for lev in range(1, o.nlevs + 1):
        g = mg.grid(lev)
        out[f"{n}/dims{lev}"] = np.array([g.nx, g.ny, g.nz])
        pp = rng.standard_normal(g._shape("p")); bb = rng.standard_normal(g._shape("b"))
        g.set("p", pp); g.set("b", bb); mg.fill_halo(lev, "p")
        o.field("p", lev)[...] = pp; o.field("b", lev)[...] = bb; o.fill_halo(lev, "p")
        n0, w0 = launches(), nhydro.get_option("rbseq_window_colours")
        mg.relax(lev, 3)
        a = g.get("p")
        out[f"{n}/launch{lev}"] = np.array(launches() - n0)
        out[f"{n}/win{lev}"] = np.array(nhydro.get_option("rbseq_window_colours") - w0)
        o.relax(lev, 3)
        c = o.field("p", lev)
        out[f"{n}/p{lev}"] = a
        out[f"{n}/err{lev}"] = np.array(rel(a, c)); out[f"{n}/eq{lev}"] = np.array(np.array_equal(a, c))


def cycle_probe(n, p, o):
    nx, ny, nz = p["dims"]
    rng = np.random.default_rng(100 + n)
    u = 1e-2 * rng.standard_normal((nz, ny + 2, nx + 1)); v = 1e-2 * rng.standard_normal((nz, ny + 1, nx + 2))
    w = -np.ones((nz + 1, ny + 2, nx + 2)); w[0] = 0
    nhydro.compute_rhs(u, v, w)
    o.field("u")[...] = u; o.field("v")[...] = v; o.field("w")[...] = w
    o.compute_rhs()
    out[f"{n}/b_rhs"] = mg.grid(1).b
    out[f"{n}/eq_b_rhs"] = np.array(np.array_equal(out[f"{n}/b_rhs"], o.field("b", 1)))
    o.field("p", 1)[...] = mg.grid(1).p
    vl = []
    for _ in range(2):
        n0 = launches()
        mg.Vcycle(1)
        vl.append(launches() - n0)
        o.vcycle(1)
    out[f"{n}/vcycle"] = np.array(vl)
    for lev in range(1, o.nlevs + 1):
        g = mg.grid(lev)
        out[f"{n}/dims{lev}"] = np.array([g.nx, g.ny, g.nz])
        for f in ("p", "b"):
            a, c = g.get(f), o.field(f, lev)
            out[f"{n}/{f}{lev}"] = a
            out[f"{n}/err_{f}{lev}"] = np.array(rel(a, c)); out[f"{n}/eq_{f}{lev}"] = np.array(np.array_equal(a, c))
    _, hist = mg.solve_p(1e-30, 2)
    _, ohist, _ = o.solve_p(1e-30, 2)
    a, c = mg.grid(1).p, o.field("p", 1)
    out[f"{n}/hist"] = np.asarray(hist); out[f"{n}/oracle_hist"] = np.asarray(ohist)
    out[f"{n}/p_solved"] = a
    out[f"{n}/err_p_solved"] = np.array(rel(a, c)); out[f"{n}/eq_p_solved"] = np.array(np.array_equal(a, c))


for n, p in enumerate(probes):
    before = {k: nhydro.get_option(k) for k in p["options"]}
    try:
        o = setup(p)
        for k, val in p["options"].items():
            nhydro.set_option(k, val)
        (relax_probe if p["kind"] == "relax" else cycle_probe)(n, p, o)
        o.close()
    finally:
        for k, val in before.items():
            nhydro.set_option(k, val)
    mg.nhydro_clean()
np.savez(dest, **out)
print("DONE", len(probes), len(out))
