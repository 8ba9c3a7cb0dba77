"""Every A/B switch of mgx_switches.cpp (and MGX_NO_SMALL) takes "its measured alternative": here each alternative runs, on the smallest
shapes that reach it, against the CPU oracle and against the default arm.  The cases, their probes and the evidence that the
alternative ran are the table of tests/_switch_cases.py; tests/test_switch_coverage_host.py keeps that table complete.

The switches are read once per process: an arm is a child process (tests/_gpu_switch_worker.py) started through _ranks.run_commands
with every variable of the table scrubbed from its environment, the arms one after another (the default arm of a probe list beside the
first variant that needs it: two processes at the most), the project's deadline of 120 s, nothing retried.  The default arm of a probe
list runs once per module.  An arm whose case shows its alternative by kernel names runs under
`rocprofv3 --kernel-trace --output-format csv`, and that one run is also its result (so does the default arm of such a list).

Tolerances: those of the header of tests/test_gpu_parity.py, no others.
  four colours, red-black with cmatrix = 'simple', red-black with option rb_exact: every field equals the oracle's and the default
      arm's bit for bit; a residual history is within 1e-12 relative of the oracle's (another order of the reduction) and equals the default arm's
  red-black with cmatrix = 'real' in the sequential order at speed (rb_seq): p within 1e-12 of max|p| of the oracle per relax call,
      within 1e-10 after V-cycles and after a solve; histories |d| <= 1e-13 + 1e-10 ref (b of the coarse levels of a cycle, a
      restricted residual, has no bound there and is held by the default arm's bits alone); and the default arm's bits, unless the case
      declares levels of the probe in not_same_bits with its reason (the switch trades the walk for the plane loop), and then exactly
      those levels differ"""
import csv
import glob
import os
import re
import shutil
import sys

import numpy as np
import pytest

from _ranks import run_commands
from _switch_cases import CASES, INIT_VARIABLES, LEVELS, PROBE_SETS, probe_id, probe_mode, table_variables

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_default = {}    # probe list -> (arrays, kernel names or None)
_variant = {}    # case -> (arrays, kernel names or None)
_failed = []     # the case whose arms did not end with status 0


def _traced(name):
    """does the default arm of this probe list need a kernel trace?"""
    return any(c["probes"] == name and c["evidence"]["kind"] == "kernel" for c in CASES.values())


def _command(case, env_add, trace, tmp, tag):
    env = {k: v for k, v in os.environ.items() if k not in set(table_variables()) | set(INIT_VARIABLES)}
    env.update(env_add)
    argv = [sys.executable, os.path.join(HERE, "_gpu_switch_worker.py"), case, str(tmp / f"{tag}.npz")]
    if trace:
        prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
        argv = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp / f"{tag}_trace"), "--"] + argv
    return argv, env


def _collect(tmp, tag, trace):
    arrays = dict(np.load(tmp / f"{tag}.npz"))
    if not trace:
        return arrays, None
    names = set()
    files = glob.glob(str(tmp / f"{tag}_trace" / "**" / "*kernel_trace.csv"), recursive=True)
    assert files, f"rocprofv3 left no kernel trace under {tmp / (tag + '_trace')}"
    for f in files:
        for row in csv.DictReader(open(f)):
            names.add(row["Kernel_Name"].replace(" ", ""))
    assert names, files
    return arrays, names


def _arms(case, tmp_path_factory):
    """(default arm, variant arm) of a case, each (arrays, kernel names): run once, shared by the tests below and left unchanged"""
    c = CASES[case]
    if case not in _variant:
        tmp = tmp_path_factory.mktemp(case)
        todo = []
        if c["probes"] not in _default:
            todo.append(("default", {}, _traced(c["probes"])))
        todo.append(("variant", c["env"], c["evidence"]["kind"] == "kernel"))
        # a child that exits with a non-zero status, or the deadline, raises in run_commands with the child's tail: the arms of the
        # cases that follow are then not started (whatever ended a process on the card is looked into first)
        # (the case stays in _failed until its results are stored: a result that cannot be read does not start the children again either)
        assert not _failed, f"not started: an arm of {_failed[0]} failed earlier in this module"
        _failed.append(case)
        run_commands([_command(case, env, trace, tmp, tag) for tag, env, trace in todo], timeout=120)
        got = {tag: _collect(tmp, tag, trace) for tag, env, trace in todo}
        if "default" in got:
            _default[c["probes"]] = got["default"]
        _variant[case] = got["variant"]
        _failed.pop()
    return _default[c["probes"]], _variant[case]


def _levels(arr, n):
    return sorted(int(k[len(f"{n}/dims"):]) for k in arr if k.startswith(f"{n}/dims"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_switch_arm_against_the_oracle(case, tmp_path_factory):
    """the variant arm against the CPU oracle on the same inputs, probe by probe; and the level shapes the case relies on"""
    (dflt, _), (var, _) = _arms(case, tmp_path_factory)
    bad = []
    for n, p in enumerate(PROBE_SETS[CASES[case]["probes"]]):
        pid, exact = probe_id(p), probe_mode(p) == "exact"
        for arr in (dflt, var):
            assert [tuple(arr[f"{n}/dims{lev}"]) for lev in _levels(arr, n)] == LEVELS[p["dims"]], pid
        for lev in _levels(var, n):
            if p["kind"] == "relax":
                err, eq = float(var[f"{n}/err{lev}"]), bool(var[f"{n}/eq{lev}"])
                print(f"{case} {pid} level {lev}: {int(var[f'{n}/launch{lev}'])} launches (default arm {int(dflt[f'{n}/launch{lev}'])}), {err:.3e} of max|p| from the oracle")
                if not (eq if exact else err <= 1e-12):
                    bad.append((pid, lev, err))
            else:
                for f in ("p", "b"):
                    err, eq = float(var[f"{n}/err_{f}{lev}"]), bool(var[f"{n}/eq_{f}{lev}"])
                    # (rb_seq: the header gives a bound for p and none for b of a coarse level, a restricted residual, whose size against
                    # the round-off of A p is not known beforehand: there b is held by its equality with the default arm alone)
                    if not exact:
                        print(f"{case} {pid} level {lev} {f}: {err:.3e} of its maximum from the oracle")
                    if not (eq if exact else (f == "b" or err <= 1e-10)):
                        bad.append((pid, f, lev, err))
        if p["kind"] == "cycle":
            h, oh = var[f"{n}/hist"], var[f"{n}/oracle_hist"]
            err, eq = float(var[f"{n}/err_p_solved"]), bool(var[f"{n}/eq_p_solved"])
            print(f"{case} {pid}: V-cycles of {var[f'{n}/vcycle'].tolist()} launches (default arm {dflt[f'{n}/vcycle'].tolist()}), history {h.tolist()}, oracle {oh.tolist()}, p {err:.3e}")
            assert h.shape == oh.shape == (3,) and np.all(np.isfinite(h)), (pid, h, oh)
            if not bool(var[f"{n}/eq_b_rhs"]):
                bad.append((pid, "b after compute_rhs"))
            if not (eq if exact else err <= 1e-10):
                bad.append((pid, "p after solve_p", err))
            if not np.all(np.abs(h - oh) <= (1e-12 * oh if exact else 1e-13 + 1e-10 * oh)):
                bad.append((pid, "history", h.tolist(), oh.tolist()))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", sorted(CASES))
def test_switch_arm_against_the_default_arm(case, tmp_path_factory):
    """every stored field and history of the variant arm equals the default arm's bit for bit -- except p of the levels the case lists
    in not_same_bits (rb_seq relax probes of a switch that trades the walk for the plane loop or the reverse), and each of those must
    indeed differ: an exemption that is not needed has to go"""
    c = CASES[case]
    (dflt, _), (var, _) = _arms(case, tmp_path_factory)
    assert sorted(dflt) == sorted(var)
    bad = []
    for n, p in enumerate(PROBE_SETS[c["probes"]]):
        pid = probe_id(p)
        keys = [k for k in sorted(var) if k.startswith(f"{n}/") and re.match(r"(p\d+|b\d+|b_rhs|hist|p_solved)$", k.split("/")[1])]
        assert keys, pid
        diff = [(k, float(np.abs(var[k] - dflt[k]).max())) for k in keys if not np.array_equal(var[k], dflt[k])]
        exempt = {f"{n}/p{lev}" for lev in c["not_same_bits"].get(pid, ((), ""))[0]}
        if exempt:
            print(f"{case} {pid}: not the same bits on levels {sorted(exempt)}; differs in {diff}")
        assert exempt <= set(keys), (pid, exempt)
        if {k for k, _ in diff} != exempt:
            bad.append((pid, "differs in", diff, "declared", sorted(exempt)))
    assert not bad, (case, bad)


def _count(arr, probes, pid, what):
    n = [probe_id(p) for p in probes].index(pid)
    if what == "vcycle":
        return int(arr[f"{n}/vcycle"][1])     # (the second of the two: nothing is built lazily any more)
    return int(arr[f"{n}/launch{what[3:]}"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_switch_alternative_ran(case, tmp_path_factory):
    """the evidence the case declares: launch counts derived from mgx_cycle.cpp, kernel names of the traced run, or the precondition
    under which a run-time argument or the grid differs"""
    c = CASES[case]
    ev, probes = c["evidence"], PROBE_SETS[c["probes"]]
    (dflt, dnames), (var, vnames) = _arms(case, tmp_path_factory)
    for pid, lev in c["one_launch"]:    # the persistent relax ran to its end in both arms (not its fallback after a time-out)
        assert _count(dflt, probes, pid, f"lev{lev}") == 1 and _count(var, probes, pid, f"lev{lev}") == 1, (case, pid, lev)
    if ev["kind"] == "launches":
        for pid, what, want_d, want_v, want_diff in ev["checks"]:
            d, v = _count(dflt, probes, pid, what), _count(var, probes, pid, what)
            print(f"{case} {pid} {what}: {d} launches by default, {v} in the variant arm")
            assert want_d is None or d == want_d, (case, pid, what, d, v)
            assert want_v is None or v == want_v, (case, pid, what, d, v)
            assert want_diff is None or v - d == want_diff, (case, pid, what, d, v)
    elif ev["kind"] == "kernel":
        assert dnames and vnames
        for pat in ev["present"]:
            hit = sorted(k for k in vnames if re.search(pat, k))
            print(f"{case} only in the variant arm, {pat}: {[k[:80] for k in hit]}")
            assert hit and not any(re.search(pat, k) for k in dnames), (case, pat, hit, sorted(k for k in dnames if re.search(pat, k)))
        for pat in ev["absent"]:
            hit = sorted(k for k in dnames if re.search(pat, k))
            print(f"{case} only in the default arm, {pat}: {[k[:80] for k in hit]}")
            assert hit and not any(re.search(pat, k) for k in vnames), (case, pat, hit, sorted(k for k in vnames if re.search(pat, k)))
    else:
        served = 0
        for pid, lev, differs in ev["checks"]:
            n = [probe_id(p) for p in probes].index(pid)
            nx, ny, nz = (int(a) for a in var[f"{n}/dims{lev}"])
            if ev.get("window"):    # the switch acts inside the windowed walk: count the levels it served (6 colours in 3 sweeps), in both arms
                wd, wv = int(dflt[f"{n}/win{lev}"]), int(var[f"{n}/win{lev}"])
                assert wd == wv, (case, pid, wd, wv)
                if wv != 6:
                    continue
            print(f"{case} {pid} level {lev} ({nx}x{ny}x{nz}): the precondition under which the arms differ holds: {differs(nx, ny, nz, probes[n]['method'])}")
            assert differs(nx, ny, nz, probes[n]["method"]), (case, pid, lev, (nx, ny, nz))
            served += 1
        assert served >= 1, case
