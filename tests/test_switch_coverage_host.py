"""The table of A/B switches (mgx_switches.cpp) and the suite stay together: every variable of the table, and the three that mgx_init
reads, is either set by a case of tests/_switch_cases.py (run by tests/test_gpu_switches.py against the oracle and the default arm)
or named in COVERED_ELSEWHERE with the test that pins it.  A switch added without a test fails here, on a machine without a GPU."""
import inspect
import os
import re

import _switch_cases as sc

ROOT = sc.ROOT


def _known():
    table = sc.table_variables()
    assert len(table) >= 20 and len(set(table)) == len(table), table
    return table + list(sc.INIT_VARIABLES)


def test_every_switch_has_a_case_or_a_named_test():
    in_cases = {v for c in sc.CASES.values() for v in c["env"]}
    missing = [v for v in _known() if v not in in_cases and v not in sc.COVERED_ELSEWHERE]
    assert not missing, missing
    assert set(sc.COVERED_ELSEWHERE) <= set(_known()), sorted(set(sc.COVERED_ELSEWHERE) - set(_known()))
    for var, where in sc.COVERED_ELSEWHERE.items():
        path, _, test = where.partition("::")
        assert path.startswith("tests/") and test.startswith("test_"), where
        text = open(os.path.join(ROOT, path)).read()
        m = re.search(rf"^def {re.escape(test)}\(", text, re.M)
        assert m, where
        assert var in text, (var, path)    # the file speaks of the variable (a worker may be the one that sets it from the test's arguments)


def test_cases_are_well_formed():
    known = set(_known())
    ids = {name: [sc.probe_id(p) for p in probes] for name, probes in sc.PROBE_SETS.items()}
    for name, probes in sc.PROBE_SETS.items():
        assert len(set(ids[name])) == len(ids[name]), name
        for p in probes:
            assert p["dims"] in sc.LEVELS and sc.LEVELS[p["dims"]][0] == p["dims"], p
    for name, c in sc.CASES.items():
        assert c["env"] and set(c["env"]) <= known, (name, sorted(set(c["env"]) - known))
        assert c["probes"] in sc.PROBE_SETS, name
        ev = c["evidence"]
        assert ev.get("kind") in sc.EVIDENCE_KINDS, (name, ev)   # exactly one kind of evidence, and something to assert with it
        if ev["kind"] == "kernel":
            assert ev["present"] and all(re.compile(p) for p in ev["present"] + ev["absent"]), name
        else:
            assert ev["checks"] and all(chk[0] in ids[c["probes"]] for chk in ev["checks"]), name
        if ev["kind"] == "launches":
            assert all(any(w is not None for w in chk[2:]) for chk in ev["checks"]), name
        if ev["kind"] == "shape":
            assert all(callable(chk[2]) and "mgx" in inspect.getsource(chk[2]) for chk in ev["checks"]), name   # the gating line is quoted
        assert all(pid in ids[c["probes"]] for pid, _ in c["one_launch"]), name


def test_only_the_sequential_order_at_speed_may_differ_from_the_default_arm():
    """not_same_bits is for red-black with cmatrix = 'real' in rb_seq mode alone: no four-colour probe, no 'simple' one, no rb_exact one
    and no transfer (cycle) probe may carry it; each entry has its one-line reason"""
    for name, c in sc.CASES.items():
        by_id = {sc.probe_id(p): p for p in sc.PROBE_SETS[c["probes"]]}
        for pid, (levels, reason) in c["not_same_bits"].items():
            p = by_id[pid]
            assert levels and all(1 <= lev <= len(sc.LEVELS[p["dims"]]) for lev in levels), (name, pid, levels)
            assert p["kind"] == "relax" and p["method"] == "RB" and p["cmatrix"] == "real" and not p["options"].get("rb_exact"), (name, pid)
            assert sc.probe_mode(p) == "rb_seq", (name, pid)
            assert isinstance(reason, str) and len(reason) > 20 and "\n" not in reason, (name, pid)


def test_design_table_names_the_test_of_every_row():
    """DESIGN.md repeats the table row for row, with a last column that names the test id that pins the row"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = dict(re.findall(r"^\| `(MGX_\w+)` \|.*\| ([^|]+) \|$", design, re.M))
    in_cases = {}
    for name, c in sc.CASES.items():
        for v in c["env"]:
            in_cases.setdefault(v, []).append(name)
    named = set(re.findall(r"`\[(\w+)\]`", design))
    assert named == set(sc.CASES), (sorted(named - set(sc.CASES)), sorted(set(sc.CASES) - named))   # every id there is a case, every case is there
    for var in sc.table_variables():
        assert var in rows, var
        if var in in_cases:
            assert "tests/test_gpu_switches.py" in rows[var] and all(f"[{n}]" in rows[var] for n in in_cases[var]), (var, rows[var])
        else:
            assert sc.COVERED_ELSEWHERE[var] in rows[var], (var, rows[var])
