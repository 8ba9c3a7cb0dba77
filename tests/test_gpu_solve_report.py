"""What solve_p reports, for each of its three drivers (fp64 cycles, "cycle_precision" = 32, "krylov" = 2): the printed lines, fort.100 and
the returned history say the same thing in the reference's formats (mg_solvers.f90:59,71-72,83-99).  The lines come from C's printf, so a child
process (tests/_gpu_solve_report_worker.py) runs the solves: the seamount at 16 x 16 x 8, four colours, tol = 1e-30 and maxite = 3, i.e. exactly
three iterations per driver, twice in one working directory.  Nothing here needs a tolerance: %24.16E carries a double exactly, and conv is
one IEEE division of two of them."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("plain", "mixed", "krylov")
ITE = re.compile(r"^ite = ([ \d]\d): res =  (0\.\d{3}E[+-]\d{2}) / conv = ([ \d]{6}\.\d{3})$")


@pytest.fixture(scope="module")
def report():
    """{(mode, k): (stdout lines of solve k, what the worker recorded after it)}"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gpu_solve_report_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out, key, lines = {}, None, []
    for ln in r.stdout.splitlines():
        if ln.startswith("@@ begin "):
            key, lines, rec = (ln.split()[2], int(ln.split()[3])), [], None
        elif ln.startswith("@@ json "):
            rec = json.loads(ln[len("@@ json "):])
        elif ln.startswith("@@ end "):
            out[key] = (lines, rec)
            key = None
        elif key is not None:
            lines.append(ln)
    assert sorted(out) == sorted((m, k) for m in MODES for k in (1, 2)), sorted(out)
    print("launches of the first solve:", {m: out[(m, 1)][1]["launches"] for m in MODES})
    return out


def e3(v):
    """Fortran's E10.3 of a positive number (0.dddE+ee) from its three-digit decimal rounding"""
    d, e = ("%.2E" % v).split("E")
    return "0.%sE%+03d" % (d.replace(".", ""), int(e) + 1)


@pytest.mark.parametrize("mode", MODES)
def test_printed_lines_fort100_and_hist_agree(report, mode):
    lines, rec = report[(mode, 1)]
    assert rec["n"] == 3
    hist = [float.fromhex(h) for h in rec["hist"]]
    assert len(hist) == 4
    # stdout: the header once, three numbered iteration lines, the summary block once
    assert lines.count(" - solve p:") == 1, lines
    ite = [ITE.match(ln) for ln in lines if ln.startswith("ite =")]
    assert len(ite) == 3 and all(ite), lines
    assert [int(m.group(1)) for m in ite] == [1, 2, 3]
    assert lines.count(" --- summary ---") == 1, lines
    q = lines.index(" --- summary ---")
    assert re.match(r"^time spent to solve :[ \d]{4}\.\d{3} s$", lines[q + 1]), lines[q + 1]
    assert re.match(r"^rescaled performance: 0\.\d{3}E[+-]\d{2}$", lines[q + 2]), lines[q + 2]
    assert lines[q + 3] == " ---------------"
    assert lines.index(" - solve p:") < lines.index(ite[0].group(0)) and lines.index(ite[2].group(0)) < q
    # fort.100: <res0> 0, then <res> <conv>, in " %24.16E" fields
    f100 = rec["fort100"].splitlines()
    assert len(f100) == 4, f100
    assert re.match(r"^ {3}\d\.\d{16}E[+-]\d{2} 0$", f100[0]), f100[0]
    for ln in f100[1:]:
        assert re.match(r"^ {3}\d\.\d{16}E[+-]\d{2} {3}\d\.\d{16}E[+-]\d{2}$", ln), ln
    col = [float(ln.split()[0]) for ln in f100]
    # the file's first column is the returned history (Krylov: its last hist entry is the true residual, the file holds the recurrence's value)
    last = 2 if mode == "krylov" else 3
    assert col[:last + 1] == hist[:last + 1], (col, hist)
    for n in (1, 2, 3):
        conv = float(f100[n].split()[1])
        assert conv == col[n - 1] / col[n], (n, conv, col)
        assert ite[n - 1].group(2) == e3(col[n]), (ite[n - 1].group(0), col[n])
        assert ite[n - 1].group(3) == "%10.3f" % conv, (ite[n - 1].group(0), conv)


@pytest.mark.parametrize("mode", MODES)
def test_second_solve_appends_to_fort100(report, mode):
    lines, rec = report[(mode, 2)]
    f100 = rec["fort100"].splitlines()
    assert len(f100) == 8, f100
    assert f100[:4] == report[(mode, 1)][1]["fort100"].splitlines()
    assert f100[4].split()[1] == "0"
    assert lines.count(" - solve p:") == 1 and lines.count(" --- summary ---") == 1 and sum(ln.startswith("ite =") for ln in lines) == 3
