"""The matrices from the caller's own depths through the Fortran boundary: fortran/testdepths_gpu (mg_testdepths_gpu.f90) solves a flat
bottom at 32x32x16 once after nhydro_matrices and once, in a new nhydro_init, after nhydro_matrices_depths on the zr, zw that grid_get
returned from the first set-up.  Every residual the second solve prints equals the first's, character for character."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fortran_depths_on_a_flat_bottom(tmp_path):
    exe = os.path.join(ROOT, "fortran", "testdepths_gpu")
    if not os.path.exists(exe) and shutil.which("flang") is None:
        pytest.skip("flang not available when build() ran")
    assert os.path.exists(exe), "build() did not make fortran/testdepths_gpu"
    (tmp_path / "nh_namelist").write_text("&nhparam\n relax_method = 'FC',\n solver_prec = 1.d-8,\n/\n")
    out = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    # the library prints through C's stdio and the program through the Fortran runtime: under a pipe the two are buffered apart, so the
    # separator the program writes does not divide the library's lines.  Two solves ran; their residual lines are the two halves.
    assert out.stdout.count("---- depths ----") == 1 and out.stdout.count("nhydro_solve:") == 2, out.stdout[-2000:]
    assert out.stdout.count("nhydro_matrices (depths):") == 1, out.stdout[-2000:]
    lines = re.findall(r"ite = *\d+: res = .*", out.stdout)
    n = len(lines) // 2
    print("\n".join(lines[n:]))
    assert n >= 2 and len(lines) == 2 * n and lines[:n] == lines[n:], lines
    assert [int(re.match(r"ite = *(\d+)", l).group(1)) for l in lines] == 2 * list(range(1, n + 1))
