"""The float state through the Fortran boundary: fortran/testsolve_r4_gpu (mg_testsolve_r4_gpu.f90) solves the seamount at 32x32x8 once
with a real(8) and once with a real(4) state through module nhydro (nhydro_solve, nhydro_solve_r4) and prints how many elements of
real(u8, 4) and u4 differ in their bits, likewise for v and w, and both iteration counts."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fortran_float_state(tmp_path):
    exe = os.path.join(ROOT, "fortran", "testsolve_r4_gpu")
    if not os.path.exists(exe) and shutil.which("flang") is None:
        pytest.skip("flang not available when build() ran")
    assert os.path.exists(exe), "build() did not make fortran/testsolve_r4_gpu"
    (tmp_path / "nh_namelist").write_text("&nhparam\n relax_method = 'FC',\n solver_prec = 1.d-8,\n/\n")
    out = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]

    def num(name):
        m = re.search(name + r" = *(-?\d+)", out.stdout)
        assert m, (name, out.stdout[-2000:])
        return int(m.group(1))

    assert (num("bits_differ_u"), num("bits_differ_v"), num("bits_differ_w")) == (0, 0, 0), out.stdout[-1500:]
    assert num("nite_r8") == num("nite_r4") and num("nite_r8") >= 2, out.stdout[-1500:]
    # both solves printed their iterations, in the reference's format
    assert len(re.findall(r"ite = *(\d+): res = ", out.stdout)) == 2 * num("nite_r8")
