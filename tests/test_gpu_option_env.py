"""The environment variables that preset a run-time option at mgx_init, one by one against tests/golden/options_surface.json (recorded
from the library as it was when mgx_init read them in a block of getenv lines of its own)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_option_environment_presets():
    """Each variable in a fresh process (mgx_init reads the environment; tests/_options_surface_worker.py): nhydro_init at 32x32x8, then
    mgx_get_option of the option it presets.  Each child under its own time limit; the first failure ends the test."""
    with open(os.path.join(ROOT, "tests", "golden", "options_surface.json")) as f:
        cases = json.load(f)["env"]
    assert len(cases) == 12
    for c in cases:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_options_surface_worker.py"), "env", c["variable"], c["value"], c["option"]],
                             capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, (c, out.stdout[-2000:], out.stderr[-2000:])
        got = [l for l in out.stdout.splitlines() if l.startswith("VALUE")][-1].split()[1]
        print(c["variable"], c["value"], c["option"], got)
        assert int(got) == c["expect"], (c, got)
