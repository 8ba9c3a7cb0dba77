"""The walking form of the fused residual + restriction with slots 4 and 7 generated in registers (k_residual_restrict<..., ZW>,
mgx_resrest.hip) against the same form with the slots streamed (MGX_RESREST_NO_ZW) and against the two separate kernels
(MGX_NO_RESREST): identical bits for every level's b and p after two V-cycles and for the history of two solve_p iterations (the NORM
instance and its second destination).  MGX_RESREST_FLAT_MAX=0 sends every level through the walk.  The shapes are the smallest at
which the kernel can go wrong:
  nz2          (8, 8, 2)     no interior row: the stored rows 1 and nz alone (a level of two rows is the coarsest of its hierarchy, so
                             no launch restricts from it today: the case holds the three paths together should that change)
  nz4          (8, 8, 4)     two interior rows
  ragged       (24, 72, 12)  coarse ny = 36: dead lanes shadow a live column and take part in both exchanges; four planes per workgroup; nz no
                             power of two
  empty_wave   (12, 8, 6)    coarse nx = 6, four planes per workgroup: two waves without a plane beside two live ones (mgx_init refuses a
                             level with an odd nx, such as the 5 of a (10, 8, 8) grid, so 6 is the smallest coarse nx with such waves)
  periodic     (32, 16, 8)   east-west and north-south wrap: the halo columns of h and zeta are wrapped values, not mirrors
  moving       (16, 16, 8)   nhydro_matrices a second time with another zeta: the depths follow the 2-D fields
  bmask, user_matrix (16, 16, 8)  the level does not carry what the generated form needs: the launch must not take it (generated slots on
                             a masked or a user matrix would change the bits)
Every case on a stretched sigma coordinate (theta_s = 6, theta_b = 0.4, hc = 250) with a free surface that is not flat: on a uniform
coordinate zw is linear in k, and a depth taken from the wrong row would leave the slots what they are.
The switches are read once per process: each path is a child process (tests/_gpu_resrest_zw_worker.py), the three of a case side by side."""
import os
import sys

import numpy as np
import pytest

from _ranks import run_commands

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"generated": {}, "stored": {"MGX_RESREST_NO_ZW": "1"}, "two_kernels": {"MGX_NO_RESREST": "1"}}


CASES = ["nz2", "nz4", "ragged", "empty_wave", "periodic", "moving", "bmask", "user_matrix"]
_results = {}


def _paths(case, tmp_path_factory):
    """the three paths of a case, each in a process of its own, side by side: run once, shared by the tests below and left unchanged"""
    if case in _results:
        return _results[case]
    tmp = tmp_path_factory.mktemp(case)
    cmds = []
    for name, var in PATHS.items():
        env = dict(os.environ, MGX_RESREST_FLAT_MAX="0")
        for k in ("MGX_RESREST_NO_ZW", "MGX_NO_RESREST", "MGX_NO_MF", "MGX_RESREST_AHEAD", "MGX_RESREST_MIN"):
            env.pop(k, None)
        env.update(var)
        cmds.append(([sys.executable, os.path.join(HERE, "_gpu_resrest_zw_worker.py"), case, str(tmp / f"{name}.npz")], env))
    res = {}
    for name, pr in zip(PATHS, run_commands(cmds, timeout=120)):
        assert pr.returncode == 0, (name, pr.stdout[-2000:], pr.stderr[-2000:])
        res[name] = dict(np.load(tmp / f"{name}.npz"))
    _results[case] = res
    return res


def _different(res, keys):
    ref = res["two_kernels"]
    return [(name, k, float(np.abs(res[name][k] - ref[k]).max())) for name in ("generated", "stored") for k in keys
            if not np.array_equal(res[name][k], ref[k])]


@pytest.mark.parametrize("case", CASES)
def test_generated_slots_same_fields(case, tmp_path_factory):
    """every level's b and p after two V-cycles, and level 1's p after two solve_p iterations (the NORM instance and its second
    destination feed the second iteration): the three paths agree bit for bit"""
    res = _paths(case, tmp_path_factory)
    ref = res["two_kernels"]
    assert np.all(np.isfinite(ref["first_hist"]))
    assert case == "nz2" or "first_b2" in ref   # a level with nz = 2 is the coarsest one: nothing below it to restrict to
    if case == "moving":
        assert not np.array_equal(ref["first_b2"], ref["second_b2"])   # the second surface changed the matrix
    for name in ("generated", "stored"):
        assert sorted(res[name]) == sorted(ref)
    bad = _different(res, [k for k in sorted(ref) if not k.endswith("_hist")])
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", CASES)
def test_generated_slots_same_history(case, tmp_path_factory):
    """the history of two solve_p iterations: the three paths agree bit for bit.

    The fused kernel adds the squares per workgroup of 4 planes x 32 coarse columns, compute_residual per workgroup of its own shape:
    as plain sums the two differed by one unit in the last place of one entry in the cases nz4 and periodic (1.7e-18 on a relative
    residual of 1e-2 .. 1e-4), with the fields equal.  Every residual norm is therefore carried as a pair (dd_add, mgx_device.h),
    which holds the sum to ~2^-100 and is rounded once, so the grouping no longer reaches the result."""
    res = _paths(case, tmp_path_factory)
    hist = [k for k in sorted(res["two_kernels"]) if k.endswith("_hist")]
    assert all(np.array_equal(res["generated"][k], res["stored"][k]) for k in hist), case
    bad = _different(res, hist)
    assert not bad, (case, bad)
