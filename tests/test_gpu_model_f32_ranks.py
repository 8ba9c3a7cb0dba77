"""The float state on a process grid: 2x2 ranks of 16x16x8 (the smallest block of the 2x2 cases of tests/test_gpu_multirank.py), four
colours, u, v, w cut from one global float32 field.  Each rank (tests/_gpu_model_f32_ranks.py) compares its float output with np.float32
of its block of the oracle on 2x2 emulated ranks, bit for bit, and its b with array_equal."""
import os

import pytest

from _ranks import free_port, run_process_ranks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_float_state_on_2x2_ranks():
    npx, npy, nx, ny, nz = 2, 2, 16, 16, 8
    run_process_ranks(os.path.join(HERE, "_gpu_model_f32_ranks.py"), npx * npy, [npx * npy, npx, npy, free_port(), nx, ny, nz])
