"""Option "periodic" as plain state (include/mgx.h): no GPU needed.  A bit mask, 0 by default; 1, 2 and 3 are taken and outlive mgx_clean
(mgx_init reads the option, so it has to survive the mgx_clean that mgx_init starts with); anything else is refused in words that name
the option.  The level table of a single rank with the option set is checked where it acts, on the GPU (tests/test_gpu_periodic.py)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def L():
    from mgroms_amd._lib import lib
    L = lib()
    yield L
    L.mgx_clean()
    assert L.mgx_set_option(b"periodic", 0) == 0


def _get(L):
    v = ctypes.c_int(-12345)
    assert L.mgx_get_option(b"periodic", ctypes.byref(v)) == 0, L.mgx_last_error()
    return v.value


def test_default_values_and_mgx_clean(L):
    assert _get(L) == 0
    for value in (1, 2, 3):
        assert L.mgx_set_option(b"periodic", value) == 0, L.mgx_last_error()
        assert _get(L) == value
        L.mgx_clean()
        assert _get(L) == value   # carried over mgx_clean
    assert L.mgx_set_option(b"periodic", 0) == 0
    assert _get(L) == 0


@pytest.mark.parametrize("value", [4, -1])
def test_other_values_are_refused_by_name(L, value):
    assert L.mgx_set_option(b"periodic", 2) == 0
    assert L.mgx_set_option(b"periodic", value) != 0
    text = L.mgx_last_error().decode()
    assert "periodic" in text and str(value) in text, text
    assert _get(L) == 2   # the refused value left the option alone


def test_documented_in_the_header_form():
    """the `"name" (default ...)` form tests/test_host_logic.py::test_documented_options_exist reads"""
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "periodic" in set(re.findall(r'"([a-z_0-9]+)" \(default', hdr))
