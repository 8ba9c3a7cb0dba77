"""CPU tests of the float state (include/mgx.h: "the float state"): the five entries are exported, the Python dispatch on the dtype of u, v, w
refuses what it cannot serve before it touches the library, and the library refuses a call before mgx_init in its own words."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mgx_solve_device_f32", "mgx_check_nondivergence_device_f32", "mgx_solve_f32", "mgx_compute_rhs_f32", "mgx_check_nondivergence_f32")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import mgroms_amd
    return mgroms_amd


def test_float_entries_are_declared_and_exported(built):
    from mgroms_amd._lib import SYMBOLS, lib
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    L = lib()
    for name in ENTRIES:
        assert name in SYMBOLS and hasattr(L, name), name
        assert ("int %s(" % name) in hdr, name


def test_mixed_dtypes_are_refused_without_the_library(built, monkeypatch):
    """u, v, w of two dtypes, or of a dtype that is neither float64 nor float32: ValueError from the dispatch itself -- lib() is never asked for"""
    from mgroms_amd import nhydro

    def no_library():
        raise AssertionError("the dispatch touched the library")
    monkeypatch.setattr(nhydro, "lib", no_library)
    nx, ny, nz = 4, 4, 2
    shapes = ((nz, ny + 2, nx + 1), (nz, ny + 1, nx + 2), (nz + 1, ny + 2, nx + 2))
    u, v, w = (np.zeros(s, dtype=np.float32) for s in shapes)
    for st in ((u, v.astype(np.float64), w), (u.astype(np.float64), v, w.astype(np.float64)), tuple(a.astype(np.float16) for a in (u, v, w)),
               tuple(a.astype(np.int32) for a in (u, v, w))):
        for fn in (nhydro.nhydro_solve, nhydro.nhydro_check_nondivergence, nhydro.compute_rhs, nhydro.nhydro_solve_device,
                   nhydro.nhydro_check_nondivergence_device):
            with pytest.raises(ValueError, match="float64 or float32"):
                fn(*st)


def test_solve_f32_before_init_fails_in_the_librarys_words(built):
    from mgroms_amd._lib import MgxError, check, lib
    L = lib()
    L.mgx_clean()
    a = np.zeros(8, dtype=np.float32)
    p = a.ctypes.data_as(C.POINTER(C.c_float))
    for name in ("mgx_solve_f32", "mgx_compute_rhs_f32", "mgx_check_nondivergence_f32"):
        with pytest.raises(MgxError, match="mgx_init has not been called"):
            check(getattr(L, name)(p, p, p, None))
    for name in ("mgx_solve_device_f32", "mgx_check_nondivergence_device_f32"):
        with pytest.raises(MgxError, match="mgx_init has not been called"):
            check(getattr(L, name)(None, None, None, None))
