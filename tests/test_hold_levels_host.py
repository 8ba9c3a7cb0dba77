"""Option "hold_odd_nz" as host logic (include/mgx.h): no GPU needed.

The level table of the pure entry mgx_level_table_hold: level l + 1 exists iff l < nl1 (the horizontal bound) and nz_l != 2, with
nz_{l+1} = nz_l / 2 for an even nz_l and nz_l for an odd one; nx, ny and the gathers are those of the reference's table.  A size whose nz
stays even down to 2 has the same table with the option and without.  The option itself is plain state like "periodic": 0 by default, 0 and
1 are taken and outlive mgx_clean, anything else is refused in words that name it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(*a, **kw):
    from mgroms_amd import nhydro
    return nhydro.level_table(*a, **kw)


def _dims(t):
    return [(l["nx"], l["ny"], l["nz"]) for l in t]


def test_128x128x40():
    t = _table(128, 128, 40, hold_odd_nz=1)
    assert [l["nz"] for l in t] == [40, 20, 10, 5, 5, 5]
    assert [(l["nx"], l["ny"]) for l in t] == [(128 >> q, 128 >> q) for q in range(6)]
    assert [l["nz"] for l in _table(128, 128, 40)] == [40, 20, 10, 5, 2]   # the reference's table: the odd level is not the coarsest


def test_64x64x28():
    assert [l["nz"] for l in _table(64, 64, 28, hold_odd_nz=1)] == [28, 14, 7, 7, 7]


def test_48x80x12_planes():
    assert _dims(_table(48, 80, 12, hold_odd_nz=1)) == [(48, 80, 12), (24, 40, 6), (12, 20, 3), (6, 10, 3)]


def test_64x64x24():
    assert [l["nz"] for l in _table(64, 64, 24, hold_odd_nz=1)] == [24, 12, 6, 3, 3]


def test_512x512x48_ends_4x4x3():
    t = _table(512, 512, 48, hold_odd_nz=1)
    assert len(t) == 8
    assert [l["nz"] for l in t] == [48, 24, 12, 6, 3, 3, 3, 3]
    assert _dims(t)[-1] == (4, 4, 3)
    assert _dims(_table(512, 512, 48))[-1] == (32, 32, 3)


@pytest.mark.parametrize("rank", range(4))
def test_2x2_ranks_gather_where_the_default_table_has_them(rank):
    """2 x 2 ranks of 16 x 16 x 20, nsmall = 8: the default table has nz 20, 10, 5, 2 and gathers level 3; the held one differs from it in the
    nz of level 4 and in nothing else"""
    held = _table(16, 16, 20, 2, 2, rank, 8, hold_odd_nz=1)
    base = _table(16, 16, 20, 2, 2, rank, 8)
    assert [l["nz"] for l in held] == [20, 10, 5, 5] and [l["nz"] for l in base] == [20, 10, 5, 2]
    assert held[:3] == base[:3] and {k: v for k, v in held[3].items() if k != "nz"} == {k: v for k, v in base[3].items() if k != "nz"}
    assert [l["gather"] for l in held] == [0, 0, 1, 0]
    assert _dims(held) == [(16, 16, 20), (8, 8, 10), (8, 8, 5), (4, 4, 5)]
    assert (held[3]["npx"], held[3]["npy"]) == (1, 1) and held[3]["neighb"] == [-1] * 8
    # the planes and gathers are those of a size that halves without an odd level: 16 x 16 x 64 on the same grid
    even = _table(16, 16, 64, 2, 2, rank, 8)
    keys = [k for k in held[0] if k != "nz"]
    assert [[l[k] for k in keys] for l in held] == [[l[k] for k in keys] for l in even[:4]]


@pytest.mark.parametrize("cfg", [(64, 64, 16, 1, 1), (512, 512, 64, 1, 1), (512, 1024, 128, 4, 2), (32, 32, 24, 1, 1)])
def test_no_odd_level_above_the_coarsest_same_table(cfg):
    nx, ny, nz, npx, npy = cfg
    for rank in range(npx * npy):
        assert _table(nx, ny, nz, npx, npy, rank, 8, hold_odd_nz=1) == _table(nx, ny, nz, npx, npy, rank, 8)


def test_periodic_and_hold_together_and_bad_arguments():
    from mgroms_amd import nhydro
    from mgroms_amd._lib import lib
    t = nhydro.level_table_periodic(32, 32, 20, 1, 1, 0, 8, 3, hold_odd_nz=1)
    assert [l["nz"] for l in t] == [20, 10, 5, 5]
    assert all(l["neighb"] == [0] * 8 for l in t)
    assert nhydro.level_table_periodic(32, 32, 20, 1, 1, 0, 8, 3)[:3] == t[:3]
    out = (ctypes.c_int * (20 * 32))()
    assert lib().mgx_level_table_hold(32, 32, 20, 1, 1, 0, 8, 0, 2, 32, out) == -1
    assert lib().mgx_level_table_hold(32, 32, 20, 1, 1, 0, 8, 0, -1, 32, out) == -1
    assert lib().mgx_level_table_hold(32, 32, 20, 1, 1, 0, 8, 0, 0, 32, out) == 4 and out[20 * 3 + 2] == 2
    assert lib().mgx_level_table_hold(32, 32, 20, 1, 1, 0, 8, 0, 1, 32, out) == 4 and out[20 * 3 + 2] == 5


def test_mixed_tail_first_describes_the_default_hierarchy():
    from mgroms_amd import nhydro
    before = nhydro.mixed_tail_first(128, 128, 40)
    nhydro.set_option("hold_odd_nz", 1)
    try:
        assert nhydro.mixed_tail_first(128, 128, 40) == before
    finally:
        nhydro.set_option("hold_odd_nz", 0)


# ---- the option surface ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def L():
    from mgroms_amd._lib import lib
    L = lib()
    yield L
    L.mgx_clean()
    assert L.mgx_set_option(b"hold_odd_nz", 0) == 0


def _get(L):
    v = ctypes.c_int(-12345)
    assert L.mgx_get_option(b"hold_odd_nz", ctypes.byref(v)) == 0, L.mgx_last_error()
    return v.value


def test_default_set_get_and_mgx_clean(L):
    assert _get(L) == 0
    assert L.mgx_set_option(b"hold_odd_nz", 1) == 0, L.mgx_last_error()
    assert _get(L) == 1
    L.mgx_clean()
    assert _get(L) == 1   # carried over mgx_clean: mgx_init, which reads it, starts with one
    assert L.mgx_set_option(b"hold_odd_nz", 0) == 0
    assert _get(L) == 0
    L.mgx_clean()
    assert _get(L) == 0


@pytest.mark.parametrize("value", [2, -1])
def test_other_values_are_refused_by_name(L, value):
    assert L.mgx_set_option(b"hold_odd_nz", 1) == 0
    assert L.mgx_set_option(b"hold_odd_nz", value) != 0
    text = L.mgx_last_error().decode()
    assert "hold_odd_nz" in text and str(value) in text, text
    assert _get(L) == 1   # the refused value left the option alone


def test_no_environment_variable(L):
    """options_from_env runs inside mgx_init only; the table gives the option no variable at all: nothing named after it is read"""
    src = open(os.path.join(ROOT, "mgroms_amd", "csrc", "mgx_api.cpp")).read()
    row = [l for l in src.splitlines() if l.lstrip().startswith('{"hold_odd_nz"')]
    assert len(row) == 1 and "ENV_NONE" in row[0] and "MGX_" not in row[0], row


def test_documented_in_the_header_form():
    """the `"name" (default ...)` form tests/test_host_logic.py::test_documented_options_exist reads"""
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "hold_odd_nz" in set(re.findall(r'"([a-z_0-9]+)" \(default', hdr))
    assert '"hold_odd_nz" (default 0' in hdr
