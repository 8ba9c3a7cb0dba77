"""The host half of the state in the model's own padded arrays (include/mgx.h: the *_view entries), no GPU: what strides
mgx_state_strides_check takes and refuses -- the pure function of mgroms_amd/csrc/mgx_state_view.h, which the view entries call before they
launch anything -- and that the header, the ctypes table and the library agree on the new symbols."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = NX, NY, NZ = 12, 10, 8
NEW = {"mgx_state_strides_check", "mgx_solve_device_view", "mgx_check_nondivergence_device_view", "mgx_update_zeta_device_view"}
FIELDS = ("u_sj", "u_sk", "v_sj", "v_sk", "w_sj", "w_sk")
# row length and rows per level of u(1:nx+1,0:ny+1,1:nz), v(0:nx+1,1:ny+1,1:nz), w(0:nx+1,0:ny+1,0:nz)
LEN = {"u": NX + 1, "v": NX + 2, "w": NX + 2}
ROWS = {"u": NY + 2, "v": NY + 1, "w": NY + 2}


@pytest.fixture(scope="module")
def nhydro():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    nhydro.set_verbose(0)
    return nhydro


def _dense():
    return {a + "_sj": LEN[a] for a in "uvw"} | {a + "_sk": LEN[a] * ROWS[a] for a in "uvw"}


def _tuple(s):
    return tuple(s[f] for f in FIELDS)


def test_dense_and_enlarged_strides_are_accepted(nhydro):
    d = _dense()
    assert _tuple(d) == (13, 13 * 12, 14, 14 * 11, 14, 14 * 12)
    nhydro.state_strides_check(*DIMS, _tuple(d))
    # every pitch enlarged: an odd row pitch, levels with ghost rows on top -- and one array at a time
    big = {a + "_sj": LEN[a] + 5 + LEN[a] % 2 for a in "uvw"}
    big |= {a + "_sk": big[a + "_sj"] * (ROWS[a] + 5) + 3 for a in "uvw"}
    assert all(big[a + "_sj"] % 2 == 1 for a in "uvw")
    nhydro.state_strides_check(*DIMS, _tuple(big))
    for f in FIELDS:
        one = dict(d)
        if f.endswith("_sj"):
            one[f] += 1
            one[f[0] + "_sk"] = one[f] * ROWS[f[0]]
        else:
            one[f] += 1
        nhydro.state_strides_check(*DIMS, _tuple(one))
    # the largest extent that fits: the last element's offset in bytes of a double just inside 63 bits
    top = dict(d)
    top["w_sk"] = ((2 ** 63 - 1) // 8 - (ROWS["w"] - 1) * LEN["w"] - (LEN["w"] - 1)) // NZ
    nhydro.state_strides_check(*DIMS, _tuple(top))


def _refused(nhydro, strides, *words):
    from mgroms_amd._lib import MgxError
    with pytest.raises(MgxError) as e:
        nhydro.state_strides_check(*DIMS, _tuple(strides))
    text = str(e.value)
    assert text.startswith("mgx_state_strides_check: "), text
    for w in words:
        assert w in text, (w, text)
    return text


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("value", [0, -1, -(2 ** 62)])
def test_a_stride_that_is_not_positive_is_refused(nhydro, field, value):
    s = _dense()
    s[field] = value
    _refused(nhydro, s, "%s = %d" % (field, value), "of %s is not positive" % field[0])


@pytest.mark.parametrize("array", "uvw")
def test_a_row_stride_below_the_row_length_is_refused(nhydro, array):
    s = _dense()
    s[array + "_sj"] = LEN[array] - 1
    _refused(nhydro, s, "%s_sj = %d" % (array, LEN[array] - 1), "row length of %s, %d" % (array, LEN[array]))


@pytest.mark.parametrize("array", "uvw")
@pytest.mark.parametrize("pad", [0, 5])
def test_a_level_stride_below_the_rows_of_a_level_is_refused(nhydro, array, pad):
    s = _dense()
    s[array + "_sj"] += pad
    s[array + "_sk"] = s[array + "_sj"] * ROWS[array] - 1
    _refused(nhydro, s, "%s_sk = %d" % (array, s[array + "_sk"]), "rows of %s = %d x %d" % (array, s[array + "_sj"], ROWS[array]))


@pytest.mark.parametrize("array", "uvw")
def test_an_extent_beyond_63_bits_is_refused(nhydro, array):
    s = _dense()
    s[array + "_sk"] = 2 ** 62          # (levels - 1) sk overflows a 64-bit integer
    _refused(nhydro, s, "%s_sk = %d" % (array, 2 ** 62), "extent of %s does not fit in 63 bits" % array)
    s = _dense()
    s[array + "_sj"] = 2 ** 62          # sj x rows does
    s[array + "_sk"] = 2 ** 63 - 1
    _refused(nhydro, s, "%s_sj = %d" % (array, 2 ** 62), "extent of %s does not fit in 63 bits" % array)
    s = _dense()
    s[array + "_sk"] = 2 ** 60          # fits as elements, not as bytes of a double
    _refused(nhydro, s, "extent of %s does not fit in 63 bits" % array)
    if array == "w":                    # one element past the largest extent that fits
        s = _dense()
        s["w_sk"] = ((2 ** 63 - 1) // 8 - (ROWS["w"] - 1) * LEN["w"] - (LEN["w"] - 1)) // NZ + 1
        _refused(nhydro, s, "extent of w does not fit in 63 bits")


def test_the_first_bad_array_is_named(nhydro):
    s = _dense()
    s["v_sj"] = 3
    s["w_sk"] = -4
    _refused(nhydro, s, "v_sj = 3")


def test_sizes_and_null_are_refused(nhydro):
    from mgroms_amd._lib import MgxError, lib
    with pytest.raises(MgxError, match="positive sizes"):
        nhydro.state_strides_check(0, NY, NZ, _tuple(_dense()))
    assert lib().mgx_state_strides_check(NX, NY, NZ, None) == 1
    assert b"NULL" in lib().mgx_last_error()


def test_the_check_needs_no_live_solver(nhydro):
    """host only: with no mgx_init behind it the check answers, and the view entries refuse in mgx_init's words, not with a fault"""
    from mgroms_amd._lib import MgxError, StateStrides, lib
    nhydro.nhydro_clean()
    nhydro.state_strides_check(*DIMS, _tuple(_dense()))
    s = StateStrides(*_tuple(_dense()))
    for entry in ("mgx_solve_device_view", "mgx_check_nondivergence_device_view"):
        assert getattr(lib(), entry)(None, None, None, ctypes.byref(s), 0, None) == 1
        assert b"mgx_init has not been called" in lib().mgx_last_error()
    assert lib().mgx_update_zeta_device_view(None, NX + 2) == 1
    assert b"mgx_init has not been called" in lib().mgx_last_error()
    for fn in (nhydro.nhydro_solve_view, nhydro.nhydro_check_nondivergence_view):
        with pytest.raises(MgxError, match="mgx_init has not been called"):
            fn(None, None, None)
    with pytest.raises(MgxError, match="mgx_init has not been called"):
        nhydro.nhydro_update_zeta_view(None)


def test_header_table_and_library_agree_on_the_new_symbols(nhydro):
    """the cross-check of tests/test_host_logic.py::test_every_declared_symbol_is_exported, seen from the new entries: declared in
    include/mgx.h, listed in the ctypes table, exported by the library; the struct has the header's six members in its order"""
    from mgroms_amd._lib import SYMBOLS, StateStrides, lib
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    declared = {d for d in re.findall(r"\b(mgx_[a-z_0-9]+)\s*\(", hdr) if not d.endswith("_fn")}
    assert NEW <= declared, NEW - declared
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    L = lib()
    for s in NEW:
        assert hasattr(L, s), s
    m = re.search(r"typedef struct \{ long long ([a-z_, ]+); \} mgx_state_strides;", hdr)
    assert m and tuple(x.strip() for x in m.group(1).split(",")) == FIELDS
    assert tuple(n for n, _ in StateStrides._fields_) == FIELDS and ctypes.sizeof(StateStrides) == 48
    import mgroms_amd
    for name in ("nhydro_solve_view", "nhydro_check_nondivergence_view", "nhydro_update_zeta_view"):
        assert callable(getattr(mgroms_amd, name)) and name in mgroms_amd.__all__
