"""The host half of the matrices from the caller's own depths (include/mgx.h: mgx_matrices_depths*), no GPU:

  * what strides mgx_depth_strides_check takes and refuses -- the pure function of mgroms_amd/csrc/mgx_depth_view.h, which the device entries
    call before they launch anything -- pinned as tests/test_state_view_host.py pins its twin;
  * the coarsening rule of the depths (tests/_depths.py: coarsen_depths) against the CPU oracle's sigma hierarchy on a flat
    bottom, where the two must agree bit for bit on every level: that is why a coarse rho point is a fine interface;
  * the launches of the kernels of mgx_depths.hip (mgx_choice_depths.h through mgx_depths_launch) over the shapes the GPU tests run and the
    two of scripts/depths_time.py, restated here from their rule and held to cover every element."""
import ctypes
import os
import re

import numpy as np
import pytest

from _depths import coarsen_depths, hierarchy, interior, old_s_depths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = NX, NY, NZ = 12, 10, 8
NEW = {"mgx_depth_strides_check", "mgx_matrices_depths", "mgx_matrices_depths_device", "mgx_update_depths_device", "mgx_depths_launch"}
FIELDS = ("zr_sj", "zr_sk", "zw_sj", "zw_sk")
LEVELS = {"zr": NZ, "zw": NZ + 1}


@pytest.fixture(scope="module")
def nhydro():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    nhydro.set_verbose(0)
    return nhydro


def _dense():
    """the strides of arrays (levels, ny, nx) with nothing between rows or levels"""
    return {"zr_sj": NX, "zr_sk": NX * NY, "zw_sj": NX, "zw_sk": NX * NY}


def _tuple(s):
    return tuple(s[f] for f in FIELDS)


def test_dense_and_enlarged_strides_are_accepted(nhydro):
    nhydro.depth_strides_check(*DIMS, _tuple(_dense()))
    big = {a + "_sj": NX + 7 for a in ("zr", "zw")}          # ghost cells and an odd pitch
    big |= {a + "_sk": big[a + "_sj"] * (NY + 5) + 3 for a in ("zr", "zw")}
    nhydro.depth_strides_check(*DIMS, _tuple(big))
    for f in FIELDS:
        one = dict(_dense())
        one[f] += 1
        if f.endswith("_sj"):
            one[f[:2] + "_sk"] = one[f] * NY
        nhydro.depth_strides_check(*DIMS, _tuple(one))
    top = dict(_dense())     # the largest extent that fits: the last element's offset in bytes of a double just inside 63 bits
    top["zw_sk"] = ((2 ** 63 - 1) // 8 - (NY - 1) * NX - (NX - 1)) // NZ
    nhydro.depth_strides_check(*DIMS, _tuple(top))


def _refused(nhydro, strides, *words):
    from mgroms_amd._lib import MgxError
    with pytest.raises(MgxError) as e:
        nhydro.depth_strides_check(*DIMS, _tuple(strides))
    text = str(e.value)
    assert text.startswith("mgx_depth_strides_check: "), text
    for w in words:
        assert w in text, (w, text)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("value", [0, -1, -(2 ** 62)])
def test_a_stride_that_is_not_positive_is_refused(nhydro, field, value):
    s = _dense()
    s[field] = value
    _refused(nhydro, s, "%s = %d" % (field, value), "of %s is not positive" % field[:2])


@pytest.mark.parametrize("array", ["zr", "zw"])
def test_a_row_stride_below_the_row_length_is_refused(nhydro, array):
    s = _dense()
    s[array + "_sj"] = NX - 1
    _refused(nhydro, s, "%s_sj = %d" % (array, NX - 1), "row length of %s, %d" % (array, NX), "rows would overlap")


@pytest.mark.parametrize("array", ["zr", "zw"])
@pytest.mark.parametrize("pad", [0, 5])
def test_a_level_stride_below_the_rows_of_a_level_is_refused(nhydro, array, pad):
    s = _dense()
    s[array + "_sj"] += pad
    s[array + "_sk"] = s[array + "_sj"] * NY - 1
    _refused(nhydro, s, "%s_sk = %d" % (array, s[array + "_sk"]), "rows of %s = %d x %d" % (array, s[array + "_sj"], NY), "levels would overlap")


@pytest.mark.parametrize("array", ["zr", "zw"])
def test_an_extent_beyond_63_bits_is_refused(nhydro, array):
    s = _dense()
    s[array + "_sk"] = 2 ** 62
    _refused(nhydro, s, "%s_sk = %d" % (array, 2 ** 62), "extent of %s does not fit in 63 bits" % array)
    s = _dense()
    s[array + "_sj"] = 2 ** 62
    s[array + "_sk"] = 2 ** 63 - 1
    _refused(nhydro, s, "%s_sj = %d" % (array, 2 ** 62), "extent of %s does not fit in 63 bits" % array)
    s = _dense()
    s[array + "_sk"] = 2 ** 60          # fits as elements, not as bytes of a double
    _refused(nhydro, s, "extent of %s does not fit in 63 bits" % array)
    s = _dense()                        # one element past the largest extent that fits
    s[array + "_sk"] = ((2 ** 63 - 1) // 8 - (NY - 1) * NX - (NX - 1)) // (LEVELS[array] - 1) + 1
    _refused(nhydro, s, "extent of %s does not fit in 63 bits" % array)


def test_the_first_bad_array_is_named_and_sizes_and_null_are_refused(nhydro):
    from mgroms_amd._lib import MgxError, lib
    s = _dense()
    s["zr_sj"] = 3
    s["zw_sk"] = -4
    _refused(nhydro, s, "zr_sj = 3")
    with pytest.raises(MgxError, match="positive sizes"):
        nhydro.depth_strides_check(0, NY, NZ, _tuple(_dense()))
    assert lib().mgx_depth_strides_check(NX, NY, NZ, None) == 1
    assert b"NULL" in lib().mgx_last_error()


def test_the_entries_need_a_live_solver_and_the_check_does_not(nhydro):
    """with no mgx_init behind them the depth entries refuse in mgx_init's words, not with a fault; the check answers"""
    from mgroms_amd._lib import DepthStrides, MgxError, lib
    nhydro.nhydro_clean()
    nhydro.depth_strides_check(*DIMS, _tuple(_dense()))
    s = DepthStrides(*_tuple(_dense()))
    L = lib()
    assert L.mgx_matrices_depths(None, None, None, None, None) == 1 and b"mgx_init has not been called" in L.mgx_last_error()
    assert L.mgx_matrices_depths_device(None, None, None, None, ctypes.byref(s), None) == 1 and b"mgx_init has not been called" in L.mgx_last_error()
    assert L.mgx_update_depths_device(None, None, ctypes.byref(s)) == 1 and b"mgx_init has not been called" in L.mgx_last_error()
    for fn, n in ((nhydro.nhydro_matrices_depths, 4), (nhydro.nhydro_matrices_depths_device, 4), (nhydro.nhydro_update_depths_device, 2)):
        with pytest.raises(MgxError, match="mgx_init has not been called"):
            fn(*([None] * n))


def test_header_table_and_library_agree_on_the_new_symbols(nhydro):
    from mgroms_amd._lib import SYMBOLS, DepthStrides, lib
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    declared = {d for d in re.findall(r"\b(mgx_[a-z_0-9]+)\s*\(", hdr) if not d.endswith("_fn")}
    assert NEW <= declared, NEW - declared
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    for s in NEW:
        assert hasattr(lib(), s), s
    m = re.search(r"typedef struct \{ long long ([a-z_, ]+); \} mgx_depth_strides;", hdr)
    assert m and tuple(x.strip() for x in m.group(1).split(",")) == FIELDS
    assert tuple(n for n, _ in DepthStrides._fields_) == FIELDS and ctypes.sizeof(DepthStrides) == 32
    import mgroms_amd
    for name in ("nhydro_matrices_depths", "nhydro_matrices_depths_device", "nhydro_update_depths_device"):
        assert callable(getattr(mgroms_amd, name)) and name in mgroms_amd.__all__


# ---- the rule against the oracle's sigma hierarchy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [(4e3, 0.0, 0.0), (250.0, 0.4, 6.0)], ids=["uniform", "stretched"])
@pytest.mark.parametrize("dims,nzs", [((32, 32, 16), [16, 8, 4, 2]), ((32, 16, 24), [24, 12, 6])], ids=["32x32x16", "32x16x24"])
def test_the_rule_is_the_sigma_hierarchy_on_a_flat_bottom(dims, nzs, sigma):
    """Constant h and zeta, dx and dy varying in i and j: zr and zw of every coarser level of the oracle are, bit for bit, the rule applied
    to the level above -- with zr_C a fine INTERFACE.  (The sigma formula at a constant h, zeta gives every column of a level the same
    depths, an average of four equal numbers is that number, and sc_r of the coarse level equals sc_w of the fine one at the even
    interfaces in floating point.)"""
    from _problem import oracle_twin, problem
    nx, ny, nz = dims
    pr = problem(dims, metric="curvilinear", sigma=sigma, relax_method="FC")
    dx, dy, _, _ = pr.fields
    pr.fields = (dx, dy, np.full((nx + 2, ny + 2), 0.3), np.full((nx + 2, ny + 2), 3000.0))
    o = oracle_twin(pr)
    try:
        assert o.nlevs == len(nzs) and [o.level_info(l)["nz"] for l in range(1, o.nlevs + 1)] == nzs
        got = hierarchy(interior(o.field("zr", 1)).copy(), interior(o.field("zw", 1)).copy(), nzs)
        for lev in range(1, o.nlevs + 1):
            zr, zw = got[lev - 1]
            assert np.array_equal(zr, interior(o.field("zr", lev))), ("zr", lev)
            assert np.array_equal(zw, interior(o.field("zw", lev))), ("zw", lev)
    finally:
        o.close()


def test_the_rule_by_hand_and_the_old_s_grid():
    """the summation order and the interfaces each pair reads, on numbers small enough to do by hand; the old-S depths are monotone (the
    helper asserts it) and are not a grid of the library: the spacing of their interfaces at the surface is not the sigma one"""
    zw = np.arange(2 * 2 * 5, dtype=np.float64).reshape(2, 2, 5) ** 2
    zr = 0.5 * (zw[:, :, 1:] + zw[:, :, :-1])
    cr, cw = coarsen_depths(zr, zw, held=False)
    assert cr.shape == (1, 1, 2) and cw.shape == (1, 1, 3)
    for kc in range(3):
        assert cw[0, 0, kc] == 0.25 * (((zw[0, 0, 2 * kc] + zw[0, 1, 2 * kc]) + zw[1, 0, 2 * kc]) + zw[1, 1, 2 * kc])
    for kc in range(2):
        assert cr[0, 0, kc] == 0.25 * (((zw[0, 0, 2 * kc + 1] + zw[0, 1, 2 * kc + 1]) + zw[1, 0, 2 * kc + 1]) + zw[1, 1, 2 * kc + 1])
    hr, hw = coarsen_depths(zr, zw, held=True)
    assert hr.shape == (1, 1, 4) and hw.shape == (1, 1, 5)
    assert hr[0, 0, 3] == 0.25 * (((zr[0, 0, 3] + zr[0, 1, 3]) + zr[1, 0, 3]) + zr[1, 1, 3])
    with pytest.raises(AssertionError, match="odd nz"):
        coarsen_depths(zr[:, :, :3], zw[:, :, :4], held=False)
    h = np.full((4, 4), 3000.0)
    zr, zw = old_s_depths(h, np.zeros((4, 4)), 16)
    assert zw[0, 0, 0] == -3000.0 and zw[0, 0, -1] == 0.0
    uniform = 3000.0 / 16
    assert (zw[0, 0, -1] - zw[0, 0, -2]) < 0.5 * uniform     # stretched towards the surface


# ---- the launches ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(32, 16, 8), (64, 32, 64), (32, 32, 16), (32, 16, 24), (32, 32, 96), (32, 32, 20), (32, 32, 24), (48, 80, 12), (16, 16, 16),
          (64, 64, 16), (24, 16, 12), (64, 64, 40), (32, 32, 5), (512, 512, 64), (512, 1024, 128), (66, 2, 65), (2, 70000, 2)]


@pytest.mark.parametrize("dims", SHAPES, ids=["%dx%dx%d" % d for d in SHAPES])
def test_the_launches_of_the_depth_kernels(nhydro, dims):
    nx, ny, nz = dims
    c = nhydro.depths_launch(nx, ny, nz)
    up = lambda a, b: -(-a // b)
    # the transpose: 64 x 64 tiles of (i, k), zr's k tiles then zw's, one row j per grid.y up to the grid limit, 64 x 65 doubles of LDS
    assert (c["in_i_tiles"], c["in_k_tiles_zr"], c["in_k_tiles_zw"]) == (up(nx, 64), up(nz, 64), up(nz + 1, 64))
    assert c["in_grid_x"] == up(nx, 64) * (up(nz, 64) + up(nz + 1, 64)) and c["in_grid_y"] == min(ny, 65535)
    assert (c["in_block_x"], c["in_block_y"], c["in_lds"]) == (64, 4, 64 * 65 * 8)
    assert c["in_i_tiles"] * 64 >= nx and c["in_k_tiles_zw"] * 64 >= nz + 1 and c["in_lds"] <= 64 * 1024
    # one lane per element: the dense copy, and the coarsening onto level 2 (nz + 1 interfaces per coarse column, nz / 2 + 1 when it halves)
    assert (c["copy_grid"], c["copy_block"]) == (up((2 * nz + 1) * ny * nx, 256), 256)
    nzc = nz if nz % 2 else nz // 2
    assert (c["coarsen_grid"], c["coarsen_block"]) == (up((nzc + 1) * (ny // 2) * (nx // 2), 256), 256)
    assert (c["hz_grid_x"], c["hz_grid_y"], c["hz_block_x"], c["hz_block_y"]) == (up(ny + 2, 64), up(nx + 2, 4), 64, 4)
    assert c["hz_grid_x"] * 64 >= ny + 2 and c["hz_grid_y"] * 4 >= nx + 2
    # the colour passes that generate from the sigma fields are those from nz = 32 on
    assert c["pass_stored"] == (1 if nz >= 32 else 0)


def test_the_launch_query_refuses_what_is_no_level(nhydro):
    from mgroms_amd._lib import MgxError, lib
    with pytest.raises(MgxError, match="31 x 16 x 8 is not a level-1 size"):
        nhydro.depths_launch(31, 16, 8)
    assert lib().mgx_depths_launch(32, 16, 8, None) == 1 and b"out is NULL" in lib().mgx_last_error()
