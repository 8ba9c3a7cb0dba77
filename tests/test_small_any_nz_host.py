"""Option "small_any_nz" on the host (no GPU): the option and its counter are plain state (include/mgx.h)."""
import pytest


@pytest.fixture(scope="module")
def nh():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    keep = nhydro.get_option("small_any_nz")
    yield nhydro
    nhydro.set_option("small_any_nz", keep)


def test_default(nh):
    """off until asked for: it changes the launch counts of the small levels with nz = 3, 5, 6, 7"""
    assert nh.get_option("small_any_nz") == 0


def test_takes_0_and_1(nh):
    for v in (0, 1, 0, 1):
        nh.set_option("small_any_nz", v)
        assert nh.get_option("small_any_nz") == v


@pytest.mark.parametrize("value", [2, -1])
def test_other_values_refused(nh, value):
    from mgroms_amd._lib import MgxError
    before = nh.get_option("small_any_nz")
    with pytest.raises(MgxError, match=r"small_any_nz must be 1 \(.*\) or 0 \(.*\), got %d" % value):
        nh.set_option("small_any_nz", value)
    assert nh.get_option("small_any_nz") == before


def test_survives_clean(nh):
    for v in (1, 0):
        nh.set_option("small_any_nz", v)
        nh.nhydro_clean()
        assert nh.get_option("small_any_nz") == v


def test_counter_reads_zero_and_is_read_only(nh):
    from mgroms_amd._lib import MgxError
    assert nh.get_option("small_any_nz_calls") == 0
    with pytest.raises(MgxError, match="small_any_nz_calls"):
        nh.set_option("small_any_nz_calls", 1)
    assert nh.get_option("small_any_nz_calls") == 0


def test_documented_beside_mixed_tail():
    """include/mgx.h documents the option and its counter in the form tests/test_host_logic.py reads ("name" (default ...))"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")).read()
    assert "small_any_nz" in set(re.findall(r'"([a-z_0-9]+)" \(default', hdr))
    assert '"small_any_nz_calls"' in hdr
