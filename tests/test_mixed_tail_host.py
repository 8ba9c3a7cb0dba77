"""Option "mixed_tail" on the host (no GPU): the option and its counter are plain state, and which levels of a one-rank hierarchy form the
tail of an fp32 cycle is pure host logic (mgx_mixed_tail_first): the run of coarsest levels with at most 32768 cells and nz <= 32."""
import pytest


@pytest.fixture(scope="module")
def nh():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    keep = nhydro.get_option("mixed_tail")
    yield nhydro
    nhydro.set_option("mixed_tail", keep)


def test_default(nh):
    """off until asked for: it changes the launch count mgx_counters reports for an fp32 cycle"""
    assert nh.get_option("mixed_tail") == 0


def test_takes_0_and_1(nh):
    for v in (0, 1, 0, 1):
        nh.set_option("mixed_tail", v)
        assert nh.get_option("mixed_tail") == v


@pytest.mark.parametrize("value", [2, -1])
def test_other_values_refused(nh, value):
    from mgroms_amd._lib import MgxError
    before = nh.get_option("mixed_tail")
    with pytest.raises(MgxError, match="mixed_tail"):
        nh.set_option("mixed_tail", value)
    assert nh.get_option("mixed_tail") == before


def test_survives_clean(nh):
    for v in (0, 1):
        nh.set_option("mixed_tail", v)
        nh.nhydro_clean()
        assert nh.get_option("mixed_tail") == v


def test_counter_reads_zero_and_is_read_only(nh):
    from mgroms_amd._lib import MgxError
    assert nh.get_option("mixed_tail_launches") == 0
    with pytest.raises(MgxError, match="mixed_tail_launches"):
        nh.set_option("mixed_tail_launches", 1)


# level sizes: nx, ny, nz halve from level to level
#   512x512x64: level 4 = 64x64x8 = 32768 cells          512x1024x128: level 4 = 64x128x16 = 131072, level 5 = 32x64x8 = 16384
#   64x64x16: level 1 = 65536, level 2 = 8192            128x64x32: level 2 = 64x32x16 = exactly 32768 (the bound is inclusive)
#   32x32x24: level 1 = 24576, every level small         16x16x2: a single level
#   32x16x64: level 1 has 32768 cells but nz = 64 > 32
TAIL_FIRST = [((512, 512, 64), 4), ((512, 1024, 128), 5), ((64, 64, 16), 2), ((128, 64, 32), 2), ((32, 32, 24), 1), ((16, 16, 2), 1),
              ((32, 16, 64), 2)]


@pytest.mark.parametrize("dims,first", TAIL_FIRST, ids=["x".join(map(str, d)) for d, _ in TAIL_FIRST])
def test_tail_first(nh, dims, first):
    assert nh.mixed_tail_first(*dims) == first
    # against the level table: `first` is the finest level from which every level is small
    small = [d["nx"] * d["ny"] * d["nz"] <= 32768 and d["nz"] <= 32 for d in nh.level_table(*dims)]
    assert all(small[first - 1:]) and not any(small[:first - 1])


def test_no_small_level(nh):
    """a hierarchy that ends above the bound has no tail: 256x256x4 has the two levels 256x256x4 and 128x128x2 = 32768 cells -- one more
    cell and there is none (512x256x4: 128x256x2 = 65536)"""
    assert nh.mixed_tail_first(256, 256, 4) == 2
    assert nh.mixed_tail_first(512, 256, 4) == 0


def test_bad_sizes_refused(nh):
    from mgroms_amd._lib import MgxError
    with pytest.raises(MgxError, match="mgx_mixed_tail_first"):
        nh.mixed_tail_first(1, 16, 2)
