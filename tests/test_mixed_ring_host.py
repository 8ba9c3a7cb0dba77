"""Option "mixed_ring" on the host (no GPU): the option and its counter are plain state, and which levels of a one-rank hierarchy the
pipelined fp32 colour pass (k_relax32r, mgx_mixed.hip) serves is pure host logic (mgx_mixed_ring_levels over choose_relax32, mgx_choice.h):
nz one of 16, 20, 24, 32, 40, 48, 64 and the level not small in the sense of option "mixed_tail" (more than 32768 cells, or nz > 32)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nh():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    keep = nhydro.get_option("mixed_ring")
    yield nhydro
    nhydro.set_option("mixed_ring", keep)


def test_default(nh):
    """off until asked for: 0 is every launch and every bit of the row-by-row kernel"""
    assert nh.get_option("mixed_ring") == 0


def test_takes_0_and_1(nh):
    for v in (0, 1, 0, 1):
        nh.set_option("mixed_ring", v)
        assert nh.get_option("mixed_ring") == v


@pytest.mark.parametrize("value", [-1, 2, 32])
@pytest.mark.parametrize("before", [0, 1])
def test_other_values_refused(nh, value, before):
    from mgroms_amd._lib import MgxError
    nh.set_option("mixed_ring", before)
    with pytest.raises(MgxError, match="mixed_ring"):
        nh.set_option("mixed_ring", value)
    assert nh.get_option("mixed_ring") == before


def test_survives_clean(nh):
    """carried across nhydro_clean to the next nhydro_init, as mixed_tail is, and independently of it"""
    for v in (1, 0):
        nh.set_option("mixed_ring", v)
        nh.set_option("mixed_tail", 1 - v)
        nh.nhydro_clean()
        assert (nh.get_option("mixed_ring"), nh.get_option("mixed_tail")) == (v, 1 - v)
    nh.set_option("mixed_tail", 0)


def test_counter_reads_zero_and_is_read_only(nh):
    from mgroms_amd._lib import MgxError
    assert nh.get_option("mixed_ring_passes") == 0
    with pytest.raises(MgxError, match="mixed_ring_passes"):
        nh.set_option("mixed_ring_passes", 1)
    assert nh.get_option("mixed_ring_passes") == 0


def test_header_documents_option_counter_and_entry():
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "mixed_ring" in set(re.findall(r'"([a-z_0-9]+)" \(default', hdr))   # the form tests/test_host_logic.py parses
    assert re.search(r'"mixed_ring" \(default 0,', hdr)
    assert '"mixed_ring_passes"' in hdr
    assert re.search(r"\bint mgx_mixed_ring_levels\(int nx, int ny, int nz, int \*mask\);", hdr)


# level sizes halve from level to level
RING_LEVELS = [
    ((512, 512, 64), 0b111),      # 64, 32, 16; level 4 has nz = 8
    ((512, 1024, 128), 0b1110),   # level 1 is tall; 64, 32, 16 on levels 2-4; level 5 has nz = 8
    ((512, 512, 48), 0b11),       # 48, 24; level 3 has nz = 12
    ((32, 32, 64), 0b1),          # 65536 cells; level 2 = 16x16x32 is small
    ((64, 64, 16), 0b1),          # 65536 cells
    ((32, 32, 16), 0),            # 16384 cells: small
    ((64, 32, 32), 0b1),          # 65536 cells
    ((32, 32, 32), 0),            # exactly 32768 cells, nz <= 32: small (the bound is inclusive)
    ((64, 64, 8), 0),             # nz = 8 has no instance
]


@pytest.mark.parametrize("dims,mask", RING_LEVELS, ids=["x".join(map(str, d)) for d, _ in RING_LEVELS])
def test_ring_levels(nh, dims, mask):
    assert nh.mixed_ring_levels(*dims) == mask
    # against the level table and the rule in words
    want = 0
    for lev, d in enumerate(nh.level_table(*dims), start=1):
        small = d["nx"] * d["ny"] * d["nz"] <= 32768 and d["nz"] <= 32
        if d["nz"] in (16, 20, 24, 32, 40, 48, 64) and not small:
            want |= 1 << (lev - 1)
    assert want == mask


def test_served_levels_are_never_tail_levels(nh):
    """what keeps mixed_tail = 0 and 1 the same bits under mixed_ring = 1: no level of the tail is served"""
    for dims, mask in RING_LEVELS:
        first = nh.mixed_tail_first(*dims)
        if first:
            assert mask >> (first - 1) == 0, (dims, mask, first)


def test_option_does_not_move_the_answer(nh):
    """the entry describes the hierarchy, whatever the option says at the moment"""
    for v in (0, 1):
        nh.set_option("mixed_ring", v)
        assert nh.mixed_ring_levels(512, 512, 64) == 0b111
    nh.set_option("mixed_ring", 0)


# (dims, planes of a colour) -> (served, look-ahead, planes per workgroup, non-temporal instance, workgroups, instance)
#   two planes per workgroup from 2048 waves of a colour on; the non-temporal instance above 256e6 / 36 B = 7.1 M cells
RING_CHOICE = [
    ((512, 512, 64), 256, (1, 3, 1, 1, 1024, 64)),    # level 1, four colours: 4 waves per half-row x 256 planes
    ((512, 512, 64), 512, (1, 3, 2, 1, 1024, 64)),    # red-black: 2048 waves, two planes per workgroup
    ((256, 256, 32), 128, (1, 3, 1, 0, 256, 32)),     # level 2: lives in the Infinity Cache
    ((256, 512, 16), 256, (1, 2, 1, 0, 1024, 16)),
    ((512, 512, 16), 512, (1, 2, 2, 0, 1024, 16)),
    ((512, 1024, 16), 512, (1, 2, 2, 1, 2048, 16)),
    ((32, 320, 16), 16, (1, 2, 1, 0, 48, 16)),        # a ragged third wave along the half-row
    ((64, 64, 24), 32, (1, 2, 1, 0, 32, 24)),
    ((32, 32, 32), 16, (0, 0, 4, 0, 4, 32)),          # small: k_relax32<32>, four planes per workgroup
    ((64, 64, 12), 32, (0, 0, 4, 0, 8, 0)),           # no instance of either kernel: the generic k_relax32
    ((16, 32, 128), 8, (0, 0, 4, 0, 2, 0)),           # tall
]


@pytest.mark.parametrize("dims,nplanes,want", RING_CHOICE, ids=[f"{'x'.join(map(str, d))}-{n}" for d, n, _ in RING_CHOICE])
def test_ring_choice(nh, dims, nplanes, want):
    c = nh.mixed_ring_choice(*dims, nplanes)
    assert tuple(c[k] for k in ("served", "depth", "planes_per_workgroup", "stream", "workgroups", "instance_nz")) == want, c


def test_bad_choice_arguments_refused(nh):
    from mgroms_amd._lib import MgxError
    for args in ((1, 16, 16, 1), (64, 64, 16, 0), (64, 64, 16, 65)):
        with pytest.raises(MgxError, match="mgx_mixed_ring_choice"):
            nh.mixed_ring_choice(*args)


def test_bad_sizes_refused(nh):
    from mgroms_amd._lib import MgxError
    with pytest.raises(MgxError, match="mgx_mixed_ring_levels"):
        nh.mixed_ring_levels(1, 16, 16)
