"""Option "mixed_direct" on the host (no GPU): the option and its counter are plain state, and whether the coarsest solve of an fp32 cycle is
served as one product (k_coarse_direct32, mgx_mixed.hip) is pure host logic (mgx_mixed_direct_cells over choose_mixed_direct_cells,
mgx_choice.h): the coarsest level of the one-rank hierarchy has nz = 2 or 4 (3 with option "small_any_nz"), even nx and ny, at most 2048
cells, and is not the only level."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nh():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    keep = nhydro.get_option("mixed_direct")
    yield nhydro
    nhydro.set_option("mixed_direct", keep)


def test_default(nh):
    """off until asked for: 0 is every launch and every bit of the sweeps"""
    assert nh.get_option("mixed_direct") == 0


def test_takes_0_and_1(nh):
    for v in (0, 1, 0, 1):
        nh.set_option("mixed_direct", v)
        assert nh.get_option("mixed_direct") == v


@pytest.mark.parametrize("value", [-1, 2, 32])
@pytest.mark.parametrize("before", [0, 1])
def test_other_values_refused(nh, value, before):
    from mgroms_amd._lib import MgxError
    nh.set_option("mixed_direct", before)
    with pytest.raises(MgxError, match="mixed_direct"):
        nh.set_option("mixed_direct", value)
    assert nh.get_option("mixed_direct") == before


def test_survives_clean(nh):
    """carried across nhydro_clean to the next nhydro_init, independently of mixed_tail and mixed_ring"""
    for v in (1, 0):
        nh.set_option("mixed_direct", v)
        nh.set_option("mixed_tail", 1 - v)
        nh.set_option("mixed_ring", 1 - v)
        nh.nhydro_clean()
        assert (nh.get_option("mixed_direct"), nh.get_option("mixed_tail"), nh.get_option("mixed_ring")) == (v, 1 - v, 1 - v)
    nh.set_option("mixed_tail", 0)
    nh.set_option("mixed_ring", 0)


def test_counter_reads_zero_and_is_read_only(nh):
    from mgroms_amd._lib import MgxError
    assert nh.get_option("mixed_direct_solves") == 0
    with pytest.raises(MgxError, match="mixed_direct_solves"):
        nh.set_option("mixed_direct_solves", 1)
    assert nh.get_option("mixed_direct_solves") == 0


def test_header_documents_option_counter_and_entry():
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "mixed_direct" in set(re.findall(r'"([a-z_0-9]+)" \(default', hdr))   # the form tests/test_host_logic.py parses
    assert re.search(r'"mixed_direct" \(default 0,', hdr)
    assert '"mixed_direct_solves"' in hdr
    assert re.search(r"\bint mgx_mixed_direct_cells\(int nx, int ny, int nz, int any_nz, int \*cells\);", hdr)


# (dims, small_any_nz) -> (the coarsest level, cells served)
DIRECT_CELLS = [
    ((512, 512, 64), 0, (16, 16, 2), 512),
    ((64, 64, 4), 0, (32, 32, 2), 2048),      # the bound is inclusive
    ((128, 64, 4), 0, (64, 32, 2), 0),        # 4096 cells
    ((16, 16, 16), 0, (4, 4, 4), 64),
    ((16, 16, 8), 0, (4, 4, 2), 32),
    ((24, 40, 4), 0, (12, 20, 2), 480),
    ((32, 32, 24), 0, (4, 4, 3), 0),          # nz = 3 has a kernel under small_any_nz only
    ((32, 32, 24), 1, (4, 4, 3), 48),
    ((512, 512, 64), 1, (16, 16, 2), 512),    # small_any_nz does not move an even nz
]


@pytest.mark.parametrize("dims,any_nz,coarsest,cells", DIRECT_CELLS, ids=[f"{'x'.join(map(str, d))}-any{a}" for d, a, _, _ in DIRECT_CELLS])
def test_direct_cells(nh, dims, any_nz, coarsest, cells):
    assert nh.mixed_direct_cells(*dims, small_any_nz=any_nz) == cells
    # against the level table and the rule in words
    t = nh.level_table(*dims)
    d = t[-1]
    assert (d["nx"], d["ny"], d["nz"]) == coarsest
    n = d["nx"] * d["ny"] * d["nz"]
    served = (d["nz"] in (2, 4) or (any_nz and d["nz"] == 3)) and d["nx"] % 2 == 0 and d["ny"] % 2 == 0 and n <= 2048 and len(t) >= 2
    assert (n if served else 0) == cells


def test_single_level_hierarchy_is_not_served(nh):
    """a coarsest level that is also the finest is never entered from a restriction"""
    one = [d for d in ((4, 4, 2), (8, 8, 2), (4, 4, 4), (16, 16, 2)) if len(nh.level_table(*d)) == 1]
    assert one, "no single-level size among the candidates"
    for d in one:
        assert d[0] * d[1] * d[2] <= 2048 and d[2] in (2, 4)   # the shape itself would be served
        assert nh.mixed_direct_cells(*d) == 0, d


def test_option_does_not_move_the_answer(nh):
    """the entry describes the hierarchy, whatever the option says at the moment"""
    for v in (0, 1):
        nh.set_option("mixed_direct", v)
        assert nh.mixed_direct_cells(512, 512, 64) == 512
        assert nh.mixed_direct_cells(128, 64, 4) == 0
    nh.set_option("mixed_direct", 0)


def test_bad_sizes_refused(nh):
    from mgroms_amd._lib import MgxError
    for args in ((1, 16, 16), (16, 16, 1), (16, 0, 16)):
        with pytest.raises(MgxError, match="mgx_mixed_direct_cells"):
            nh.mixed_direct_cells(*args)
