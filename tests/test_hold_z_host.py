"""Option "hold_z_levels" on the host (no GPU): the level table mgx_init will build (mgx_level_table_semi) against the rule of include/mgx.h
over a sweep of sizes, m = 0..4, both values of "hold_odd_nz" and process grids; m = 0 against mgx_level_table_hold; the hint for m
(mgx_hold_z_hint) on the seamount sizes of DESIGN.md 7.1.1; and the option's own surface (range, mgx_clean, the documented default)."""
import ctypes
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def nh():
    import __graft_entry__ as g
    g.build()
    from mgroms_amd import nhydro
    return nhydro


def rule_nz(nx, ny, nz, npx, npy, m, hold):
    """nz of every level: the first m coarsenings keep nz; then the reference's halving, min(nl1, m + nl2) levels in all (hold_odd_nz = 0),
    or the rule of hold_odd_nz -- an odd nz is handed on, and the hierarchy ends at nz = 2 or at the horizontal bound"""
    nl1 = 1 + int(math.floor(math.log(min(nx * npx, ny * npy) / 4.0) / math.log(2.0)))
    z = [nz]
    if not hold:
        nl2 = 1 + int(math.floor(math.log(nz / 2.0) / math.log(2.0)))
        for l in range(1, min(nl1, m + nl2)):
            z.append(z[-1] if l <= m else z[-1] // 2)
        return z
    for l in range(1, nl1):
        if l <= m:
            z.append(z[-1])
        elif z[-1] == 2:
            break
        else:
            z.append(z[-1] if z[-1] & 1 else z[-1] // 2)
    return z


SIZES = [(8, 8), (16, 16), (32, 32), (48, 80), (64, 64), (80, 48), (128, 128), (256, 128), (512, 512)]
NZS = [2, 4, 8, 12, 16, 20, 28, 32, 40, 64, 80]
GRIDS = [(1, 1), (2, 1), (2, 2), (4, 2)]


def test_table_against_the_rule(nh):
    """nz of every level is the rule's; nx, ny, the ranks, the gathers, keys, colours and neighbours are those of the reference's table --
    taken from a hierarchy of the same plane whose nz never runs out (they do not depend on nz) -- for every rank of every grid"""
    n = 0
    for nx, ny in SIZES:
        for npx, npy in GRIDS:
            deep = [nh.level_table(nx, ny, 1 << 20, npx, npy, r) for r in range(npx * npy)]
            for nz in NZS:
                for hold in (0, 1):
                    for m in range(5):
                        want = rule_nz(nx, ny, nz, npx, npy, m, hold)
                        for r in range(npx * npy):
                            t = nh.level_table(nx, ny, nz, npx, npy, r, hold_odd_nz=hold, hold_z_levels=m)
                            assert [l["nz"] for l in t] == want, (nx, ny, nz, npx, npy, r, hold, m)
                            for a, b in zip(t, deep[r]):
                                assert {k: v for k, v in a.items() if k != "nz"} == {k: v for k, v in b.items() if k != "nz"}, (nx, ny, nz, npx, npy, r, hold, m)
                            n += 1
    assert n > 10000


def test_examples_of_the_issue(nh):
    """128 x 128 x 16: m = 2 gives nz 16, 16, 16, 8, 4, 2 on 128, 64, 32, 16, 8, 4 columns; an m above nl1 - 1 holds every pair; the level
    count without hold_odd_nz is min(nl1, m + nl2)"""
    t = nh.level_table(128, 128, 16, hold_z_levels=2)
    assert [(l["nx"], l["ny"], l["nz"]) for l in t] == [(128, 128, 16), (64, 64, 16), (32, 32, 16), (16, 16, 8), (8, 8, 4), (4, 4, 2)]
    assert [l["nz"] for l in nh.level_table(128, 128, 16, hold_z_levels=8)] == [16] * 6
    assert [l["nz"] for l in nh.level_table(512, 512, 64, hold_z_levels=1)] == [64, 64, 32, 16, 8, 4, 2]
    assert [l["nz"] for l in nh.level_table(512, 512, 32, hold_z_levels=2)] == [32, 32, 32, 16, 8, 4, 2]
    assert [l["nz"] for l in nh.level_table(64, 64, 40, hold_odd_nz=1, hold_z_levels=1)] == [40, 40, 20, 10, 5]
    assert [l["nz"] for l in nh.level_table_periodic(32, 32, 16, periodic=3, hold_z_levels=1)] == [16, 16, 8, 4]


def test_m0_is_the_hold_table(nh):
    """hold_z = 0 equals mgx_level_table_hold, entry for entry, periodic included; values outside 0..8 are refused"""
    from mgroms_amd._lib import lib
    L = lib()
    a = (ctypes.c_int * (20 * 32))()
    b = (ctypes.c_int * (20 * 32))()
    for nx, ny in SIZES:
        for npx, npy in GRIDS:
            for nz in NZS:
                for hold in (0, 1):
                    for per in (0, 3):
                        for r in range(npx * npy):
                            na = L.mgx_level_table_semi(nx, ny, nz, npx, npy, r, 8, per, hold, 0, 32, a)
                            nb = L.mgx_level_table_hold(nx, ny, nz, npx, npy, r, 8, per, hold, 32, b)
                            assert na == nb > 0 and list(a[:20 * na]) == list(b[:20 * nb]), (nx, ny, nz, npx, npy, r, hold, per)
    assert L.mgx_level_table_semi(32, 32, 16, 1, 1, 0, 8, 0, 0, 9, 32, a) == -1
    assert L.mgx_level_table_semi(32, 32, 16, 1, 1, 0, 8, 0, 0, -1, 32, a) == -1


def test_hint_on_the_seamount(nh):
    """the smallest m with 2^m min(dx, dy) >= max(h) / nz: 1, 2, 1 on the three sizes of DESIGN.md 7.1.1; 1 and 2 at the bench plane with
    nz = 64 and 32 (dx = 19.5 m against dz = 62.5 m and 125 m); per rank of a 2 x 2 grid (the caller sets the maximum); 0 for flat cells;
    8 at the most; and the refusals"""
    from mgroms_amd._lib import MgxError
    from mgroms_amd.testcases import seamount_geometry

    def hint(nx, ny, nz, npx=1, npy=1, rank=0):
        dx, dy, _, h = seamount_geometry(nx, ny, npx, npy, rank)
        return nh.hold_z_hint(dx, dy, h, nz)
    assert [hint(64, 64, 16), hint(128, 128, 16), hint(128, 128, 32)] == [1, 2, 1]
    assert [hint(512, 512, 64), hint(512, 512, 32)] == [2, 3]
    assert max(hint(64, 64, 16, 2, 2, r) for r in range(4)) == 2      # the blocks of 128 x 128 x 16
    dx, dy, _, h = seamount_geometry(32, 32, 1, 1, 0)
    assert nh.hold_z_hint(dx, dy, h, 4096) == 0
    assert nh.hold_z_hint(dx * 1e-6, dy, h, 2) == 8
    # by hand, on a metric that varies: the halo is not read
    rng = np.random.default_rng(3)
    dx = rng.uniform(10.0, 20.0, (10, 14)); dy = rng.uniform(10.0, 20.0, (10, 14)); h = rng.uniform(100.0, 1000.0, (10, 14))
    dx[0] = dy[:, -1] = 1e-9; h[-1] = 1e9
    want = next(m for m in range(9) if m == 8 or 2.0 ** m * min(dx[1:-1, 1:-1].min(), dy[1:-1, 1:-1].min()) >= h[1:-1, 1:-1].max() / 8)
    assert nh.hold_z_hint(dx, dy, h, 8) == want
    with pytest.raises(MgxError, match="positive and finite"):
        nh.hold_z_hint(dx * 0.0, dy, h, 8)
    with pytest.raises(MgxError):
        nh.hold_z_hint(dx, dy[:-1], h, 8)


def test_option_surface(nh):
    """default 0; 0..8 accepted, anything else refused in words that name the option; the value survives mgx_clean; no environment variable"""
    from mgroms_amd._lib import MgxError
    assert nh.get_option("hold_z_levels") == 0 and nh.get_option("hold_z_fused") == 0
    try:
        for v in (8, 3, 1):
            nh.set_option("hold_z_levels", v)
            assert nh.get_option("hold_z_levels") == v
        nh.nhydro_clean()
        assert nh.get_option("hold_z_levels") == 1
        for v in (-1, 9):
            with pytest.raises(MgxError, match="hold_z_levels must be 0 .* or m = 1..8"):
                nh.set_option("hold_z_levels", v)
        with pytest.raises(MgxError, match="unknown option"):
            nh.set_option("hold_z_fused", 1)
        assert nh.get_option("hold_z_fuse") == 1
        with pytest.raises(MgxError, match="hold_z_fuse must be 1 .* or 0"):
            nh.set_option("hold_z_fuse", 2)
    finally:
        nh.set_option("hold_z_levels", 0)
