"""Option "periodic" on a process grid, the host logic (no GPU): the neighbour tables of every rank (mgx_level_table_periodic) and the
entry list of an exchange (mgx_exchange_plan).

With the wrap one rank is the neighbour on several sides at once (two ranks along a periodic direction: east and west; one rank along it:
S, SW and SE; a doubly periodic 2 x 2 grid: all four corners), and every transport behind mgx_set_comm matches the messages of one pair of
ranks in list order.  The plan is replayed here with exactly that matching, for every level and every pair of ranks: what was packed for
direction d has to land in the slot opp(d) of neighb[d]."""
import itertools

import pytest

from mgroms_amd import nhydro

OPP = [2, 3, 0, 1, 6, 7, 4, 5]          # S E N W SW SE NE NW
DI = [0, 1, 0, -1, -1, 1, 1, -1]
DJ = [-1, 0, 1, 0, -1, -1, 1, 1]
KIND = [0, 1, 0, 1, 2, 2, 2, 2]          # S/N edge, E/W edge, corner
GRIDS = [(2, 1), (1, 2), (2, 2), (4, 1), (1, 4), (4, 2), (2, 4)]
BLOCK = (32, 32, 16)
CASES = list(itertools.product(GRIDS, (1, 2, 3), (8, 16, 32)))
IDS = ["%dx%d-per%d-nsmall%d" % (g[0], g[1], p, n) for g, p, n in CASES]


def tables(grid, per, nsmall):
    npx, npy = grid
    return [nhydro.level_table_periodic(*BLOCK, npx, npy, r, nsmall, per) for r in range(npx * npy)]


@pytest.mark.parametrize("grid,per,nsmall", CASES, ids=IDS)
def test_tables_are_symmetric_and_absent_only_at_closed_edges(grid, per, nsmall):
    npx, npy = grid
    T = tables(grid, per, nsmall)
    gathered = False
    for lev in range(len(T[0])):
        for a in range(npx * npy):
            L = T[a][lev]
            pi, pj = a % npx, a // npx
            gathered |= bool(L["gather"])
            for d in range(8):
                b = L["neighb"][d]
                # absent exactly where a step of the level leaves the grid in a closed direction
                ti, tj = pi + DI[d] * L["incx"], pj + DJ[d] * L["incy"]
                out_i, out_j = not 0 <= ti < npx, not 0 <= tj < npy
                absent = (out_i and not per & 1) or (out_j and not per & 2)
                assert (b < 0) == absent, (lev, a, d, b)
                if b < 0:
                    continue
                assert b == (tj % npy) * npx + ti % npx, (lev, a, d, b)
                assert T[b][lev]["neighb"][OPP[d]] == a, (lev, a, d, b)          # symmetry
                if L["npx"] == 1 and DJ[d] == 0:
                    assert b == a, (lev, a, d)                                   # one rank along i: the rank itself
                if L["npy"] == 1 and DI[d] == 0:
                    assert b == a, (lev, a, d)
    assert gathered or nsmall == 8   # the combinations reach gathered levels


@pytest.mark.parametrize("grid,nsmall", list(itertools.product(GRIDS, (8, 16, 32))))
def test_periodic_zero_is_the_closed_table(grid, nsmall):
    npx, npy = grid
    for r in range(npx * npy):
        assert nhydro.level_table_periodic(*BLOCK, npx, npy, r, nsmall, 0) == nhydro.level_table(*BLOCK, npx, npy, r, nsmall)


@pytest.mark.parametrize("per", [0, 1, 2, 3])
def test_one_rank_table_is_the_one_rank_rule(per):
    """what mgx_level_info reports on one rank since the option exists: the rank itself on the periodic sides, at a corner where both of its
    sides are periodic, nothing elsewhere (the GPU suite compares the two on a live hierarchy)"""
    closed = nhydro.level_table(*BLOCK)
    T = nhydro.level_table_periodic(*BLOCK, 1, 1, 0, 8, per)
    assert len(T) == len(closed)
    for L, C in zip(T, closed):
        want = [0 if per & 2 else -1, 0 if per & 1 else -1] * 2 + [0 if per == 3 else -1] * 4
        assert L["neighb"] == want
        assert {k: v for k, v in L.items() if k != "neighb"} == {k: v for k, v in C.items() if k != "neighb"}


def test_invalid_arguments_are_refused():
    with pytest.raises(nhydro.MgxError):
        nhydro.level_table_periodic(*BLOCK, 2, 1, 0, 8, 4)
    with pytest.raises(nhydro.MgxError):
        nhydro.exchange_plan([1, -1, -1, -1, -1, -1, -1, -1], 1)   # a wrap (the rank itself to the south) without its northern end


def replay(lists, neighb):
    """in-order matching per pair of ranks: lists[a] = [(peer, send direction, receive direction)].  Returns the deliveries
    [(a, d, b, slot)]: what a packed for direction d arrived in b's halo of direction `slot`."""
    n = len(lists)
    got = []
    for a in range(n):
        for b in range(n):
            sends = [sd for peer, sd, _ in lists[a] if peer == b]
            slots = [rd for peer, _, rd in lists[b] if peer == a]
            assert len(sends) == len(slots), (a, b, sends, slots)
            got += [(a, d, b, s) for d, s in zip(sends, slots)]
    return got


@pytest.mark.parametrize("grid,per,nsmall", CASES, ids=IDS)
def test_plan_delivers_every_edge_to_the_opposite_slot(grid, per, nsmall):
    npx, npy = grid
    T = tables(grid, per, nsmall)
    for lev in range(len(T[0])):
        nb = [T[r][lev]["neighb"] for r in range(npx * npy)]
        lists = []
        for r in range(npx * npy):
            entries, self_dirs = nhydro.exchange_plan(nb[r], r)
            assert self_dirs == [d for d in range(8) if nb[r][d] == r], (lev, r)
            assert all(peer != r and peer >= 0 for peer, _, _ in entries), (lev, r, entries)        # no self peer in the hook list
            assert all(KIND[sd] == KIND[rd] for _, sd, rd in entries), (lev, r, entries)             # one count per entry
            assert all(nb[r][sd] == peer and nb[r][rd] == peer for peer, sd, rd in entries), (lev, r, entries)
            assert sorted(sd for _, sd, _ in entries) == sorted(rd for _, _, rd in entries) == [d for d in range(8) if nb[r][d] >= 0 and nb[r][d] != r]
            for peer in {p for p, _, _ in entries}:
                sd = [s for p, s, _ in entries if p == peer]
                assert sd == sorted(sd), (lev, r, entries)                                           # sends to one peer in ascending direction
            lists.append(entries)
        deliveries = replay(lists, nb)
        assert len(deliveries) == sum(len(l) for l in lists)
        for a, d, b, slot in deliveries:
            assert nb[a][d] == b and slot == OPP[d] and nb[b][slot] == a, (lev, a, d, b, slot)


def test_plain_direction_order_misdelivers_on_two_ranks():
    """why the plan exists: 2 x 1 ranks, periodic = 1, both sides listing their entries in direction order -- the counts are equal, and
    rank 0's eastern edge arrives in rank 1's EASTERN halo"""
    T = tables((2, 1), 1, 8)
    nb = [T[r][0]["neighb"] for r in range(2)]
    assert nb[0][1] == nb[0][3] == 1 and nb[1][1] == nb[1][3] == 0
    plain = [[(nb[r][d], d, d) for d in range(8) if nb[r][d] >= 0 and nb[r][d] != r] for r in range(2)]
    wrong = [(a, d, b, s) for a, d, b, s in replay(plain, nb) if s != OPP[d]]
    assert (0, 1, 1, 1) in wrong and len(wrong) == 4
    plan = [nhydro.exchange_plan(nb[r], r)[0] for r in range(2)]
    assert plan[0] == [(1, 1, 3), (1, 3, 1)]
    assert all(s == OPP[d] for _, d, _, s in replay(plan, nb))
