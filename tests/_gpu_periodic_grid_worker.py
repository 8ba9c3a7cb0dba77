"""One rank of a periodic multi-rank GPU solve (tests/test_gpu_periodic_grid.py).  All ranks share cuda:0 and talk over gloo with host
staging, as in tests/_gpu_rank_worker.py.

The yardstick is not the CPU oracle (closed walls only) but the ONE-RANK periodic solve, which tests/test_gpu_periodic.py pins: four
colours do not depend on the decomposition, so every rank's arrays are, bit for bit, its block of the one-rank arrays.  Each worker
first solves the GLOBAL problem on one rank with the option on, then cleans and initialises its rank of the grid; every input is cut
from one global array.  "Expected" is the rank's block cut from the one-rank array with its halo: interior of that array across a rank
seam, the array's own halo on a side of the domain -- the wrap image in a periodic direction, the closed rule in a closed one -- so every
corner rule is part of the comparison.  Three kinds of halo cell have no one-rank counterpart and are left out, each where it is compared
(expected(), the cA branch): the two-column corner of zr between a closed side and a rank seam inside the domain, the halo of cA on a rank
seam without bmask (nothing exchanges it), and the halo of cA's diagonal slot (formed after the exchange, on the interior only).

usage: _gpu_periodic_grid_worker.py rank world npx npy port nx ny nz nsmall periodic method [opt+opt...]
  hooks     the solve again through the exchange hooks (comm.set_p2p(False)): the same bits
  count     a level-1 fill_halo("p") through the pushes: exactly one launch, no hook exchange
  refuse    the fp32 cycles and a change of the option under the live grid are refused
  uvw       nhydro_solve on random global u, v, w: b, p, u, v, w bit for bit; the face on the wrap seam equal on both of its ranks
  bmask     an island across a rank seam and the wrap seam: rmask, cA (halos included: the 4-D exchange) and p
  rbseq     (method RB) three sweeps of the sequential order at speed against "rb_exact" on the same grid, every level
  gs        (method GS) solved to 1e-11 on the grid against the one-rank four-colour solution, in units of d0 = one-rank GS against it
  shift     no yardstick: every global input rolled by one block in i moves every rank's outputs to its eastern neighbour, bit for bit;
            and the operator identity through the model calls per rank, on the whole block (no exclusion ring on a periodic side)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ranks import gloo_rank

TOL_HIST = 1e-12   # p is bit-identical: only the order of the norm's reduction differs (the bound of tests/_gpu_rank_worker.py)


def island_on_seams(NX, NY, per):
    """interior (NX, NY) mask: one island centred on the crossing of the wrap seams (a closed direction: at 0.25 of its length), one on the
    crossing of the rank seams of a 2 x 2 grid"""
    i = np.arange(NX)[:, None] + 0.5
    j = np.arange(NY)[None, :] + 0.5
    r2 = (0.15 * min(NX, NY)) ** 2
    land = np.zeros((NX, NY), dtype=bool)
    for ci, cj in ((0.0 if per & 1 else 0.25 * NX, 0.0 if per & 2 else 0.25 * NY), (0.5 * NX, 0.5 * NY)):
        di = np.abs(i - ci); dj = np.abs(j - cj)
        if per & 1:
            di = np.minimum(di, NX - di)
        if per & 2:
            dj = np.minimum(dj, NY - dj)
        land |= di ** 2 + dj ** 2 <= r2
    return np.where(land, 0.0, 1.0)


def land_on_both_sides(mask, NX, NY):
    """land columns on each side of the wrap seam and of the rank seam of a 2 x 2 grid, in i and in j: within a quarter of the domain"""
    land = mask == 0.0
    qi, qj = NX // 4, NY // 4
    return [int(land[:qi].sum()), int(land[NX - qi:].sum()), int(land[NX // 2 - qi:NX // 2].sum()), int(land[NX // 2:NX // 2 + qi].sum()),
            int(land[:, :qj].sum()), int(land[:, NY - qj:].sum()), int(land[:, NY // 2 - qj:NY // 2].sum()), int(land[:, NY // 2:NY // 2 + qj].sum())]


def main():
    rank, world, npx, npy, port, nx, ny, nz, nsmall, per = (int(a) for a in sys.argv[1:11])
    method = sys.argv[11]
    opts = set(sys.argv[12].split("+")) if len(sys.argv) > 12 and sys.argv[12] else set()
    with gloo_rank(rank, world, port):
        rank_main(rank, world, npx, npy, nx, ny, nz, nsmall, per, method, opts)
    print(f"rank {rank} ok")


def rank_main(rank, world, npx, npy, nx, ny, nz, nsmall, per, method, opts):
    bmask = "bmask" in opts
    import torch
    import torch.distributed as dist
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd._lib import MgxError
    from mgroms_amd.parallel import Comm
    from test_gpu_periodic import full2d, geometry, velocities_from, velocity_bases
    from _operator_identity import COUPLING_TOL, scaled_defect

    nhydro.set_verbose(0)
    NX, NY = npx * nx, npy * ny
    pi, pj = rank % npx, rank // npx
    qi, qj = pi * nx, pj * ny
    model = "uvw" in opts or "shift" in opts
    maxit = 2 if "shift" in opts else 3
    tol = 1e-11 if "gs" in opts else 1e-30
    par = nhydro.default_params(relax_method=method, solver_prec=tol, nsmall=nsmall, ns_coarsest=6, bmask=1 if bmask else 0,
                                **(dict(solver_maxiter=maxit) if model else {}))

    g = geometry(NX, NY, per)
    if bmask:
        g["rmask"] = island_on_seams(NX, NY, per)
        counts = land_on_both_sides(g["rmask"], NX, NY)
        assert min(counts) >= 8, ("the island does not lie across every seam: land columns per side", counts)
    bases = velocity_bases(NX, NY, nz, per, 5)

    def cut2d(a, poison=True):
        """this rank's (nx+2, ny+2) piece of a global (NX+2, NY+2) array; the halo ON a periodic side of the domain is the library's to fill"""
        a = a[qi:qi + nx + 2, qj:qj + ny + 2].copy()
        if poison and per & 1:
            if pi == 0:
                a[0, :] = np.nan
            if pi == npx - 1:
                a[-1, :] = np.nan
        if poison and per & 2:
            if pj == 0:
                a[:, 0] = np.nan
            if pj == npy - 1:
                a[:, -1] = np.nan
        return a

    def cut_uvw(u, v, w):
        return (u[:, qj:qj + ny + 2, qi:qi + nx + 1].copy(), v[:, qj:qj + ny + 1, qi:qi + nx + 2].copy(), w[:, qj:qj + ny + 2, qi:qi + nx + 2].copy())

    def set_matrices(geo, local):
        f = full2d(geo, per)
        a = {n: (None if f[n] is None else (cut2d(f[n]) if local else f[n])) for n in ("dx", "dy", "zeta", "h", "rmask")}
        mg.nhydro_matrices(a["dx"], a["dy"], a["zeta"], a["h"], a["rmask"], geo["hc"], geo["theta_b"], geo["theta_s"])

    # ---- the yardstick: the global problem on one rank ------------------------------------------------------------------------------
    ref = {}
    if "shift" not in opts and "rbseq" not in opts:
        def one_rank(meth):
            mg.nhydro_clean()
            nhydro.set_option("periodic", per)
            mg.nhydro_init(NX, NY, nz, 1, 1, 0, nhydro.default_params(relax_method=meth, solver_prec=tol, nsmall=nsmall, ns_coarsest=6, bmask=1 if bmask else 0,
                                                                      **(dict(solver_maxiter=maxit) if model else {})))
            set_matrices(g, False)
            out = {"nlevs": mg.nlevs()}
            table = nhydro.level_table_periodic(NX, NY, nz, 1, 1, 0, nsmall, per)
            for lev in range(1, mg.nlevs() + 1):
                gl = mg.grid(lev)
                assert gl.neighb == table[lev - 1]["neighb"], (lev, gl.neighb)     # the one-rank table is what mgx_level_info reports
                out[lev] = {name: gl.get(name) for name in ("h", "zr", "cA")}
            out["rmask"] = mg.grid(1).get("rmask")
            U, V, W = velocities_from(bases, per)
            nhydro.compute_rhs(U, V, W)
            out["b"] = mg.grid(1).b
            out["n"], out["hist"] = mg.solve_p(tol, 200 if "gs" in opts else 3)
            out["p"] = mg.grid(1).p
            if "uvw" in opts:
                mg.nhydro_solve(U, V, W)
                out["b2"], out["p2"], out["uvw"] = mg.grid(1).b, mg.grid(1).p, (U, V, W)
            return out
        ref = one_rank("FC")
        if "gs" in opts:
            gs1 = one_rank("GS")
            pmax = np.abs(ref["p"][1:-1, 1:-1]).max()
            d0 = np.abs(gs1["p"][1:-1, 1:-1] - ref["p"][1:-1, 1:-1]).max() / pmax
            assert ref["hist"][-1] <= tol and gs1["hist"][-1] <= tol and d0 > 0, (ref["hist"][-1], gs1["hist"][-1], d0)
        mg.nhydro_clean()

    # ---- this rank of the grid -----------------------------------------------------------------------------------------------------------
    nhydro.set_option("periodic", per)
    if method == "RB":
        nhydro.set_option("rb_seq", 1); nhydro.set_option("rb_exact", 0)
    comm = Comm(device="cuda", p2p=True)
    mg.nhydro_init(nx, ny, nz, npx, npy, rank, par, comm=comm)
    assert comm.p2p_active, comm.p2p_error
    assert "periodic" in comm.transport() and "peer-to-peer" in comm.transport(), comm.transport()
    set_matrices(g, True)
    table = nhydro.level_table_periodic(nx, ny, nz, npx, npy, rank, nsmall, per)
    assert mg.nlevs() == len(table)
    for lev in range(1, mg.nlevs() + 1):
        assert mg.grid(lev).neighb == table[lev - 1]["neighb"], (rank, lev)

    def block(lev):
        """(i0, j0, NXl, NYl): where this rank's block of the level lies in the one-rank level, from mgx_level_info"""
        gl = mg.grid(lev)
        bi = pi // gl.incx if gl.npx > 1 else 0
        bj = pj // gl.incy if gl.npy > 1 else 0
        return bi * gl.nx, bj * gl.ny, gl.nx * gl.npx, gl.ny * gl.npy

    def expected(A, lev, h, wrap=True):
        """the block with h halo columns cut from the one-rank array A (halo h).  The block lies inside the domain, so its halo is either interior
        of the one-rank array (a rank seam) or the one-rank array's own halo (a side of the domain: the wrap image in a periodic direction,
        the closed rule in a closed one, and the one-rank corner rule where two of them meet).  Second value: where the entry is compared.
          h = 2 (zr): a corner between a CLOSED side of the domain and a rank seam inside it is left out -- there the reference's mixed-corner
            rule mirrors the received columns while the one-rank array extrapolates its own, on closed grids as well (mg_mpi_exchange.f90:1216-1240
            against :956-964); across the wrap seam both are the mirror of the wrapped columns and are compared.
          wrap = False: a halo entry counts only beyond the edge of the domain (see cA below)."""
        gl = mg.grid(lev)
        i0, j0, NXl, NYl = block(lev)
        assert A.shape[0] == NXl + 2 * h and A.shape[1] == NYl + 2 * h, (lev, A.shape, NXl, NYl)
        ii, jj = np.arange(i0 - h, i0 + gl.nx + h), np.arange(j0 - h, j0 + gl.ny + h)
        ini, inj = (ii >= i0) & (ii < i0 + gl.nx), (jj >= j0) & (jj < j0 + gl.ny)
        outi, outj = (ii < 0) | (ii >= NXl), (jj < 0) | (jj >= NYl)
        if not wrap:
            # (next to a rank seam inside the domain the halo cell beyond a closed side reads the mixed corner of zr / zw described above)
            fari = ini & ~((ii == i0) & (i0 > 0)) & ~((ii == i0 + gl.nx - 1) & (i0 + gl.nx < NXl))
            farj = inj & ~((jj == j0) & (j0 > 0)) & ~((jj == j0 + gl.ny - 1) & (j0 + gl.ny < NYl))
            ok = (ini[:, None] & inj[None, :]) | (outi[:, None] & farj[None, :]) | (fari[:, None] & outj[None, :]) | (outi[:, None] & outj[None, :])
        else:
            ok = np.full((ii.size, jj.size), True)
            if h == 2:
                seam_i, seam_j = ~ini & ~outi, ~inj & ~outj
                closed_i = outi if not per & 1 else np.zeros_like(outi)
                closed_j = outj if not per & 2 else np.zeros_like(outj)
                ok &= ~(seam_i[:, None] & closed_j[None, :]) & ~(closed_i[:, None] & seam_j[None, :])
        return A[i0:i0 + gl.nx + 2 * h, j0:j0 + gl.ny + 2 * h], ok

    def same(got, A, lev, h, what, wrap=True):
        want, ok = expected(A, lev, h, wrap)
        assert got.shape == want.shape, (rank, lev, what, got.shape, want.shape)
        bad = (got != want) & ok.reshape(ok.shape + (1,) * (got.ndim - 2))
        assert not bad.any(), (rank, lev, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())

    if ref:
        assert mg.nlevs() == ref["nlevs"]
        for lev in range(1, mg.nlevs() + 1):
            gl = mg.grid(lev)
            same(gl.get("h"), ref[lev]["h"], lev, 1, "h")
            same(gl.get("zr"), ref[lev]["zr"], lev, 2, "zr")
            cA = gl.get("cA")
            if bmask:
                # fill_halo_4D exchanged the halo: the neighbour's interior, across the wrap too -- of the seven off-diagonal slots.  The diagonal is
                # formed AFTER that exchange, on the interior only, here as in the reference (mg_define_matrix.f90:612 before :620-650): its halo
                # holds what the exchange found in the neighbour's scratch, never a coefficient, and nothing reads it
                same(cA[..., 1:], ref[lev]["cA"][..., 1:], lev, 1, "cA slots 2-8")
                same(cA[1:-1, 1:-1], ref[lev]["cA"][1:-1, 1:-1], lev, 0, "cA interior")
            else:
                # without bmask nothing exchanges cA (mg_define_matrix.f90:611 is under bmask): its halo holds what the set-up kernel leaves in a halo
                # cell, which is the one-rank array's OWN halo on every side of the domain, periodic ones included, and compared there; a halo
                # cell on a rank seam inside the domain has no one-rank counterpart (there it would be an interior cell with a full stencil)
                same(cA, ref[lev]["cA"], lev, 1, "cA", wrap=False)
                same(cA[1:-1, 1:-1], ref[lev]["cA"][1:-1, 1:-1], lev, 0, "cA interior")
        if bmask:
            same(mg.grid(1).get("rmask"), ref["rmask"], 1, 1, "rmask")

    U, V, W = velocities_from(bases, per)
    u, v, w = cut_uvw(U, V, W)
    c0 = nhydro.counters()

    if ref:
        nhydro.compute_rhs(u, v, w)
        same(mg.grid(1).b[1:-1, 1:-1], ref["b"][1:-1, 1:-1], 1, 0, "b")
        n, hist = mg.solve_p(tol, 200 if "gs" in opts else 3)
        p = mg.grid(1).p
        c = nhydro.counters()
        assert c["p2p_exchanges"] > c0["p2p_exchanges"] and c["exchanges"] > 0 and c["allreduces"] > 0
        if "gs" in opts:
            want, _ = expected(ref["p"], 1, 1)
            d = np.abs(p[1:-1, 1:-1] - want[1:-1, 1:-1]).max() / pmax
            print(f"rank {rank} GS on the grid: {n} iterations, {d:.3e} from the one-rank FC solution; d0 (one-rank GS against it, {gs1['n']} iterations) = {d0:.3e}")
            assert hist[-1] <= tol, hist
            assert d <= 16 * d0, (d, d0)
        else:
            assert n == ref["n"] == 3, (n, ref["n"])
            same(p, ref["p"], 1, 1, "p")
            assert np.all(np.abs(hist - ref["hist"]) <= TOL_HIST * np.abs(ref["hist"])), (hist, ref["hist"])
        if "hooks" in opts:
            comm.set_p2p(False)
            n2, hist2 = mg.solve_p(tol, 3)
            c2 = nhydro.counters()
            assert n2 == n and np.array_equal(hist2, hist) and np.array_equal(mg.grid(1).p, p), rank
            assert c2["p2p_exchanges"] == c["p2p_exchanges"] and c2["exchanges"] > c["exchanges"]
            comm.set_p2p(True)
        if "count" in opts:
            g1 = mg.grid(1)
            g1.set("p", np.random.default_rng(3 + rank).standard_normal(g1._shape("p")))
            a = nhydro.counters()
            mg.fill_halo(1, "p")
            b = nhydro.counters()
            assert (b["launches"] - a["launches"], b["exchanges"] - a["exchanges"], b["p2p_exchanges"] - a["p2p_exchanges"], b["halo_fills"] - a["halo_fills"]) == (1, 0, 1, 1), (a, b)
            filled = g1.get("p")
            comm.set_p2p(False)             # the same fill through the hooks: the same halo, the closed side's image and its corners included
            g1.set("p", np.random.default_rng(3 + rank).standard_normal(g1._shape("p")))
            mg.fill_halo(1, "p")
            assert np.array_equal(g1.get("p"), filled), rank
            comm.set_p2p(True)
        if "uvw" in opts:
            mg.nhydro_solve(u, v, w)
            same(mg.grid(1).b[1:-1, 1:-1], ref["b2"][1:-1, 1:-1], 1, 0, "b of nhydro_solve")
            same(mg.grid(1).p, ref["p2"], 1, 1, "p of nhydro_solve")
            U1, V1, W1 = cut_uvw(*ref["uvw"])
            assert not np.array_equal(u, cut_uvw(U, V, W)[0])
            assert np.array_equal(u[:, 1:-1, :], U1[:, 1:-1, :]) and np.array_equal(v[:, :, 1:-1], V1[:, :, 1:-1]) and np.array_equal(w[:, 1:-1, 1:-1], W1[:, 1:-1, 1:-1]), rank
            if per & 1 and npx > 1:   # the face on the wrap seam is held by the last and by the first rank of the row
                mine = torch.from_numpy(np.ascontiguousarray(u[:, 1:-1, nx] if pi == npx - 1 else u[:, 1:-1, 0]))
                faces = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(faces, mine)
                if pi == npx - 1:
                    assert torch.equal(mine, faces[pj * npx]), rank
        if "refuse" in opts:
            for name in ("cycle_precision", "krylov_precision"):
                if name == "krylov_precision":
                    nhydro.set_option("krylov", 2)
                nhydro.set_option(name, 32)
                try:
                    mg.solve_p(1e-8, 5)
                    raise AssertionError(f"{name} = 32 was served on a periodic grid")
                except MgxError as e:
                    assert f'"periodic" = {per} is not served by the fp32 cycles (cycle_precision = 32, krylov_precision = 32)' in str(e), str(e)
                nhydro.set_option(name, 64); nhydro.set_option("krylov", 0)
            for value in {0, 1, 2, 3} - {per}:
                try:
                    nhydro.set_option("periodic", value)
                    raise AssertionError("the option changed under a live grid")
                except MgxError as e:
                    assert f"periodic = {value}: the hierarchy in use was built with periodic = {per}" in str(e), str(e)
            n3, hist3 = mg.solve_p(tol, 3)   # and the grid is usable afterwards
            assert np.array_equal(hist3, hist) and np.array_equal(mg.grid(1).p, p)

    if "rbseq" in opts:
        start = {}
        for lev in range(1, mg.nlevs() + 1):   # one global state per level, cut per block: the members of a gather group hold the same block
            gl = mg.grid(lev)
            i0, j0, NXl, NYl = block(lev)
            rng = np.random.default_rng(31 + lev)
            P, B = rng.standard_normal((NXl + 2, NYl + 2, gl.nz)), rng.standard_normal((NXl + 2, NYl + 2, gl.nz))
            start[lev] = (P[i0:i0 + gl.nx + 2, j0:j0 + gl.ny + 2].copy(), B[i0:i0 + gl.nx + 2, j0:j0 + gl.ny + 2].copy())

        def run():
            out = {}
            for lev, (p0, b0) in start.items():
                gl = mg.grid(lev)
                gl.set("p", p0); gl.set("b", b0); mg.fill_halo(lev, "p")
                mg.relax(lev, 3)
                out[lev] = gl.get("p")
            return out
        seq = run()
        nhydro.set_option("rb_exact", 1)
        exact = run()
        nhydro.set_option("rb_exact", 0)
        for lev in start:
            d = np.abs(seq[lev] - exact[lev]).max() / np.abs(exact[lev]).max()
            print(f"rank {rank} level {lev}: sequential order at speed against the plane loop {d:.3e}")
            assert not np.array_equal(exact[lev], start[lev][0])
            assert d <= 1e-12, (rank, lev, d)

    if "shift" in opts:
        assert per == 3 and npx == 2 and method == "FC"

        def outputs(geo, bas):
            set_matrices(geo, True)
            uu, vv, ww = cut_uvw(*velocities_from(bas, per))
            mg.nhydro_solve(uu, vv, ww)
            return [mg.grid(1).p, uu, vv, ww]
        first = outputs(g, bases)
        g2 = dict(g)
        for name in ("dx", "dy", "zeta", "h"):
            g2[name] = np.roll(g[name], nx, axis=0)
        moved = outputs(g2, tuple(np.roll(a, nx, axis=2) for a in bases))
        west = pj * npx + (pi - 1) % npx
        for a, b in zip(first, moved):   # what my western neighbour held before the roll is what I hold after it
            mine = torch.from_numpy(np.ascontiguousarray(a))
            parts = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            assert np.array_equal(parts[west].numpy(), b) and not np.array_equal(a, b), rank
        # the operator identity through the model calls (tests/_operator_identity.py: coupling_defect's sequence), on the whole block
        set_matrices(g, True)
        sel = np.ones((nx, ny), dtype=bool)
        u0, v0, w0 = cut_uvw(*velocities_from(velocity_bases(NX, NY, nz, per, 1), per))
        uu, vv, ww = u0.copy(), v0.copy(), w0.copy()
        mg.nhydro_solve(uu, vv, ww)
        assert not np.array_equal(uu, u0) and not np.array_equal(ww, w0)
        nhydro.compute_rhs(u0, v0, w0)
        b = mg.grid(1).b[1:-1, 1:-1]
        mg.compute_residual(1)
        r = mg.grid(1).r[1:-1, 1:-1]
        # (u', v', w' of this rank alone: the halo columns a model would refresh by its own exchange are taken from the neighbours' results)
        got = []
        for a in (uu, vv, ww):
            mine = torch.from_numpy(np.ascontiguousarray(a))
            parts = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            got.append([t.numpy() for t in parts])
        UU = np.zeros((nz, NY + 2, NX + 1)); VV = np.zeros((nz, NY + 1, NX + 2)); WW = np.zeros((nz + 1, NY + 2, NX + 2))
        for r_ in range(world):
            ri, rj = (r_ % npx) * nx, (r_ // npx) * ny
            UU[:, rj + 1:rj + ny + 1, ri:ri + nx + 1] = got[0][r_][:, 1:-1, :]
            VV[:, rj:rj + ny + 1, ri + 1:ri + nx + 1] = got[1][r_][:, :, 1:-1]
            WW[:, rj + 1:rj + ny + 1, ri + 1:ri + nx + 1] = got[2][r_][:, 1:-1, 1:-1]
        UU[:, 0, :] = UU[:, NY, :]; UU[:, NY + 1, :] = UU[:, 1, :]
        VV[:, :, 0] = VV[:, :, NX]; VV[:, :, NX + 1] = VV[:, :, 1]
        WW[:, 0, :] = WW[:, NY, :]; WW[:, NY + 1, :] = WW[:, 1, :]; WW[:, :, 0] = WW[:, :, NX]; WW[:, :, NX + 1] = WW[:, :, 1]
        nhydro.compute_rhs(*cut_uvw(UU, VV, WW))
        b2 = mg.grid(1).b[1:-1, 1:-1]
        Ap = b - r
        assert np.abs(Ap).max() > 1e-3 * np.abs(b).max()
        defect = scaled_defect(b2, r, sel, b, Ap)
        print(f"rank {rank} operator identity through the model calls: {defect:.3e}")
        assert defect <= COUPLING_TOL, (rank, defect)

    mg.nhydro_clean()
    nhydro.set_option("periodic", 0)


if __name__ == "__main__":
    main()
