"""One rank of a multi-rank GPU solve (tests/test_gpu_multirank.py).  All ranks share cuda:0 of the one-GPU box and
talk over gloo with host staging (RCCL refuses several ranks on one device); everything else -- kernels, packs,
neighbour tables, gather/split, callbacks -- is the code path the 8-GPU runs use."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _ranks import gloo_rank   # (tests/ is the script's directory: already on sys.path)


def main():
    rank, world, npx, npy, port, nx, ny, nz, nsmall = (int(a) for a in sys.argv[1:10])
    method = sys.argv[10]
    opts = set(sys.argv[11].split("+")) if len(sys.argv) > 11 and sys.argv[11] else set()
    import time
    T0 = time.time()
    stamps = []

    def stamp(what):
        stamps.append(f"{what}={time.time() - T0:.1f}s")
    with gloo_rank(rank, world, port):
        stamp("rendezvous")
        line = rank_main(rank, npx, npy, nx, ny, nz, nsmall, method, opts, stamp)
    stamp("teardown")
    print(f"rank {rank} ok {line} " + " ".join(stamps))


def rank_main(rank, npx, npy, nx, ny, nz, nsmall, method, opts, stamp):
    bmask = "bmask" in opts
    p2p = "nop2p" not in opts
    exact = "exact" in opts        # relax_method='RB' in the reference's sequential order, one launch per plane (mgx_set_option("rb_exact")): bitwise
    par = "par" in opts            # relax_method='RB' as the plain parallel sweep (rb_seq = 0); default: the sequential order at speed (rb_seq = 1)
    golden = "golden" in opts      # namelist defaults, compared with the reference's recorded 2x2 history (tests/golden)
    rndtopo = "rndtopo" in opts    # mg_testrndtopo's geometry (BASELINE config 4) instead of the seamount
    fuse0 = "fuse0" in opts        # red-black, sequential order: the correction inside the walk's launch on every level that has an instance (rbseq_fuse_min = 0), open sides included
    connectfail = "connectfail" in opts  # rank 1 cannot open its neighbours' buffers (test hook): everybody must end up on the hooks, and every norm's all-reduce must carry the same count on all ranks
    uvw = "uvw" in opts            # random u, v, w: one global field cut per rank, so the copies of a shared face agree
    uvw_indep = "uvw_indep" in opts  # random u, v, w drawn per rank: the copies of a shared face disagree, and the reference takes the neighbour's flux there
    overlap0 = "overlap0" in opts  # the shipped default overlap = 0 (nhydro_solve as a model calls it) instead of the exchange beside the interior sweep
    curv = "curv" in opts          # dx, dy times this rank's block of the global curvilinear metric (testcases.curvilinear_metric): dx(i,j), dy(i,j)
    model = uvw or uvw_indep       # ... and nhydro_solve on both sides afterwards: u, v, w per rank, bit for bit
    assert not model or method == "FC" or exact
    if connectfail:
        os.environ["MGX_P2P_TEST_FAIL_CONNECT"] = "1"
    import time
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    from mgroms_amd.parallel import Comm
    from oracle.mgoracle import Oracle, make_seamount, seamount_geometry, rndtopo_geometry

    nhydro.set_verbose(0)
    comm = Comm(device="cuda", p2p=p2p)
    tol, maxit, nsc = (1e-6, 50, 40) if golden else (1e-9, 3, 6)
    mkw = dict(solver_maxiter=maxit) if model else {}
    par = nhydro.default_params(relax_method=method, solver_prec=tol, nsmall=nsmall, ns_coarsest=nsc, bmask=1 if bmask else 0, **mkw)
    nhydro.set_option("rb_exact", 1 if exact else 0)
    nhydro.set_option("rb_seq", 0 if par else 1)
    if fuse0:
        nhydro.set_option("rbseq_fuse_min", 0)
        nhydro.set_option("rbseq_window", 0)   # (the windowed walk, the default, needs no hand-off: this case is about the launch that has one)
    nhydro.set_option("overlap", 0 if overlap0 else 1)   # the exchange beside the interior sweep (off by default: slower on a shared GPU); the bits must not depend on it
    mg.nhydro_init(nx, ny, nz, npx, npy, rank, par, comm=comm)
    stamp("init")
    geometry = rndtopo_geometry if rndtopo else seamount_geometry
    dx, dy, zeta, h = geometry(nx, ny, npx, npy, rank)
    from mgroms_amd.testcases import curvilinear_metric, island_mask, resting_column_state

    def rank_metric(r):
        """dx, dy of rank r"""
        gx, gy = geometry(nx, ny, npx, npy, r)[:2]
        if curv:
            fx, fy = curvilinear_metric(nx, ny, npx, npy, r)
            gx, gy = gx * fx, gy * fy
        return gx, gy
    dx, dy = rank_metric(rank)
    rmask = island_mask(nx, ny, npx, npy, rank) if bmask else None
    mg.nhydro_matrices(dx, dy, zeta, h, rmask, 4e3, 0.0, 0.0)
    def rank_uvw(r):
        """u, v, w of rank r: (nz, ny+2, nx+1), (nz, ny+1, nx+2), (nz+1, ny+2, nx+2)"""
        if uvw_indep:
            g = np.random.default_rng(1000 + r)
            return g.standard_normal((nz, ny + 2, nx + 1)), g.standard_normal((nz, ny + 1, nx + 2)), g.standard_normal((nz + 1, ny + 2, nx + 2))
        g = np.random.default_rng(999)
        ug = g.standard_normal((nz, npy * ny + 2, npx * nx + 1))
        vg = g.standard_normal((nz, npy * ny + 1, npx * nx + 2))
        wg = g.standard_normal((nz + 1, npy * ny + 2, npx * nx + 2))
        qj, qi = (r // npx) * ny, (r % npx) * nx
        return (ug[:, qj:qj + ny + 2, qi:qi + nx + 1].copy(), vg[:, qj:qj + ny + 1, qi:qi + nx + 2].copy(),
                wg[:, qj:qj + ny + 2, qi:qi + nx + 2].copy())
    if model:
        u, v, w = rank_uvw(rank)
    else:
        u, v, w = resting_column_state(nx, ny, nz)
    nhydro.compute_rhs(u, v, w)
    stamp("matrices_rhs")
    t0 = time.time()
    n, hist = mg.solve_p(tol, maxit)
    t_solve = time.time() - t0
    stamp("solve")

    o = make_seamount(nx, ny, nz, npx, npy, relax_method=method, solver_prec=tol, nsmall=nsmall, ns_coarsest=nsc, bmask=bmask, **mkw)
    if bmask or rndtopo or curv:  # rebuild the oracle's matrices with every rank's mask / topography / metric in place
        for r in range(o.nranks):
            if curv:
                o.field("dx", 1, r)[...], o.field("dy", 1, r)[...] = rank_metric(r)
            if bmask:
                o.field("rmask", 1, r)[...] = island_mask(nx, ny, npx, npy, r)
            if rndtopo:
                o.field("h", 1, r)[...] = rndtopo_geometry(nx, ny, npx, npy, r)[3]
        o.matrices(4e3, 0.0, 0.0)
    if model:
        for r in range(o.nranks):
            for name, a in zip(("u", "v", "w"), rank_uvw(r)):
                o.field(name, 1, r)[...] = a
    o.compute_rhs()
    no, ho, _ = o.solve_p(tol, maxit)
    stamp("oracle")
    assert mg.nlevs() == o.nlevs
    gathered = [l for l in range(1, o.nlevs + 1) if o.level_info(l, rank)["gather"]]
    for lev in range(1, o.nlevs + 1):
        g = mg.grid(lev)
        for name in ("h", "zr", "cA") + (("dx", "dy") if curv else ()):   # (dx, dy: their halos between ranks and their coarsening)
            assert np.array_equal(g.get(name), o.field(name, lev, rank)), (rank, lev, name)
    if curv:
        assert np.ptp(mg.grid(1).get("dx")[1:-1, 0]) > 0 and np.ptp(mg.grid(1).get("dy")[0, 1:-1]) > 0   # the metric varies along the halo
    assert np.array_equal(mg.grid(1).b, o.field("b", 1, rank))
    assert n == no, (n, no)
    if method == "FC" or exact:
        # FC is order independent, and exact-order RB reproduces the reference's sequential sweep per rank (its result
        # depends on the decomposition, and the emulated ranks decompose the same way): every rank's block is bit-identical
        assert np.array_equal(mg.grid(1).p, o.field("p", 1, rank)), rank
        # p is bit-identical, so only the order of the norm's reduction differs from the oracle's: 1e-12 relative (the looser
        # 1e-10 of north_star is kept for the reference's RECORDED series below, which were printed by another build)
        assert np.all(np.abs(hist - ho) <= 1e-12 * np.abs(ho)), (hist, ho)
    elif par:  # parallel red-black: same-colour k=1 diagonals read as before the pass
        assert np.all(np.abs(hist - ho) <= 5e-5 * np.abs(ho))
    else:
        # the reference's sequential order per rank (halo cells old during a colour, as in the reference: its decomposition-dependent
        # result), reproduced up to the association of one sum per column: north_star's 1e-10 on the history and on p
        assert np.all(np.abs(hist - ho) <= 1e-13 + 1e-10 * np.abs(ho)), (hist, ho)
        pm, po = mg.grid(1).p, o.field("p", 1, rank)
        assert np.abs(pm - po).max() <= 1e-10 * np.abs(po).max(), (rank, np.abs(pm - po).max() / np.abs(po).max())
        # ... by the windowed walk on the levels with neighbours too (u is zero in a halo plane: a rank's walk starts at its own plane 1
        # or m planes back, whichever is later), unless this case asked for the launch with the hand-off
        assert (nhydro.get_option("rbseq_window_colours") > 0) == (not fuse0), (rank, nhydro.get_option("rbseq_window_colours"))
    if golden:  # the reference's own recorded history for this decomposition (BASELINE.md 3.1, 2x2 column)
        import json
        with open(os.path.join(ROOT, "tests", "golden", "baseline_known_answers.json")) as f:
            g = json.load(f)["seamount_%dx%dx%d_%s_%dx%dranks" % (nx * npx, ny * npy, nz, method, npx, npy)]
        ref = np.array(g["res"])
        assert n == g["nite"] == len(ref), (n, g["nite"])
        assert np.all(np.abs(hist[1:] - ref) <= (5e-5 * ref if par else 1e-13 + 1e-10 * ref)), (hist[1:], ref)
    # compute_residual on every level incl. the gathered ones: the redundant copies are counted once (the rescale of
    # global_sum, mg_mpi_exchange.f90:1569)
    for lev in (range(2, o.nlevs + 1) if (method == "FC" or exact) else ()):
        rl, rlo = mg.compute_residual(lev), o.residual(lev)
        assert abs(rl - rlo) <= 1e-12 * rlo + 1e-300, (lev, rl, rlo, lev in gathered)
    if method == "FC":
        # r's neighbour halo is exchanged lazily (nothing in the cycle reads it): asking for r must deliver the same
        # array, halo included, as the reference's eager fill (mg_relax.f90:373); all ranks ask together
        rres, rres_o = mg.compute_residual(1), o.residual(1)
        assert abs(rres - rres_o) <= 1e-12 * rres_o
        assert np.array_equal(mg.grid(1).r, o.field("r", 1, rank)), rank
    c = nhydro.counters()
    assert c["exchanges"] > 0 and c["allreduces"] > 0  # the set-up halos always use the callback
    if method == "FC" and p2p and not connectfail and not bmask and not overlap0:
        # the colour passes of the levels with neighbours ran in two parts on two streams, the exchange beside the interior part
        # (mgx_cycle.cpp relax()); the bits above are the oracle's, and the re-run through the hooks below (one stream) repeats them
        assert nhydro.get_option("overlap") == 1 and nhydro.get_option("overlapped_passes") > 0, rank
    if connectfail:
        assert comm.p2p_active is False and comm.p2p_error, (rank, comm.p2p_error)
        assert c["p2p_exchanges"] == 0
    else:
        assert (c["p2p_exchanges"] > 0) == p2p
    if p2p and method == "FC" and not connectfail:
        # same solve through the other transport (exchange callback): the iterates must not depend on it
        p_first = mg.grid(1).p
        comm.set_p2p(False)
        n2, hist2 = mg.solve_p(tol, maxit)
        assert n2 == n and np.array_equal(hist2, hist) and np.array_equal(mg.grid(1).p, p_first)
        assert nhydro.counters()["p2p_exchanges"] == c["p2p_exchanges"]
        comm.set_p2p(True)
    if model:
        # nhydro_solve as the model calls it: compute_rhs (with the flux exchange of mg_compute_rhs.f90:170-172, 271-273 unless bmask),
        # solve_p, correct_uvw on this rank's u, v, w -- every rank's p, u, v, w bit for bit against the oracle's emulated ranks
        mg.nhydro_solve(u, v, w)
        no2, _, _ = o.nhydro_solve()
        assert no2 == n, (no2, n)
        assert np.array_equal(mg.grid(1).b, o.field("b", 1, rank)), rank
        assert np.array_equal(mg.grid(1).p, o.field("p", 1, rank)), rank
        for name, a in (("u", u), ("v", v), ("w", w)):
            assert np.array_equal(a, o.field(name, 1, rank)), (rank, name)
    # src/old_tests/mg_testhalo.f90:75-92: fill p with the rank number, fill the halo: every halo plane holds the neighbour's
    # rank, or the own one across a physical boundary
    g1 = mg.grid(1)
    g1.set("p", np.full(g1._shape("p"), float(rank)))
    mg.fill_halo(1, "p")
    ph = g1.get("p")
    nbr = g1.neighb
    want = lambda q: float(q if q >= 0 else rank)
    assert np.all(ph[1:-1, 0, :] == want(nbr[0])) and np.all(ph[-1, 1:-1, :] == want(nbr[1])), rank
    assert np.all(ph[1:-1, -1, :] == want(nbr[2])) and np.all(ph[0, 1:-1, :] == want(nbr[3])), rank
    # the generic fill_halo of mg_mpi_exchange.f90:10-16 on the other array kinds: 2-D (dx), nh = 2 with the linear extrapolation
    # at physical sides (zr), and the 4-D cA (neighbour exchange only); rank-dependent random contents, halos compared with the
    # oracle's emulated exchange.  Last: set_field(cA) replaces the solver's matrix.
    if method == "FC":
        for name in ("dx", "zr", "cA"):
            for r in range(o.nranks):
                a = o.field(name, 1, r)
                a[...] = np.random.default_rng(77 + r).standard_normal(a.shape)
            g1.set(name, o.field(name, 1, rank))
            mg.fill_halo(1, name); o.fill_halo(1, name)
            assert np.array_equal(g1.get(name), o.field(name, 1, rank)), (rank, name)
    stamp("checks")
    mg.nhydro_clean()
    return f"nite={n} gathered_levels={gathered} exchanges={c['exchanges']} solve_s={t_solve:.1f}"


if __name__ == "__main__":
    main()
