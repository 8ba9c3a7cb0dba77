// Host side of libmgx.so, set-up: the level tables (mg_grids.f90), mgx_init's allocations, the matrix set-up (mg_define_matrix.f90),
// the model coupling (mg_compute_rhs.f90, mg_correct_uvw.f90) on the device copies of u, v, w, and mgx_clean.
#include "mgx_host.h"
#include "mgx_choice_depths.h"

namespace mgx_host {

int dmalloc(double **p, size_t n) {
  void *q = nullptr;
  HIPCHK(hipMalloc(&q, (n ? n : 1) * sizeof(double)));
  HIPCHK(hipMemsetAsync(q, 0, (n ? n : 1) * sizeof(double), S.stream));
  S.allocs.push_back(q);
  *p = (double *)q;
  return 0;
}

int roundup(int a, int m) { return (a + m - 1) / m * m; }

void make_view(LevView &v, int nx, int ny, int nz) {
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.EO = 15;
  v.HO = roundup(16 + ny / 2, 16);
  v.RS = roundup(v.HO + ny / 2 + 1, 16);
  v.plane = (long long)nz * v.RS;
}

// ---- mg_grids.f90:468-738 -------------------------------------------------------------------------
// hold (option "hold_odd_nz"): level l + 1 exists iff l < nl1 and nz_l != 2, with nz_{l+1} = nz_l / 2 for an even nz_l and nz_l for an odd one --
// for a size whose nz stays even down to 2 that is the reference's count
// hold_z (option "hold_z_levels" = m): the first m coarsenings (levels 1 -> 2 ... m -> m + 1) keep nz, whatever it is, and the rule above --
// the reference's or hold's -- applies from level m + 1 on: min(nl1, m + nl2) levels without hold; an m above nl1 - 1 holds every pair
int find_grid_levels(int npxg, int npyg, int nx, int ny, int nz, int hold, int hold_z) {
  const int nxg = npxg * nx, nyg = npyg * ny, nzg = nz, ncoarsest = 4, nzmin = 2;
  const int nhoriz = nxg < nyg ? nxg : nyg;
  const int nl1 = 1 + (int)floor(log(nhoriz * 1.0 / ncoarsest * 1.0) / log(2.0));
  if (hold) {
    int l = 1;
    for (int z = nzg; l < nl1 && (l <= hold_z || z != nzmin); l++) z = (l <= hold_z || (z & 1)) ? z : z / 2;
    return l;
  }
  const int nl2 = hold_z + 1 + (int)floor(log(nzg * 1.0 / nzmin * 1.0) / log(2.0));
  return nl1 < nl2 ? nl1 : nl2;
}

// level table of an arbitrary rank (needed to form gather groups without communication)
// periodic (option "periodic"): one step of the level past the last column of a periodic i direction wraps to column (pi +- incx) mod npx0 of the same
// row -- the rank's own column on a level with one rank along i -- and likewise in j; a corner exists exactly where both of its steps resolve, so
// between a periodic and a closed side it is absent (the mixed-corner rule of the halo fills then takes the closed side's image of the wrapped edge)
// hold (option "hold_odd_nz"): an odd nz is handed on unchanged; nx, ny and the gathers are what they are without it
// hold_z (option "hold_z_levels"): so do levels 1 .. hold_z, whatever their nz (semi-coarsening at the fine end)
void rank_level_table(int rank, std::vector<Level> &T, int npx0, int npy0, int nsmall, int periodic, int hold, int hold_z) {
  const int pi = rank % npx0, pj = rank / npx0;
  int nx = T[0].nx, ny = T[0].ny, nz = T[0].nz, npx = npx0, npy = npy0, incx = 1, incy = 1;
  T[0].npx = npx; T[0].npy = npy; T[0].incx = 1; T[0].incy = 1; T[0].gather = 0; T[0].ngx = 1; T[0].ngy = 1; T[0].key = 0; T[0].color = 0;
  for (int l = 1; l < (int)T.size(); l++) {  // define_grid_dims :503-577
    Level &L = T[l];
    if (nz == 1 || (hold && (nz & 1)) || l <= hold_z) { nx /= 2; ny /= 2; } else { nx /= 2; ny /= 2; nz /= 2; }
    L.gather = 0; L.ngx = 1; L.ngy = 1; L.key = 0; L.color = 0;
    if (((nx < ny ? nx : ny) < nsmall) && (npx * npy > 1)) {
      L.gather = 1;
      if (npx > 1) { npx /= 2; nx *= 2; L.ngx = 2; }
      if (npy > 1) { npy /= 2; ny *= 2; L.ngy = 2; }
      incx *= 2; incy *= 2;
    }
    L.nx = nx; L.ny = ny; L.nz = nz; L.npx = npx; L.npy = npy; L.incx = incx; L.incy = incy;
  }
  for (auto &L : T) {  // define_neighbours :580-661
    const int ix = L.incx, iy = L.incy;
    auto col = [&](int s) { const int t = pi + s * ix; return (t >= 0 && t < npx0) ? t : ((periodic & 1) ? ((t % npx0) + npx0) % npx0 : -1); };
    auto row = [&](int s) { const int t = pj + s * iy; return (t >= 0 && t < npy0) ? t : ((periodic & 2) ? ((t % npy0) + npy0) % npy0 : -1); };
    static const int di[8] = {0, 1, 0, -1, -1, 1, 1, -1}, dj[8] = {-1, 0, 1, 0, -1, -1, 1, 1};  // S,E,N,W,SW,SE,NE,NW
    for (int d = 0; d < 8; d++) {
      const int c = col(di[d]), r = row(dj[d]);
      L.neighb[d] = (c >= 0 && r >= 0) ? r * npx0 + c : -1;
    }
  }
  for (int l = 1; l < (int)T.size(); l++) {  // define_gather_informations :664-738
    Level &L = T[l];
    if (!L.gather) continue;
    const int ix = L.incx / 2, iy = L.incy / 2;
    const int family = (pi / ix) * ix * iy + npx0 * iy * (pj / iy);
    const int nextfamily = (pi / (2 * ix)) * ix * iy * 4 + npx0 * 2 * iy * (pj / (iy * 2));
    L.color = nextfamily + (pi % ix) + (pj % iy) * ix;
    const int N = ix * npx0;
    L.key = ((family % N) / (ix * iy)) % 2 + 2 * ((family / N) % 2);
  }
}

// ---- set-up: mg_define_matrix.f90:28-208 ----------------------------------------------------------
int gather2d(Level &L, double *src_tmp, double *dst) {
  const int nxc = L.nx / L.ngx, nyc = L.ny / L.ngy, Ng = nxc * nyc;
  rect(src_tmp, L.blk, 3, 1, 1, nyc, 1, nyc, 1, nxc);
  if (!S.ag) return fail("a gather is needed but mgx_set_comm was not called");
  if (S.ag(S.ctx, L.group, L.ngroup, L.blk, L.gbuf, Ng)) return fail("allgather callback failed");
  for (int q = 0; q < L.ngroup; q++) {
    const int l = q % L.ngx, m = q / L.ngx;
    rect(dst, L.gbuf + (size_t)q * Ng, 4, 1, 1, L.ny, 1 + m * nyc, (m + 1) * nyc, 1 + l * nxc, (l + 1) * nxc);
  }
  return 0;
}

// gather2d for the packed interior block of a 3-D depth array (nzz rows per column) the coarsening of the depths has left in `blk`:
// all-gather into `gbuf`, then every member's block into its place in the level's array dst (nzz, -1:ny+2, -1:nx+2)
static int gather_depths(Level &L, double *blk, double *gbuf, double *dst, int nzz) {
  const int nxc = L.nx / L.ngx, nyc = L.ny / L.ngy, Ng = nzz * nxc * nyc;
  if (!S.ag) return fail("a gather is needed but mgx_set_comm was not called");
  if (S.ag(S.ctx, L.group, L.ngroup, blk, gbuf, Ng)) return fail("allgather callback failed");
  for (int q = 0; q < L.ngroup; q++) {
    const int l = q % L.ngx, m = q / L.ngx;
    rect(dst, gbuf + (size_t)q * Ng, 4, nzz, 2, L.ny, 1 + m * nyc, (m + 1) * nyc, 1 + l * nxc, (l + 1) * nxc);
  }
  return 0;
}

// the planes of warm-up each level's windowed red-black walk needs (mgx_rbseq.hip: k_rbseq_window), from the rho the set-up has just copied back
// (known = false: the set-up did not copy rho and the decay figures back -- every level keeps the walk over the whole level)
void set_window_planes(bool known) {
  for (int l = 0; l < S.nlevs && l < 32; l++) {
    Level &L = S.lev[l];
    if (!L.v.gk || !S.rho_dev || !known) { L.rbs_rho = -1.0; L.rbs_m = 0; L.rbs_rows = L.nz; continue; }
    L.rbs_rho = S.rho_host[l];
    L.rbs_m = mgxk_rbseq_window_planes(L.rbs_rho);
    L.rbs_rows = (L.gdec && !L.gdec_h.empty()) ? mgxk_rbseq_window_rows(L.gdec_h.data(), L.nz) : L.nz;
    if (S.verbose > 1 && S.rank == 0) printf(" level %d: red-black walk contracts by %.4g per plane: %d planes of warm-up%s\n", l + 1, L.rbs_rho, L.rbs_m, L.rbs_m ? "" : " (none: the walk over the whole level stays)");
  }
}

// zeta of a hierarchy whose levels are all closed and un-gathered, from the interior of level 1: every coarser level and the halos of all
// of them in one launch per mgxs_zeta_chain_depth() levels (mgx_setup.hip: k_zeta_chain).  false = not such a hierarchy, nothing was enqueued.
static bool zeta_chain() {
  for (int l = 0; l < S.nlevs; l++) {
    const Level &L = S.lev[l];
    if (L.gather || !all_physical(sides_of(L))) return false;
    if (l > 0 && (2 * L.nx != S.lev[l - 1].nx || 2 * L.ny != S.lev[l - 1].ny)) return false;
  }
  const int D = mgxs_zeta_chain_depth();
  for (int s = 0;; s += D) {
    const int nd = std::min(D, S.nlevs - 1 - s);
    double *a[16];
    for (int d = 0; d <= nd; d++) a[d] = S.lev[s + d].g.zeta;
    mgxs_zeta_chain(S.stream, a, S.lev[s].ny, S.lev[s].nx, nd); S.n_launch++;
    if (s + nd >= S.nlevs - 1) break;
  }
  return true;
}

// The level-1 mask across the periodic sides: first the i direction, whole planes (j = 0..ny+1 as they stand), then the j direction, whole rows
// (i = 0..nx+1, the planes just wrapped included) -- the order that makes the result the one-rank array on every process grid.  Only the sides ON the
// wrap seam are replaced (the first and last rank of a row or column; a rank seam inside the domain keeps the halo the caller gave): by the
// interior of the rank at the other end, through exchange(), which serves a rank that is its own neighbour by device copies.
static int wrap_rmask(Level &L) {
  for (int ax = 0; ax < 2; ax++) {
    if (!(S.periodic & (1 << ax))) continue;
    const int lo = ax == 0 ? 3 : 0, hi = ax == 0 ? 1 : 2;                                    // W,E or S,N
    const bool first = ax == 0 ? S.pi == 0 : S.pj == 0, last = ax == 0 ? S.pi == S.npx - 1 : S.pj == S.npy - 1;
    const int nn = ax == 0 ? L.nx : L.ny, cnt = (ax == 0 ? L.ny : L.nx) + 2;
    if ((size_t)cnt > S.xbuf_n) return fail("halo buffer too small");
    auto line = [&](double *buf, int op, int c) { if (ax == 0) rect(L.g.rmask, buf, op, 1, 1, L.ny, 0, L.ny + 1, c, c); else rect(L.g.rmask, buf, op, 1, 1, L.ny, c, c, 0, L.nx + 1); };
    int n = 0, peer[2], cn[2], dr[2]; double *sb[2], *rb[2];
    if (first) { line(S.xbuf[lo], 3, 1); peer[n] = L.neighb[lo]; cn[n] = cnt; sb[n] = S.xbuf[lo]; rb[n] = S.xbuf[8 + lo]; dr[n] = lo; n++; }
    if (last) { line(S.xbuf[hi], 3, nn); peer[n] = L.neighb[hi]; cn[n] = cnt; sb[n] = S.xbuf[hi]; rb[n] = S.xbuf[8 + hi]; dr[n] = hi; n++; }
    if (!n) continue;
    CHK(exchange(n, peer, sb, rb, cn, dr));
    if (first) line(S.xbuf[8 + lo], 4, 0);
    if (last) line(S.xbuf[8 + hi], 4, nn + 1);
  }
  return 0;
}

// what = DM_ALL: the level-1 dx, dy, zeta, h (and rmask) are new (mgx_matrices, mgx_matrices_device).  what = DM_ZETA: only the level-1 zeta is
// (mgx_update_zeta_device) -- dx, dy, h of every level, their halos, the coarse masks, the sigma tables, the 2-D factors of k_zw_js and the
// model-space copies of dx, dy, rmask are what the last DM_ALL left and stay; everything zeta reaches is rebuilt by the same kernels in the
// same order.  may_return_early: the caller is one of the device entry points, which under option "async" only enqueue -- unless the
// sequential-order red-black needs rho and the decay figures of the new coefficients on the host (set_window_planes).
// what = DM_DEPTHS_ALL: the level-1 dx, dy (and rmask) are new and the interior of the level-1 zr, zw holds the caller's depths
// (mgx_matrices_depths, mgx_matrices_depths_device); what = DM_DEPTHS: only those depths are new (mgx_update_depths_device).  No h, zeta or
// stretching then: zeta and h are not coarsened, k_zr_zw and k_zw_js do not run; every coarser level's depths are averages of the finer
// level's (k_depths_coarsen, the rule of DESIGN.md 6.4; through the packed blocks and an all-gather on a gathered level), h and zeta of
// every level are read off its zw (k_depths_hz), and everything from the halo fills of zr, zw on is what the other modes run.  The levels
// keep their slopes and lose the nine sigma fields (LevShape: slopes without zw); a level whose colour pass cannot do without them hands it
// the stored coefficients (Level::pass_stored).  A halving from an odd nz is refused before anything is enqueued.
int define_matrices(int what, bool may_return_early) {
  const bool depths = what == DM_DEPTHS_ALL || what == DM_DEPTHS;
  const bool all = what == DM_ALL || what == DM_DEPTHS_ALL;
  if (depths)
    for (int l = 1; l < S.nlevs; l++)
      if (depths_pair(S.lev[l - 1].nz, S.lev[l].nz) == DEPTHS_REFUSED)
        return fail("the depths of level %d (nz = %d) have no coarsening onto level %d (nz = %d): halving from an odd nz has no top interface; set option \"hold_odd_nz\" = 1 before mgx_init", l, S.lev[l - 1].nz, l + 1, S.lev[l].nz);
  const bool wait = !(may_return_early && S.async_ops) || (S.rho_dev && S.rb_seq);
  if (S.rho_dev) HIPCHK(hipMemsetAsync(S.rho_dev, 0, sizeof S.rho_host, S.stream));
  const bool chained = what == DM_ZETA && zeta_chain();
  if (chained) S.n_zeta_chain++;
  for (int l = 0; l < S.nlevs; l++) {
    Level &L = S.lev[l];
    if (l > 0) {
      Level &F = S.lev[l - 1];
      const int nxc = L.gather ? L.nx / L.ngx : L.nx, nyc = L.gather ? L.ny / L.ngy : L.ny;
      double *src[4] = {F.g.dx, F.g.dy, F.g.zeta, F.g.h};
      double *own[4] = {L.g.dx, L.g.dy, L.g.zeta, L.g.h};
      const double fac[4] = {0.5, 0.5, 0.25, 0.25};
      for (int q = 0; q < 4; q++) {
        if (depths ? (!all || q >= 2) : (!all && (q != 2 || chained))) continue;
        mgxs_coarsen2d(S.stream, src[q], L.gather ? L.tmp2[q] : own[q], F.ny, nyc, nxc, fac[q]); S.n_launch++;
        if (L.gather) CHK(gather2d(L, L.tmp2[q], own[q]));
      }
      if (depths) {
        mgxd_coarsen(S.stream, &F.g, nxc, nyc, L.nz, L.gather ? L.blk : L.g.zr, L.gather ? L.dblk : L.g.zw, L.gather ? 1 : 0); S.n_launch++;
        if (L.gather) { CHK(gather_depths(L, L.blk, L.gbuf, L.g.zr, L.nz)); CHK(gather_depths(L, L.dblk, L.dgbuf, L.g.zw, L.nz + 1)); }
      }
    }
    if (all) CHK(rl_fill_halo(L, L.g.dx, 1, 1, 0));
    if (all) CHK(rl_fill_halo(L, L.g.dy, 1, 1, 0));
    if (!chained && !depths) CHK(rl_fill_halo(L, L.g.zeta, 1, 1, 0));
    if (all && !depths) CHK(rl_fill_halo(L, L.g.h, 1, 1, 0));
    // option "periodic": the caller's mask wraps like the geometry; whole rows and planes, so that a corner between a periodic and a closed side is
    // the wrapped image of the mask the caller gave on the closed side (the closed halo of a mask is the caller's to set, never a mirror)
    if (all && l == 0 && S.par.bmask && S.periodic) CHK(wrap_rmask(L));
    if (!depths) { mgxs_zr_zw(S.stream, &L.g, S.hlim, S.theta_b, S.theta_s); S.n_launch++; }
    CHK(rl_fill_halo(L, L.g.zr, L.nz, 2, 0));
    CHK(rl_fill_halo(L, L.g.zw, L.nz + 1, 2, 0));
    if (depths) { mgxd_hz(S.stream, &L.g); S.n_launch++; }   // h = -zw(1), zeta = zw(nz+1) on 0:n+1
    // (no clearing of the cA scratch: k_cA_offdiag stores every slot of every cell, zeros included)
    L.g.bmask = S.par.bmask ? 1 : 0;
    if (l > 0 && all) {  // boundary mask of a coarse level = 1, 0 in the physical halo when bmask (:157-161, fill_halo_2D_bmask)
      rect(L.g.rmask, 0, 5, 1, 1, L.ny, 0, L.ny + 1, 0, L.nx + 1);
      if (S.par.bmask) {
        if (L.neighb[0] < 0) rect(L.g.rmask, 0, 2, 1, 1, L.ny, 0, 0, 0, L.nx + 1);
        if (L.neighb[1] < 0) rect(L.g.rmask, 0, 2, 1, 1, L.ny, 0, L.ny + 1, L.nx + 1, L.nx + 1);
        if (L.neighb[2] < 0) rect(L.g.rmask, 0, 2, 1, 1, L.ny, L.ny + 1, L.ny + 1, 0, L.nx + 1);
        if (L.neighb[3] < 0) rect(L.g.rmask, 0, 2, 1, 1, L.ny, 0, L.ny + 1, 0, 0);
      }
    }
    L.g.szx = L.g.szy + (size_t)L.nz * (L.ny + 2) * (L.nx + 2);
    mgxs_slopes_ref(S.stream, &L.g); S.n_launch++;  // zy, zx once per cell: the cross coefficients and the smoother's matrix-free slopes both come from here
    mgxs_define_matrix(S.stream, &L.g, l == 0, 0); S.n_launch += 2;
    // fill_halo(lev,cA), mg_define_matrix.f90:611-613: the 4-D exchange, slot by slot (the set-up scratch is slot-major)
    if (S.par.bmask) for (int s = 0; s < 8; s++) CHK(rl_fill_halo(L, L.g.cA + (size_t)s * L.nz * (L.ny + 2) * (L.nx + 2), L.nz, 1, 0, true));
    mgxs_define_matrix(S.stream, &L.g, l == 0, 1); S.n_launch++;
    if (l == 0) {  // i-fastest copies for compute_rhs / correct_uvw (mgx_model.hip)
      mgxm_ref2model(S.stream, L.g.zw, L.g.mzw, L.nz + 1, 2, L.nx, L.ny);
      mgxm_ref2model(S.stream, L.g.dzw, L.g.mdzw, L.nz + 1, 1, L.nx, L.ny);
      mgxm_ref2model(S.stream, L.g.cw, L.g.mcw, L.nz + 1, 1, L.nx, L.ny);
      mgxm_ref2model(S.stream, L.g.zxdy, L.g.mzxdy, L.nz, 1, L.nx, L.ny);
      mgxm_ref2model(S.stream, L.g.zydx, L.g.mzydx, L.nz, 1, L.nx, L.ny);
      S.n_launch += 5;
      if (all) {
        mgxm_ref2model_2d(S.stream, L.g.dx, L.g.mdx, L.nx, L.ny);
        mgxm_ref2model_2d(S.stream, L.g.dy, L.g.mdy, L.nx, L.ny);
        mgxm_ref2model_2d(S.stream, L.g.rmask, L.g.mrmask, L.nx, L.ny);
        S.n_launch += 3;
      }
    }
    if (L.nz <= 1024) { mgxk_convert8(S.stream, &L.v, L.g.cA); S.n_launch++; }  // LDS-tiled transposition, one slot per block
    else for (int s = 0; s < 8; s++) { mgxk_convert(S.stream, &L.v, L.v.cA[s], L.g.cA + (size_t)s * L.nz * (L.ny + 2) * (L.nx + 2), 1, 0, 0); S.n_launch++; }
    mgxs_pivots(S.stream, &L.v); S.n_launch++;
    if (L.v.gk) { mgxk_rbseq_setup(S.stream, &L.v); S.n_launch++; }
    if (L.v.gk && S.rho_dev && l < 32) { mgxk_rbseq_rho(S.stream, &L.v, S.rho_dev + l); S.n_launch++; }
    if (L.v.gk && L.gdec) {
      HIPCHK(hipMemsetAsync(L.gdec, 0, (size_t)L.nz * sizeof(double), S.stream));
      mgxk_rbseq_gdecay(S.stream, &L.v, L.gdec); S.n_launch++;
      if (wait) HIPCHK(hipMemcpyAsync(L.gdec_h.data(), L.gdec, (size_t)L.nz * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    }
    L.v.zy = L.zy_store; L.v.zx = L.zx_store;
    if (L.nz <= 1024) { mgxk_convert2(S.stream, &L.v, L.zy_store, L.zx_store, L.g.szy); S.n_launch++; }
    else { mgxk_convert(S.stream, &L.v, L.zy_store, L.g.szy, 1, 0, 0); mgxk_convert(S.stream, &L.v, L.zx_store, L.g.szx, 1, 0, 0); S.n_launch += 2; }
    if (depths) {  // the caller's depths follow no formula a kernel could generate them from: slopes, and slots 4 / 7 as stored
      L.v.m4 = L.v.d4 = L.v.m7 = L.v.d7 = L.v.h2 = L.v.hi2 = L.v.ze2 = nullptr; L.v.cffw = L.v.csw = nullptr;
      L.v.dx2 = L.v.dy2 = nullptr; L.v.cffr = L.v.csr = nullptr;
    } else {
      L.v.m4 = L.f2d_store[0]; L.v.d4 = L.f2d_store[1]; L.v.m7 = L.f2d_store[2]; L.v.d7 = L.f2d_store[3];
      L.v.h2 = L.f2d_store[4]; L.v.hi2 = L.f2d_store[5]; L.v.ze2 = L.f2d_store[6]; L.v.cffw = L.tab_store[0]; L.v.csw = L.tab_store[1];
      L.v.dx2 = L.zg_store[0]; L.v.dy2 = L.zg_store[1]; L.v.cffr = L.zg_store[2]; L.v.csr = L.zg_store[3];
      if (all) { mgxs_zw_js(S.stream, &L.g, &L.v, S.hlim, S.theta_b, S.theta_s); S.n_launch += 3; }
      else { mgxs_ze2_js(S.stream, &L.g, &L.v); S.n_launch++; }  // of the 2-D factors and tables only ze2 holds zeta
    }
    L.pass_stored = depths && depths_pass_stored(L.nz);
    if (S.no_mf || S.par.bmask) { L.v.zy = L.v.zx = nullptr; L.v.m4 = nullptr; }  // masked coefficients are not rebuilt from the slopes
  }
  if (wait) {
    if (S.rho_dev) HIPCHK(hipMemcpyAsync(S.rho_host, S.rho_dev, sizeof S.rho_host, hipMemcpyDeviceToHost, S.stream));
    CHK(sync_stream());
  }
  set_window_planes(wait);
  S.cd_valid = 0;
  S.coef_gen++;
  S.have_matrix = true;
  S.have_geometry = true;
  S.depths_user = depths;
  return 0;
}

// the model fields + the mask of the call.  The reference multiplies the w cross terms of compute_rhs by the rmask of the
// call whatever bmask says, and builds umask / vmask from it only when bmask (mg_compute_rhs.f90:56-72,110-111,
// mg_correct_uvw.f90:51-68).  Without a per-call mask (NULL): the level-1 mask of nhydro_matrices when bmask, else all ones.
ModelView model_view() {
  double *m = S.call_mask ? S.d_rmask_m : (S.par.bmask ? S.lev[0].g.mrmask : nullptr);
  return ModelView{S.d_u, S.d_v, S.d_w, m, S.par.bmask ? 1 : 0, S.state_f32, S.state_view, S.state_str};
}

// the model state of one call in place of the library's fp64 staging copies: the caller's device arrays (the *_device entries), or the
// staging buffers themselves holding floats (the host *_f32 entries: u = v = w = nullptr); with `str`, the caller's arrays are the model's own
// padded ones (the *_view entries).  Put back when the call ends, whatever it returns.
StateScope::StateScope(void *u, void *v, void *w, bool f32, const mgx_state_strides *str)
    : su(S.d_u), sv(S.d_v), sw(S.d_w), sf(S.state_f32), sview(S.state_view), sstr(S.state_str) {
  if (u) { S.d_u = (double *)u; S.d_v = (double *)v; S.d_w = (double *)w; }
  S.state_f32 = f32 ? 1 : 0;
  S.state_view = str ? 1 : 0;
  if (str) S.state_str = *str;
}
StateScope::~StateScope() { S.d_u = su; S.d_v = sv; S.d_w = sw; S.state_f32 = sf; S.state_view = sview; S.state_str = sstr; }

// rmaska of nhydro_solve / nhydro_check_nondivergence: (0:ny+1,0:nx+1), j fastest -- the layout the reference's drivers
// allocate (mg_testseamount.f90:97) and compute_rhs indexes (rmask(j,i)).  `dev`: the pointer is a device pointer.
int set_call_mask(const double *rmask, bool dev) {
  S.call_mask = rmask != nullptr;
  if (!rmask) return 0;
  Level &L = S.lev[0];
  const size_t n2 = (size_t)(L.ny + 2) * (L.nx + 2) * sizeof(double);
  HIPCHK(hipMemcpyAsync(S.d_rmask_ref, rmask, n2, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, S.stream));
  mgxm_ref2model_2d(S.stream, S.d_rmask_ref, S.d_rmask_m, L.nx, L.ny); S.n_launch++;
  return 0;
}

// fill_halo(1,uf,lbc_null='u') / fill_halo(1,vf,lbc_null='v') (mg_compute_rhs.f90:171,272), reduced to the entries the
// divergence reads: the first and last face.  Physical side: zero flux.  Neighbour: my last face is the neighbour's first
// face, computed over there from its own copy of the shared velocity (the reference takes that value too).
int flux_halo(Level &L, int face, double *fx) {
  const int lo = face == 0 ? L.neighb[3] : L.neighb[0], hi = face == 0 ? L.neighb[1] : L.neighb[2];  // W,E or S,N
  const int last = face == 0 ? L.nx + 1 : L.ny + 1, cnt = L.nz * (face == 0 ? L.ny : L.nx);
  if (lo < 0) { mgxm_flux_zero_face(S.stream, &L.g, fx, face, 1); S.n_launch++; }
  if (hi < 0) { mgxm_flux_zero_face(S.stream, &L.g, fx, face, last); S.n_launch++; }
  if (lo < 0 && hi < 0) return 0;
  if ((size_t)cnt > S.xbuf_n) return fail("halo buffer too small");
  // the exchange callback moves equal counts both ways with every peer: the unused direction carries a zero buffer
  int n = 0, peer[2], cn[2], dr[2]; double *sb[2], *rb[2];
  if (lo >= 0) { mgxm_flux_face_copy(S.stream, &L.g, fx, S.xbuf[0], face, 1, 0); S.n_launch++; peer[n] = lo; cn[n] = cnt; sb[n] = S.xbuf[0]; rb[n] = S.xbuf[8]; dr[n] = face == 0 ? 3 : 0; n++; }
  if (hi >= 0) { peer[n] = hi; cn[n] = cnt; sb[n] = S.xbuf[2]; rb[n] = S.xbuf[9]; dr[n] = face == 0 ? 1 : 2; n++; }
  if (hi >= 0) HIPCHK(hipMemsetAsync(S.xbuf[2], 0, (size_t)cnt * sizeof(double), S.stream));
  CHK(exchange(n, peer, sb, rb, cn, dr));
  if (hi >= 0) { mgxm_flux_face_copy(S.stream, &L.g, fx, S.xbuf[9], face, last, 1); S.n_launch++; }
  return 0;
}

// mg_compute_rhs.f90:14-379 on the device copies of u,v,w
int compute_rhs_dev() {
  Level &L = S.lev[0];
  TicScope ts(1, "compute_rhs");  // nhydro.f90:81
  ModelView M = model_view();
  HIPCHK(hipMemsetAsync(L.v.b, 0, L.n3js * sizeof(double), S.stream));
  mgxm_rhs_uf(S.stream, &L.g, &M, S.d_fx); S.n_launch++;
  if (!S.par.bmask) CHK(flux_halo(L, 0, S.d_fx));  // mg_compute_rhs.f90:170-172
  mgxm_rhs_vf(S.stream, &L.g, &M, S.d_fy); S.n_launch++;
  if (!S.par.bmask) CHK(flux_halo(L, 1, S.d_fy));  // :271-273
  mgxm_rhs_wf(S.stream, &L.g, &M, S.d_fz); S.n_launch++;
  mgxm_rhs_accum(S.stream, &L.g, S.d_bm, S.d_fx, S.d_fy, S.d_fz); S.n_launch++;  // :173, :274, :362-370 in one pass, same order
  mgxm_js_model(S.stream, &L.v, L.v.b, S.d_bm, 1); S.n_launch++;  // interior of b in the solver's layout
  return 0;
}

// mg_correct_uvw.f90:15-115 on the device copies of u,v,w
int correct_uvw_dev() {
  Level &L = S.lev[0];
  TicScope ts(1, "correct_uvw");
  ModelView M = model_view();
  mgxm_js_model(S.stream, &L.v, L.v.p, S.d_bm, 0); S.n_launch++;
  mgxm_correct_uvw(S.stream, &L.g, S.d_bm, &M); S.n_launch++;
  return 0;
}

// host u, v, w <-> the staging buffers; esz: the size of an element of the state (8, or 4 for the float state, which fills their first half)
static int copy_uvw(void *u, void *v, void *w, size_t esz, bool up) {
  Level &L = S.lev[0];
  const size_t nu = (size_t)(L.nx + 1) * (L.ny + 2) * L.nz, nv = (size_t)(L.nx + 2) * (L.ny + 1) * L.nz, nw = (size_t)(L.nx + 2) * (L.ny + 2) * (L.nz + 1);
  const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  HIPCHK(hipMemcpyAsync(up ? (void *)S.d_u : u, up ? u : (void *)S.d_u, nu * esz, kind, S.stream));
  HIPCHK(hipMemcpyAsync(up ? (void *)S.d_v : v, up ? v : (void *)S.d_v, nv * esz, kind, S.stream));
  HIPCHK(hipMemcpyAsync(up ? (void *)S.d_w : w, up ? w : (void *)S.d_w, nw * esz, kind, S.stream));
  return 0;
}
int upload_uvw(const void *u, const void *v, const void *w, size_t esz) { return copy_uvw((void *)u, (void *)v, (void *)w, esz, true); }
int download_uvw(void *u, void *v, void *w, size_t esz) { return copy_uvw(u, v, w, esz, false); }

int apply_params(const mgx_params &p) {
  if (streq(p.relax_method, "GS") || streq(p.relax_method, "Gauss-Seidel")) S.method = M_GS;
  else if (streq(p.relax_method, "RB") || streq(p.relax_method, "Red-Black")) S.method = M_RB;
  else if (streq(p.relax_method, "FC") || streq(p.relax_method, "Four-Color")) S.method = M_FC;
  else return fail("unknown relax_method '%s'", p.relax_method);
  S.real = streq(p.cmatrix, "real") ? 1 : 0;
  if (streq(p.interp_type, "linear")) S.linear = 1; else if (streq(p.interp_type, "nearest")) S.linear = 0; else return fail("unknown interp_type '%s'", p.interp_type);
  if (S.linear && streq(p.restrict_type, "linear")) return fail("linear interp + linear restrict is not permitted");
  if (p.aggressive) return fail("aggressive=.true.: coarse2fine_aggressive is not available in the reference either (mg_intergrids.f90:243)");
  S.par = p;
  return 0;
}

}  // namespace mgx_host
using namespace mgx_host;

extern "C" {

void mgx_clean(void) {
  if (S.stream || S.inited) (void)hipStreamSynchronize(S.stream);
  p2p_release();
  for (void *q : S.allocs) (void)hipFree(q);
  if (S.h_scalar) (void)hipHostFree(S.h_scalar);
  if (S.kerr) (void)hipHostFree(S.kerr);
  if (S.stream2) { (void)hipStreamSynchronize(S.stream2); (void)hipStreamDestroy(S.stream2); }
  if (S.ev_a) (void)hipEventDestroy(S.ev_a);
  if (S.ev_s) (void)hipEventDestroy(S.ev_s);
  if (S.ev_x) (void)hipEventDestroy(S.ev_x);
  tt_collect();
  hipStream_t st = S.stream; const int vb = S.verbose; const std::vector<int> opts = options_carried();
  mgx_exchange_fn ex = S.ex; mgx_allreduce_fn ar = S.ar; mgx_allgather_fn ag = S.ag; void *ctx = S.ctx; const bool nat = S.native_rccl;
  // the timer table is module state of mg_tictoc in the reference: it outlives nhydro_clean (the drivers print it afterwards, mg_testseamount.f90:220-221)
  std::vector<std::string> tn = S.tt_names; std::vector<HostTic> th = S.tt_host; const int tnb = S.tt_nblev;
  static thread_local double tsave[32][32]; static thread_local long long csave[32][32];
  memcpy(tsave, S.tt_time, sizeof tsave); memcpy(csave, S.tt_calls, sizeof csave);
  S = State();
  S.tt_names = tn; S.tt_host = th; S.tt_nblev = tnb; memcpy(S.tt_time, tsave, sizeof tsave); memcpy(S.tt_calls, csave, sizeof csave);
  S.native_rccl = nat;
  S.stream = st; S.verbose = vb; options_restore(opts); S.ex = ex; S.ar = ar; S.ag = ag; S.ctx = ctx;
}

int mgx_init(int nx, int ny, int nz, int npx, int npy, int rank, const mgx_params *par) {
  if (S.inited) mgx_clean();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible: libmgx has no CPU path");
  mgx_params p;
  if (par) p = *par; else { mgx_params_default(&p); CHK(mgx_read_namelist(nullptr, &p)); }
  CHK(apply_params(p));
  if (nx < 2 || ny < 2 || nz < 2 || (nx & 1) || (ny & 1) || (nz & 1)) return fail("nx,ny,nz must be even and >= 2 (got %d %d %d)", nx, ny, nz);
  if (npx < 1 || npy < 1 || (npx & (npx - 1)) || (npy & (npy - 1))) return fail("the process grid must be powers of two in both directions (got %d x %d)", npx, npy);
  if (rank < 0 || rank >= npx * npy) return fail("rank %d outside the %d x %d process grid", rank, npx, npy);
  // a periodic process grid is served through the transports of a rank seam: unlike a closed grid, whose first exchange reports missing hooks,
  // it is refused here, before anything is built, while the ranks are not connected
  if (S.periodic && npx * npy > 1 && !S.ex)
    return fail("option \"periodic\" = %d needs a single rank (process grid %d x %d) or connected ranks: install the hooks (mgx_set_comm, mgx_rccl_connect) before mgx_init", S.periodic, npx, npy);
  S.npx = npx; S.npy = npy; S.nranks = npx * npy; S.rank = rank; S.pi = rank % npx; S.pj = rank / npx;
  S.nlevs = find_grid_levels(npx, npy, nx, ny, nz, S.hold_odd_nz, S.hold_z_levels);
  if (S.nlevs < 1) return fail("grid %dx%dx%d too small for a multigrid hierarchy", nx * npx, ny * npy, nz);
  S.lev.assign(S.nlevs, Level());
  S.lev[0].nx = nx; S.lev[0].ny = ny; S.lev[0].nz = nz;
  rank_level_table(rank, S.lev, npx, npy, S.par.nsmall, S.periodic, S.hold_odd_nz, S.hold_z_levels);
  for (int l = 0; l < S.nlevs; l++) {
    const Level &L = S.lev[l];
    if ((L.nx & 1) || (L.ny & 1) || L.nz < 2) return fail("level %d has local size %dx%dx%d: odd sizes are not supported (assumptions:1-2)", l + 1, L.nx, L.ny, L.nz);
  }
  // gather groups: ranks with my colour, ordered by (key, rank)  (MPI_COMM_SPLIT, mg_grids.f90:717)
  for (int l = 1; l < S.nlevs; l++) {
    Level &L = S.lev[l];
    if (!L.gather) continue;
    std::vector<std::pair<int, int>> mem;
    for (int r = 0; r < S.nranks; r++) {
      std::vector<Level> T(S.nlevs);
      T[0].nx = nx; T[0].ny = ny; T[0].nz = nz;
      rank_level_table(r, T, npx, npy, S.par.nsmall, 0, S.hold_odd_nz, S.hold_z_levels);
      if (T[l].color == L.color) mem.push_back({T[l].key, r});
    }
    std::sort(mem.begin(), mem.end());
    L.ngroup = (int)mem.size();
    if (L.ngroup != L.ngx * L.ngy) return fail("gather group of level %d has %d members, expected %d", l + 1, L.ngroup, L.ngx * L.ngy);
    for (int q = 0; q < L.ngroup; q++) L.group[q] = mem[q].second;
  }
  // allocations
  size_t max_part = 1;
  for (int l = 0; l < S.nlevs; l++) {
    Level &L = S.lev[l];
    make_view(L.v, L.nx, L.ny, L.nz);
    L.n3js = (size_t)(L.nx + 2) * L.v.plane;
    CHK(dmalloc(&L.v.p, L.n3js)); CHK(dmalloc(&L.v.b, L.n3js)); CHK(dmalloc(&L.v.r, L.n3js));
    for (int s = 0; s < 8; s++) CHK(dmalloc(&L.v.cA[s], L.n3js));
    CHK(dmalloc(&L.v.bet, L.n3js)); CHK(dmalloc(&L.v.gam, L.n3js));
    CHK(dmalloc(&L.v.p1, (size_t)(L.nx + 2) * L.v.RS)); CHK(dmalloc(&L.p1b, (size_t)(L.nx + 2) * L.v.RS)); L.v.p1w = nullptr;
    { double *q = nullptr; CHK(dmalloc(&q, (size_t)(L.nx + 2) / 2 + 1)); L.ksp_done = (unsigned int *)q; L.ksp_seq = 0; }  // zeroed by dmalloc
    CHK(dmalloc(&L.zy_store, L.n3js)); CHK(dmalloc(&L.zx_store, L.n3js));
    L.v.zy = L.v.zx = nullptr;
    for (int q = 0; q < 7; q++) CHK(dmalloc(&L.f2d_store[q], (size_t)(L.nx + 2) * L.v.RS));
    for (int q = 0; q < 2; q++) CHK(dmalloc(&L.tab_store[q], (size_t)L.nz + 1));
    L.v.m4 = L.v.d4 = L.v.m7 = L.v.d7 = L.v.h2 = L.v.hi2 = L.v.ze2 = nullptr; L.v.cffw = L.v.csw = nullptr;
    for (int q = 0; q < 2; q++) CHK(dmalloc(&L.zg_store[q], (size_t)(L.nx + 2) * L.v.RS));
    for (int q = 2; q < 4; q++) CHK(dmalloc(&L.zg_store[q], (size_t)L.nz + 1));
    L.v.dx2 = L.v.dy2 = nullptr; L.v.cffr = L.v.csr = nullptr;
    L.v.gk = L.v.ag58 = L.v.u1 = nullptr; L.v.d0w = nullptr;
    if (S.method == M_RB && S.real) {  // sequential-order red-black (mgx_rbseq.hip): +8 B per cell
      CHK(dmalloc(&L.v.gk, L.n3js));
      CHK(dmalloc(&L.gdec, (size_t)L.nz)); L.gdec_h.assign((size_t)L.nz, 0.0);
      CHK(dmalloc(&L.v.ag58, (size_t)2 * (L.nx + 2) * L.v.RS)); CHK(dmalloc(&L.v.u1, (size_t)(L.nx + 2) * L.v.RS));
      { double *q = nullptr; CHK(dmalloc(&q, (size_t)(L.nx / 8 + 2) * 8 + 16)); L.rbs_flag = (unsigned int *)q; L.rbs_seq = 0; }  // one word per chunk of 8 planes, 64 B apart (zeroed by dmalloc): what the walk has handed to the correction workers
    }
    const size_t n2 = (size_t)(L.ny + 2) * (L.nx + 2);
    L.g.nx = L.nx; L.g.ny = L.ny; L.g.nz = L.nz;
    CHK(dmalloc(&L.g.dx, n2)); CHK(dmalloc(&L.g.dy, n2)); CHK(dmalloc(&L.g.zeta, n2)); CHK(dmalloc(&L.g.h, n2));
    CHK(dmalloc(&L.g.rmask, n2)); L.g.bmask = 0;
    CHK(dmalloc(&L.g.zr, (size_t)(L.ny + 4) * (L.nx + 4) * L.nz));
    CHK(dmalloc(&L.g.zw, (size_t)(L.ny + 4) * (L.nx + 4) * (L.nz + 1)));
    CHK(dmalloc(&L.g.cw, n2 * (L.nz + 1)));
    L.g.dzw = L.g.zxdy = L.g.zydx = nullptr;
    L.g.mzw = L.g.mdzw = L.g.mzxdy = L.g.mzydx = L.g.mcw = L.g.mdx = L.g.mdy = L.g.mrmask = nullptr;
    if (l == 0) {
      CHK(dmalloc(&L.g.dzw, n2 * (L.nz + 1))); CHK(dmalloc(&L.g.zxdy, n2 * L.nz)); CHK(dmalloc(&L.g.zydx, n2 * L.nz));
      CHK(dmalloc(&L.g.mzw, n2 * (L.nz + 1))); CHK(dmalloc(&L.g.mdzw, n2 * (L.nz + 1))); CHK(dmalloc(&L.g.mcw, n2 * (L.nz + 1)));
      CHK(dmalloc(&L.g.mzxdy, n2 * L.nz)); CHK(dmalloc(&L.g.mzydx, n2 * L.nz));
      CHK(dmalloc(&L.g.mdx, n2)); CHK(dmalloc(&L.g.mdy, n2)); CHK(dmalloc(&L.g.mrmask, n2));
    }
    if (L.gather) {
      const int nxc = L.nx / L.ngx, nyc = L.ny / L.ngy;
      L.vs = L.v;
      make_view(L.vs, nxc, nyc, L.nz);
      const size_t ns = (size_t)(nxc + 2) * L.vs.plane;
      CHK(dmalloc(&L.vs.b, ns)); CHK(dmalloc(&L.vs.p, ns));
      const size_t Ng = (size_t)L.nz * (nyc + 2) * (nxc + 2);
      CHK(dmalloc(&L.blk, Ng)); CHK(dmalloc(&L.gbuf, Ng * L.ngroup));
      const size_t Nd = (size_t)(L.nz + 1) * nyc * nxc;   // the interior block of zw (mgx_matrices_depths*)
      CHK(dmalloc(&L.dblk, Nd)); CHK(dmalloc(&L.dgbuf, Nd * L.ngroup));
      for (int q = 0; q < 4; q++) CHK(dmalloc(&L.tmp2[q], (size_t)(nyc + 2) * (nxc + 2)));
    }
    size_t np = (size_t)mgxk_residual_nblocks(&L.v);
    if (l == 1) {  // the fused closing residual of solve_p, of a halving or of a held pair
      const size_t nf = (size_t)(held_pair(S.lev[0], L) ? mgxk_residual_restrict_held_grid(&S.lev[0].v, &L.v) : mgxk_residual_restrict_grid(&S.lev[0].v, &L.v));
      if (nf > np) np = nf;
    }
    if (np > max_part) max_part = np;
  }
  S.npartial = (int)max_part;
  CHK(dmalloc(&S.d_partial, 2 * max_part));  // the residual norms leave a pair per workgroup (dd_add, mgx_device.h)
  CHK(dmalloc(&S.d_scalar, 8));
  if (S.method == M_RB && S.real) CHK(dmalloc(&S.rho_dev, 32));
  HIPCHK(hipHostMalloc((void **)&S.h_scalar, 8 * sizeof(double)));
  HIPCHK(hipHostMalloc((void **)&S.kerr, 64, hipHostMallocMapped));
  *S.kerr = 0;
  if (S.nranks > 1) {
    HIPCHK(hipStreamCreateWithFlags(&S.stream2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&S.ev_a, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&S.ev_s, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&S.ev_x, hipEventDisableTiming));
  }
  Level &L1 = S.lev[0];
  S.ref_scratch_n = (size_t)8 * L1.nz * (L1.ny + 2) * (L1.nx + 2);
  CHK(dmalloc(&S.ref_scratch, S.ref_scratch_n));
  CHK(dmalloc(&S.slope_scratch, S.ref_scratch_n / 4));  // 2 x level-1 field: the slopes zy, zx in the reference layout
  for (auto &L : S.lev) { L.g.cA = S.ref_scratch; L.g.szy = S.slope_scratch; L.g.szx = nullptr; }
  S.xbuf_n = (size_t)(L1.nz + 1) * 2 * ((L1.nx > L1.ny ? L1.nx : L1.ny) + 4);
  if (S.par.bmask && S.nranks > 1) {  // the 4-D cA halo of define_matrix travels through the same buffers
    const size_t n4 = (size_t)8 * L1.nz * (L1.nx > L1.ny ? L1.nx : L1.ny);
    if (n4 > S.xbuf_n) S.xbuf_n = n4;
  }
  for (int q = 0; q < 16; q++) CHK(dmalloc(&S.xbuf[q], S.xbuf_n));
  CHK(dmalloc(&S.d_u, (size_t)(L1.nx + 1) * (L1.ny + 2) * L1.nz));
  CHK(dmalloc(&S.d_v, (size_t)(L1.nx + 2) * (L1.ny + 1) * L1.nz));
  CHK(dmalloc(&S.d_w, (size_t)(L1.nx + 2) * (L1.ny + 2) * (L1.nz + 1)));
  CHK(dmalloc(&S.d_fx, (size_t)(L1.nx + 2) * (L1.ny + 2) * (L1.nz + 1)));
  CHK(dmalloc(&S.d_fy, (size_t)(L1.nx + 2) * (L1.ny + 2) * (L1.nz + 1)));
  CHK(dmalloc(&S.d_fz, (size_t)(L1.nx + 2) * (L1.ny + 2) * (L1.nz + 1)));
  CHK(dmalloc(&S.d_bm, (size_t)(L1.nx + 2) * (L1.ny + 2) * L1.nz));
  CHK(dmalloc(&S.d_rmask_ref, (size_t)(L1.nx + 2) * (L1.ny + 2))); CHK(dmalloc(&S.d_rmask_m, (size_t)(L1.nx + 2) * (L1.ny + 2)));
  S.call_mask = false;
  CHK(sync_stream());
  S.use_small = getenv("MGX_NO_SMALL") ? 0 : 1;
  S.no_mf = getenv("MGX_NO_MF") ? 1 : 0;
  options_from_env();
  if (getenv("MGX_P2P_TIMEOUT_MS")) (void)mgxk_set_p2p_timeout(atof(getenv("MGX_P2P_TIMEOUT_MS")));
  S.inited = true;
  if (S.verbose && S.rank == 0) {  // read_nhnamelist prints (mg_namelist.f90:108-124) and print_grids (mg_grids.f90:741-762)
    printf(" Non hydrostatic parameters:\n   - solver_prec   : %g\n   - solver_maxiter: %d\n   - nsmall        : %d\n   - ns_coarsest   : %d\n"
           "   - ns_pre        : %d\n   - ns_post       : %d\n   - cmatrix       : %s\n   - relax_method  : %s\n   - interp_type   : %s\n"
           "   - restrict_type : %s\n   - aggressive    : %c\n   - netcdf_output : %c\n   - bmask         : %c\n\n",
           p.solver_prec, p.solver_maxiter, p.nsmall, p.ns_coarsest, p.ns_pre, p.ns_post, p.cmatrix, p.relax_method, p.interp_type,
           p.restrict_type, p.aggressive ? 'T' : 'F', p.netcdf_output ? 'T' : 'F', p.bmask ? 'T' : 'F');
    printf(" - print grid information:\n");
    for (int l = 0; l < S.nlevs; l++) {
      const Level &L = S.lev[l];
      printf("  lev=%2d: %3d x%3d x%3d on %3d x%3d procs%s\n", l + 1, L.nx, L.ny, L.nz, L.npx, L.npy, L.gather ? " / gather" : "");
    }
  }
  return 0;
}

}  // extern "C"
