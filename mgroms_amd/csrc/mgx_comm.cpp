// Host side of libmgx.so, the transports: halo fills of the solver fields and of the set-up arrays, the all-reduce behind global_sum,
// the stream synchronisation that reports what the device flagged, and the entry points of the two optional transports
// (peer-to-peer pushes over hipIpc-shared buffers: mgx_p2p_*; the library's own RCCL communicator: mgx_rccl_*, mgx_rccl.cpp).
#include "mgx_host.h"

// a HIP error that was pending when a kernel wrapper started (mgx_before_launch, mgx_device.h): reported by the next synchronising call
thread_local hipError_t mgx_pending_error = hipSuccess;

namespace mgx_host {

// ---- halo exchange buffers ---------------------------------------------------------------------------
// The entry list of one exchange, from the neighbour table of the level (0 S, 1 E, 2 N, 3 W, 4 SW, 5 SE, 6 NE, 7 NW; -1 = no neighbour).  Pure.
// Every transport behind mgx_set_comm matches the messages of one pair of ranks in list order, and with option "periodic" on a process grid one rank
// can be the neighbour on several sides at once (two ranks along a periodic direction: east and west; one rank along it: S, SW and SE; a doubly
// periodic 2 x 2 grid: all four corners).  So for each peer the sends go in ascending direction d, and the receive slots in ascending order of the
// SENDER's direction opp(e): the k-th message a peer sends is the one this rank expects k-th, and what was packed for d lands in slot opp(d) over
// there.  Entries are listed by ascending send direction, which for distinct peers is the plain direction order.  A direction whose peer is the
// rank itself is not an entry: its bit is set in *self_mask (exchange() serves it by a device copy).  The two directions of an entry are of one kind
// (S/N edge, E/W edge, corner), so one count serves both.  Returns the number of entries, -1 for a table no decomposition produces.
int exchange_plan(const int *neighb, int rank, XEntry *out, int *self_mask) {
  static const int opp[8] = {2, 3, 0, 1, 6, 7, 4, 5};
  auto kind = [](int d) { return d >= 4 ? 2 : (d & 1); };
  int n = 0, self = 0;
  for (int d = 0; d < 8; d++) {
    if (neighb[d] < 0) continue;
    if (neighb[d] == rank) { self |= 1 << d; continue; }
    // the receive slot: among the slots of this peer, the one whose sender's direction has the rank this send has among the sends to the peer
    int k = 0, rd = -1;
    for (int t = 0; t < d; t++) k += neighb[t] == neighb[d];
    for (int f = 0; f < 8 && rd < 0; f++) {   // f = opp(e) ascending
      const int e = opp[f];
      if (neighb[e] != neighb[d]) continue;
      if (k-- == 0) rd = e;
    }
    if (rd < 0 || kind(rd) != kind(d)) return -1;
    out[n].peer = neighb[d]; out[n].sd = d; out[n].rd = rd; n++;
  }
  for (int d = 0; d < 8; d++) if ((self >> d & 1) && !(self >> opp[d] & 1)) return -1;   // a wrap has both of its ends here
  if (self_mask) *self_mask = self;
  return n;
}

// dir[q] = the direction entry q was packed for: sb[q] holds what the neighbour in that direction needs, rb[q] is where the halo of that side is
// unpacked from.  The entries go through exchange_plan(): a peer that is the rank itself (option "periodic", one rank along the direction) is served
// here, without hooks -- what was packed for direction d is what the neighbour in direction d receives from its opposite side, so it goes into the
// receive buffer of the entry of direction opp(d), by a device copy on the solver's stream; the others are handed to the hook in the plan's order.
// dir == nullptr (the self-test of the native transport): the list as given.
int exchange(int n, const int *peer, double *const *sb, double *const *rb, const int *cnt, const int *dir) {
  if (!dir) {
    if (S.periodic && S.nranks == 1 && n > 0) return fail("exchange: a local wrap (option \"periodic\") needs the directions of its entries");
    if (!S.ex) return fail("a halo exchange is needed (npx*npy > 1) but mgx_set_comm was not called");
    S.n_exch++;
    if (S.ex(S.ctx, n, peer, sb, rb, cnt)) return fail("exchange callback failed%s%s", S.native_rccl ? ": " : "", S.native_rccl ? mgxr_last_error() : "");
    return 0;
  }
  static const int opp[8] = {2, 3, 0, 1, 6, 7, 4, 5};
  int nbv[8], qof[8], self = 0;
  for (int d = 0; d < 8; d++) nbv[d] = qof[d] = -1;
  for (int q = 0; q < n; q++) {
    if (dir[q] < 0 || dir[q] > 7 || qof[dir[q]] >= 0 || peer[q] < 0) return fail("exchange: entry %d names direction %d", q, dir[q]);
    nbv[dir[q]] = peer[q]; qof[dir[q]] = q;
  }
  XEntry pl[8];
  const int nh = exchange_plan(nbv, S.rank, pl, &self);
  if (nh < 0) return fail("exchange: the entries of rank %d have no matching order (a wrap without its opposite side, or one peer on sides of two kinds)", S.rank);
  if (nh && !S.ex) return fail("a halo exchange is needed (npx*npy > 1) but mgx_set_comm was not called");
  if (n > 0) S.n_exch++;
  for (int d = 0; d < 8; d++) {
    if (!(self >> d & 1)) continue;
    const int q = qof[d], q2 = qof[opp[d]];
    if (cnt[q2] != cnt[q]) return fail("exchange: direction %d of a local wrap (option \"periodic\") has no opposite entry of its size", d);
    HIPCHK(hipMemcpyAsync(rb[q2], sb[q], (size_t)cnt[q] * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
  }
  if (!nh) return 0;
  int hp[8], hc[8]; double *hs[8], *hr[8];
  for (int t = 0; t < nh; t++) {
    const int qs = qof[pl[t].sd], qr = qof[pl[t].rd];
    if (cnt[qs] != cnt[qr]) return fail("exchange: directions %d and %d of peer %d differ in size", pl[t].sd, pl[t].rd, pl[t].peer);
    hp[t] = pl[t].peer; hc[t] = cnt[qs]; hs[t] = sb[qs]; hr[t] = rb[qr];
  }
  if (S.ex(S.ctx, nh, hp, hs, hr, hc)) return fail("exchange callback failed%s%s", S.native_rccl ? ": " : "", S.native_rccl ? mgxr_last_error() : "");
  return 0;
}

// the three hooks of mgx_set_comm served by the library's own RCCL communicator (mgx_rccl_connect), on the solver's stream
int rccl_exchange_hook(void *, int n, const int *peer, double *const *sb, double *const *rb, const int *cnt) { return mgxr_exchange(S.stream, n, peer, sb, rb, cnt); }
int rccl_allreduce_hook(void *, double *buf, int n) { return mgxr_allreduce(S.stream, buf, n); }
int rccl_allgather_hook(void *, const int *group, int ng, const double *sb, double *rb, int cnt) { return mgxr_allgather(S.stream, group, ng, sb, rb, cnt); }

// fill_halo_3D_relax / fill_halo_3D for the JS fields p,b,r (nh = 1): mg_mpi_exchange.f90:396-745
// xonly: fill_halo_4D's rule (mg_mpi_exchange.f90:1247-1534): nothing but the exchange with existing neighbours
int fill_halo_js(Level &L, double *a, bool phys_done, bool xonly) {
  S.n_halo++;
  const int *nb = L.neighb;
  const Sides ph = sides_of(L);
  int np = 0, nself = 0;
  for (int d = 0; d < 8; d++) if (nb[d] >= 0) { np++; nself += nb[d] == S.rank; }
  if (np && nself == np) {  // every neighbour is the rank itself: the wrap, and with it the images of the closed sides where they are still due, in one launch
    const int closed_rule = phys_done ? 0 : 2;
    mgxk_halo_wrap(S.stream, &L.v, a, nb[1] >= 0 ? 1 : closed_rule, nb[0] >= 0 ? 1 : closed_rule); S.n_launch++;
    return 0;
  }
  // A mixed level (option "periodic" on a strip of ranks: the wrap is local in one direction, the other has real peers): a self direction takes no
  // slab, flag or hook entry -- the kernel that unpacks copies its halo from the interior the opposite side would have packed.  On the push path the
  // images of the closed sides that are still due ride in the same launch (a mixed level has no corner between two closed sides).
  const bool push = np && S.p2p_on, fold = push && nself > 0;
  if (!phys_done && any_physical(ph) && !fold) { mgxk_halo_phys(S.stream, &L.v, a, ph); S.n_launch++; }
  int n = 0, peer[8], cnt[8], present[8], dr[8];   // present: 0 no neighbour, 1 another rank, 2 the rank itself, 3 a closed side whose image is due (HALO_* of mgx_wrappers.h)
  double *sb[8], *rb[8];
  for (int d = 0; d < 8; d++) {
    present[d] = nb[d] < 0 ? ((fold && !phys_done && d < 4) ? HALO_MIRROR : HALO_NONE) : (nb[d] == S.rank ? HALO_SELF : HALO_PEER);
    if (present[d] != HALO_PEER) continue;
    const int c = L.nz * ((d == 0 || d == 2) ? L.nx : ((d == 1 || d == 3) ? L.ny : 1));
    peer[n] = nb[d]; cnt[n] = c; sb[n] = S.xbuf[d]; rb[n] = S.xbuf[8 + d]; dr[n] = d; n++;
  }
  int m[4] = {0, 0, 0, 0};  // mixed corners SW,SE,NE,NW: 1 = copy across the physical W/E side, 2 = across S/N (:720-743)
  bool any = false;
  if (np) {
    const int side1[4] = {0, 0, 2, 2}, side2[4] = {3, 1, 1, 3};  // SW:(S,W) SE:(S,E) NE:(N,E) NW:(N,W)
    for (int c = 0; c < 4; c++) {
      if (nb[4 + c] < 0) { if (nb[side1[c]] >= 0) m[c] = 1; else if (nb[side2[c]] >= 0) m[c] = 2; }
      if (xonly) m[c] = 0;
      any |= m[c] != 0;
    }
  }
  if (push) {  // push into the neighbours' receive buffers over xGMI, then wait on the local flags: no host step
    static const int opp[8] = {2, 3, 0, 1, 6, 7, 4, 5};
    const unsigned long long seq = ++L.p2p_seq;
    const int par = (int)(seq & 1), li = (int)(&L - &S.lev[0]);
    double *rbuf[8], *lbuf[8];
    unsigned long long *rflag[8], *lflag[8];
    for (int d = 0; d < 8; d++) {
      rbuf[d] = lbuf[d] = nullptr; rflag[d] = lflag[d] = nullptr;
      if (present[d] != HALO_PEER) continue;
      rbuf[d] = S.peer_slab[nb[d]] + L.p2p_off[opp[d]][par];
      rflag[d] = S.peer_flags[nb[d]] + (li * 8 + opp[d]) * 2 + par;
      lbuf[d] = S.p2p_slab + L.p2p_off[d][par];
      lflag[d] = S.p2p_flags + (li * 8 + d) * 2 + par;
    }
    int drop = 0;
    if (S.p2p_test_drop > 0 && --S.p2p_test_drop == 0) drop = 1;
    mgxk_halo_p2p(S.stream, &L.v, a, rbuf, lbuf, rflag, lflag, present, seq, S.p2p_counter, S.p2p_err, m, drop);  // push, wait, unpack, mixed corners
    S.n_launch++; S.n_p2p++;
  } else if (np) {
    mgxk_halo_pack_all(S.stream, &L.v, a, S.xbuf, present, 0); S.n_launch++;       // all edges + corners, one launch
    CHK(exchange(n, peer, sb, rb, cnt, dr));
    mgxk_halo_pack_all(S.stream, &L.v, a, S.xbuf + 8, present, 1); S.n_launch++;
    if (any) { mgxk_halo_mixed_corners(S.stream, &L.v, a, m[0], m[1], m[2], m[3]); S.n_launch++; }
  }
  return 0;
}

// generic halo fill of a reference-layout array a(nzz,1-nh:ny+nh,1-nh:nx+nh); lbc = 0,'u','v'
// (mg_mpi_exchange.f90:23-352 2D, :750-1242 3D incl. nh=2 extrapolation and lbc_null)
void rect(double *a, double *buf, int op, int nzz, int nh, int ny, int j0, int j1, int i0, int i1, int mj, int cj, int mi,
          int ci, int mj2, int cj2, int mi2, int ci2) {
  RectOp R = {op, nzz, nh, ny, j0, j1, i0, i1, mj, cj, mi, ci, mj2, cj2, mi2, ci2};
  mgxs_rect(S.stream, a, buf, &R);
  S.n_launch++;
}

// xonly = fill_halo_4D (mg_mpi_exchange.f90:1245-1552): only the exchange with existing neighbours
int rl_fill_halo(Level &L, double *a, int nzz, int nh, char c, bool xonly) {
  S.n_halo++;
  const int nx = L.nx, ny = L.ny;
  const int *nb = L.neighb;
  const int So = nb[0], E = nb[1], N = nb[2], W = nb[3], SW = nb[4], SE = nb[5], NE = nb[6], NW = nb[7];
  const bool zSW = (c == 'u' && W < 0), zSE = (c == 'u' && E < 0), zNE = (c == 'u' && E < 0) || c == 'v', zNW = (c == 'u' && W < 0) || c == 'v';
  if (!xonly && c == 0 && So < 0 && E < 0 && N < 0 && W < 0 && (nh == 1 || nh == 2) && nx >= 2 && ny >= 2) {
    // no neighbour at all: every halo cell is an image (or, nh = 2, an extrapolation) of interior cells -- one launch for all sides and corners
    mgxs_halo_ref_closed(S.stream, a, nzz, nh, ny, nx); S.n_launch++;
    return 0;
  }
  if (!xonly) {
  // phase 1: physical sides, in the reference's order S,E,N,W then the corners
  if (So < 0) {
    if (c == 'v') rect(a, 0, 2, nzz, nh, ny, 1, 1, 1 - nh, nx + nh);
    else { rect(a, 0, 0, nzz, nh, ny, 0, 0, 1, nx, 0, 1, 0, 0); if (nh == 2) rect(a, 0, 1, nzz, nh, ny, -1, -1, 1, nx, 0, 2, 0, 0, 0, 3, 0, 0); }
  }
  if (E < 0) {
    if (c == 'u') rect(a, 0, 2, nzz, nh, ny, 1 - nh, ny + nh, nx + 1, nx + 1);
    else { rect(a, 0, 0, nzz, nh, ny, 1, ny, nx + 1, nx + 1, 0, 0, 0, -1); if (nh == 2) rect(a, 0, 1, nzz, nh, ny, 1, ny, nx + 2, nx + 2, 0, 0, 0, -2, 0, 0, 0, -3); }
  }
  if (N < 0) {
    if (c == 'v') rect(a, 0, 2, nzz, nh, ny, ny + 1, ny + 1, 1 - nh, nx + nh);
    else { rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + 1, 1, nx, 0, -1, 0, 0); if (nh == 2) rect(a, 0, 1, nzz, nh, ny, ny + 2, ny + 2, 1, nx, 0, -2, 0, 0, 0, -3, 0, 0); }
  }
  if (W < 0) {
    if (c == 'u') rect(a, 0, 2, nzz, nh, ny, 1 - nh, ny + nh, 1, 1);
    else { rect(a, 0, 0, nzz, nh, ny, 1, ny, 0, 0, 0, 0, 0, 1); if (nh == 2) rect(a, 0, 1, nzz, nh, ny, 1, ny, -1, -1, 0, 0, 0, 2, 0, 0, 0, 3); }
  }
  if (SW < 0) { if (zSW) rect(a, 0, 2, nzz, nh, ny, 1 - nh, 0, 1 - nh, 0); else if (So < 0 && W < 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, 1 - nh, 0, 1, 1, 1, 1); }
  if (SE < 0) { if (zSE) rect(a, 0, 2, nzz, nh, ny, 1 - nh, 0, nx + 1, nx + nh); else if (So < 0 && E < 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, nx + 1, nx + nh, 1, 1, 1, 2 * nx + 1); }
  if (NE < 0) { if (zNE) rect(a, 0, 2, nzz, nh, ny, ny + 1, ny + nh, nx + 1, nx + nh); else if (N < 0 && E < 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, nx + 1, nx + nh, 1, 2 * ny + 1, 1, 2 * nx + 1); }
  if (NW < 0) { if (zNW) rect(a, 0, 2, nzz, nh, ny, ny + 1, ny + nh, 1 - nh, 0); else if (N < 0 && W < 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, 1 - nh, 0, 1, 2 * ny + 1, 1, 1); }
  }
  // phase 2: exchange with the existing neighbours
  int n = 0, peer[8], cnt[8], dr[8];
  double *sb[8], *rb[8];
  int rr[8][4];
  for (int d = 0; d < 8; d++) {
    if (nb[d] < 0) continue;
    int sj0, sj1, si0, si1, rj0, rj1, ri0, ri1;
    const bool south = (d == 0 || d == 4 || d == 5), north = (d == 2 || d == 6 || d == 7);
    const bool east = (d == 1 || d == 5 || d == 6), west = (d == 3 || d == 4 || d == 7);
    if (south) { sj0 = 1; sj1 = nh; rj0 = 1 - nh; rj1 = 0; } else if (north) { sj0 = ny - nh + 1; sj1 = ny; rj0 = ny + 1; rj1 = ny + nh; } else { sj0 = rj0 = 1; sj1 = rj1 = ny; }
    if (west) { si0 = 1; si1 = nh; ri0 = 1 - nh; ri1 = 0; } else if (east) { si0 = nx - nh + 1; si1 = nx; ri0 = nx + 1; ri1 = nx + nh; } else { si0 = ri0 = 1; si1 = ri1 = nx; }
    const int count = nzz * (sj1 - sj0 + 1) * (si1 - si0 + 1);
    if ((size_t)count > S.xbuf_n) return fail("halo buffer too small");
    rect(a, S.xbuf[d], 3, nzz, nh, ny, sj0, sj1, si0, si1);
    peer[n] = nb[d]; cnt[n] = count; sb[n] = S.xbuf[d]; rb[n] = S.xbuf[8 + d]; dr[n] = d;
    rr[n][0] = rj0; rr[n][1] = rj1; rr[n][2] = ri0; rr[n][3] = ri1; n++;
  }
  if (n) {
    CHK(exchange(n, peer, sb, rb, cnt, dr));
    for (int q = 0; q < n; q++) rect(a, rb[q], 4, nzz, nh, ny, rr[q][0], rr[q][1], rr[q][2], rr[q][3]);
  }
  if (xonly) return 0;
  // phase 3: mixed corners (:1216-1240)
  if (SW < 0 && !zSW) { if (So >= 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, 1 - nh, 0, 0, 0, 1, 1); else if (W >= 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, 1 - nh, 0, 1, 1, 0, 0); }
  if (SE < 0 && !zSE) { if (So >= 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, nx + 1, nx + nh, 0, 0, 1, 2 * nx + 1); else if (E >= 0) rect(a, 0, 0, nzz, nh, ny, 1 - nh, 0, nx + 1, nx + nh, 1, 1, 0, 0); }
  if (NE < 0 && !zNE) { if (N >= 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, nx + 1, nx + nh, 0, 0, 1, 2 * nx + 1); else if (E >= 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, nx + 1, nx + nh, 1, 2 * ny + 1, 0, 0); }
  if (NW < 0 && !zNW) { if (N >= 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, 1 - nh, 0, 0, 0, 1, 1); else if (W >= 0) rect(a, 0, 0, nzz, nh, ny, ny + 1, ny + nh, 1 - nh, 0, 1, 2 * ny + 1, 0, 0); }
  return 0;
}

// global_sum (mg_mpi_exchange.f90:1555-1571) of the value in d_scalar[0]; returns it on the host
// The all-reduce doubles as the point where the ranks AGREE on the health of the peer-to-peer transport: a second value carries
// "a wait of mine timed out" (the device-side error word, read in stream order, or a time-out an earlier sync saw).  If any rank
// says so, every rank switches the pushes off, rewinds its sequence numbers and flags, and returns the same error: nobody is
// left pushing to, or waiting for, a rank that fell back alone.
int global_sum(const Level &L, double *out) {
  // The count is the same on every rank of a multi-rank job whatever this rank's transport state (a rank whose hipIpc mapping failed keeps
  // running on the hooks while its neighbours may have connected: a count chosen from the rank-local p2p_ready would mismatch): always two
  // values, the second one 0 from a rank without pushes.
  const bool agree = S.nranks > 1;
  if (S.nranks > 1) {
    if (!S.ar) return fail("an all-reduce is needed (npx*npy > 1) but mgx_set_comm was not called");
    S.n_allred++;
    if (S.p2p_ready && S.p2p_err) { mgxk_err_to_double(S.stream, S.p2p_err, S.p2p_failed, S.d_scalar + 1); S.n_launch++; }
    else HIPCHK(hipMemsetAsync(S.d_scalar + 1, 0, sizeof(double), S.stream));
    if (S.ar(S.ctx, S.d_scalar, 2)) return fail("allreduce callback failed");
  }
  HIPCHK(hipMemcpyAsync(S.h_scalar, S.d_scalar, 2 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  CHK(sync_stream());
  if (agree && S.h_scalar[1] > 0.0) {
    S.p2p_on = false; S.p2p_failed = 0;
    if (S.p2p_err) *S.p2p_err = 0;
    for (auto &Lv : S.lev) { Lv.p2p_seq = 0; Lv.p2p_gseq = 0; }
    if (S.p2p_flags) HIPCHK(hipMemsetAsync(S.p2p_flags, 0, 4096 * sizeof(unsigned long long), S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    return fail("the peer-to-peer halo transport timed out on %d rank(s): ALL ranks have switched to the hooks together (sequence numbers "
                "rewound); the halos of the affected exchanges were stale, so the current solve is void -- repeat it", (int)S.h_scalar[1]);
  }
  *out = S.h_scalar[0] * (L.npx * L.npy) / (S.lev[0].npx * S.lev[0].npy);
  return 0;
}

// ---- peer-to-peer halo transport: set-up / tear-down ---------------------------------------------------------
void p2p_release() {
  for (int r = 0; r < (int)S.peer_slab.size(); r++) {
    if (r == S.rank || S.p2p_borrowed) continue;
    if (S.peer_slab[r]) (void)hipIpcCloseMemHandle(S.peer_slab[r]);
    if (S.peer_flags[r]) (void)hipIpcCloseMemHandle(S.peer_flags[r]);
  }
  S.peer_slab.clear(); S.peer_flags.clear();
  if (S.p2p_slab) (void)hipFree(S.p2p_slab);
  if (S.p2p_flags) (void)hipFree(S.p2p_flags);
  if (S.p2p_counter) (void)hipFree(S.p2p_counter);
  if (S.p2p_err) (void)hipHostFree(S.p2p_err);
  S.p2p_slab = nullptr; S.p2p_flags = nullptr; S.p2p_counter = nullptr; S.p2p_err = nullptr;
  S.p2p_ready = S.p2p_on = S.p2p_borrowed = false;
}

// stream synchronise + the peer-to-peer error word (a neighbour that never raised its flag)
int sync_stream() {
  HIPCHK(hipStreamSynchronize(S.stream));
  // a kernel launch this thread issued since the last check was refused (launch configuration, LDS or register demand on this
  // device / ROCm): the operator it belonged to did not run, so the fields are not what the caller thinks -- fail loudly
  {
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && mgx_pending_error != hipSuccess) le = mgx_pending_error;
    mgx_pending_error = hipSuccess;
    if (le != hipSuccess) return fail("a HIP call of this thread failed since the last synchronisation (a rejected kernel launch, or an earlier call of the host program): %s", hipGetErrorString(le));
  }
  if (S.kerr && *S.kerr == 2) {
    // the fused sequential-order red-black launch: a forwarding wave did not see the walk's progress within 2 s, or found itself on another
    // XCD than the walk (mgx_rbseq.hip).  The correction of that colour used stale values: the fused launch is OFF from now on.
    *S.kerr = 0;
    S.rbseq_fuse = 0; S.rbseq_test_stall = 0;
    return fail("the fused red-black walk + correction launch lost its hand-off (forwarding waves timed out or ran on another XCD than the walk); "
                "the fields of that level are wrong -- it is now OFF (option rbseq_fuse = 0: the correction in a launch of its own)");
  }
  if (S.kerr && *S.kerr) {
    // a workgroup of the persistent relax kernel waited 2 s for its neighbour plane: some of its workgroups were kept off the chip
    // (the GPU is shared with kernels that do not finish).  The sweep is incomplete: counters back to zero, the separate launches from now on.
    *S.kerr = 0;
    for (auto &L : S.lev) { if (L.ksp_done) (void)hipMemsetAsync(L.ksp_done, 0, (size_t)(L.nx + 2) * sizeof(unsigned int), S.stream); L.ksp_seq = 0; }
    S.ksp_down = 1;
    return fail("the persistent relax kernel timed out waiting for a neighbouring plane (its workgroups were not all resident); "
                "the fields of that level are incomplete -- it is now OFF (one launch per colour pair)");
  }
  if (S.p2p_err && *S.p2p_err) {
    // A wait on a neighbour's flag timed out (the edge it was waiting for stayed stale).  This rank must NOT fall back alone -- its
    // neighbours would go on pushing to flags nobody reads and waiting for pushes that never come: it keeps exchanging (the
    // sequence numbers stay in step, flags are compared with >=) and remembers; the ranks agree at the next global_sum (every
    // solve_p iteration, every norm), where all of them switch to the hooks together and report the error.
    *S.p2p_err = 0;
    S.p2p_failed = 1;
    if (S.verbose) fprintf(stderr, "mgx warning: rank %d: a peer-to-peer halo wait timed out; reported collectively at the next norm\n", S.rank);
  }
  return 0;
}

// end of a cycle / operator entry point: wait for the stream (and report what the device flagged), unless the caller asked for asynchronous
// operators (option "async"): then the work is only enqueued, as a GPU-resident model would want, and mgx_synchronize reports later
int op_sync() { return S.async_ops ? 0 : sync_stream(); }

// A level-1 halo fill of a rank-coded field through the CURRENT neighbour transport (the hooks, or the pushes when they are on), all
// eight directions: every halo cell must hold the value its owner encoded (mg_testhalo.f90:75-92 with positions, not just ranks).
// Collective.  Leaves level-1 p zeroed.
int halo_rank_coded_check(const char *who) {
  Level &L = S.lev[0];
  const int nx = L.nx, ny = L.ny, nz = L.nz;
  const size_t n3 = (size_t)nz * (ny + 2) * (nx + 2);
  std::vector<double> h(n3, -1.0);
  auto at = [&](int k, int j, int i) -> size_t { return (size_t)k + (size_t)nz * ((size_t)j + (size_t)(ny + 2) * i); };
  auto code = [&](int r, int k, int j, int i) { return 1.0e7 * (r + 1) + (double)at(k, j, i); };
  for (int i = 1; i <= nx; i++) for (int j = 1; j <= ny; j++) for (int k = 0; k < nz; k++) h[at(k, j, i)] = code(S.rank, k, j, i);
  HIPCHK(hipMemcpyAsync(S.ref_scratch, h.data(), n3 * sizeof(double), hipMemcpyHostToDevice, S.stream));
  mgxk_convert(S.stream, &L.v, L.v.p, S.ref_scratch, 1, 0, 0);
  CHK(fill_halo_js(L, L.v.p));
  mgxk_convert(S.stream, &L.v, L.v.p, S.ref_scratch, 1, 0, 1);
  HIPCHK(hipMemcpyAsync(h.data(), S.ref_scratch, n3 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  CHK(sync_stream());
  HIPCHK(hipMemsetAsync(L.v.p, 0, L.n3js * sizeof(double), S.stream));
  const int *nb = L.neighb;
  // halo cell (j,i) of direction d is the owner's cell (js,is): S,E,N,W,SW,SE,NE,NW
  for (int d = 0; d < 8; d++) {
    if (nb[d] < 0) continue;
    const bool south = (d == 0 || d == 4 || d == 5), north = (d == 2 || d == 6 || d == 7), east = (d == 1 || d == 5 || d == 6), west = (d == 3 || d == 4 || d == 7);
    const int j0 = south ? 0 : (north ? ny + 1 : 1), j1 = south ? 0 : (north ? ny + 1 : ny);
    const int i0 = west ? 0 : (east ? nx + 1 : 1), i1 = west ? 0 : (east ? nx + 1 : nx);
    for (int i = i0; i <= i1; i++) for (int j = j0; j <= j1; j++) for (int k = 0; k < nz; k++) {
      const int js = south ? ny : (north ? 1 : j), is = west ? nx : (east ? 1 : i);
      if (h[at(k, j, i)] != code(nb[d], k, js, is)) return fail("%s: halo cell (k=%d,j=%d,i=%d) of direction %d does not hold rank %d's value", who, k + 1, j, i, d, nb[d]);
    }
  }
  return 0;
}

}  // namespace mgx_host
using namespace mgx_host;

extern "C" {

// ---- native RCCL transport -------------------------------------------------------------------------------------
int mgx_rccl_unique_id_bytes(void) { return 128; }
int mgx_rccl_get_unique_id(void *id_out) { if (mgxr_get_unique_id(id_out)) return fail("mgx_rccl_get_unique_id: %s", mgxr_last_error()); return 0; }
int mgx_rccl_connect(const void *id, int nranks, int rank) {
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail("mgx_rccl_connect: rank %d of %d", rank, nranks);
  if (mgxr_connect(id, nranks, rank)) return fail("mgx_rccl_connect: %s", mgxr_last_error());
  S.ex = rccl_exchange_hook; S.ar = rccl_allreduce_hook; S.ag = rccl_allgather_hook; S.ctx = nullptr; S.native_rccl = true;
  return 0;
}
int mgx_rccl_disconnect(void) {
  if (S.native_rccl) { S.ex = nullptr; S.ar = nullptr; S.ag = nullptr; S.native_rccl = false; }
  mgxr_disconnect();
  return 0;
}
// Collective self-test of the native transport (any world size, after mgx_init): one grouped exchange of rank-coded buffers with the
// next and the previous rank (with itself on one rank), an all-reduce of rank+1, an all-gather inside groups of up to four ranks and a
// level-1 halo fill of a position-coded field over all eight neighbour directions -- through the same hooks the solver uses.
// 0 = every value arrived.  Level-1 p is zero afterwards.
int mgx_rccl_selftest(void) {
  NEED_INIT();
  if (!S.native_rccl || !mgxr_connected()) return fail("mgx_rccl_selftest: the native RCCL transport is not connected");
  const int n = mgxr_nranks(), me = S.rank;
  if (n != S.nranks) return fail("mgx_rccl_selftest: communicator has %d ranks, the solver %d", n, S.nranks);
  const int cnt = (int)std::min<size_t>(1000, S.xbuf_n);
  int peers[2], np = 0;
  peers[np++] = (me + 1) % n;
  if ((me - 1 + n) % n != peers[0]) peers[np++] = (me - 1 + n) % n;
  std::vector<double> h(cnt);
  double *sb[2], *rb[2]; int cn[2];
  for (int q = 0; q < np; q++) {
    for (int t = 0; t < cnt; t++) h[t] = 1000.0 * me + peers[q] + 1e-3 * t;
    HIPCHK(hipMemcpyAsync(S.xbuf[q], h.data(), cnt * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    HIPCHK(hipMemsetAsync(S.xbuf[8 + q], 0, cnt * sizeof(double), S.stream));
    sb[q] = S.xbuf[q]; rb[q] = S.xbuf[8 + q]; cn[q] = cnt;
  }
  CHK(exchange(np, peers, sb, rb, cn));
  for (int q = 0; q < np; q++) {
    HIPCHK(hipMemcpyAsync(h.data(), S.xbuf[8 + q], cnt * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    CHK(sync_stream());
    for (int t = 0; t < cnt; t++) if (h[t] != 1000.0 * peers[q] + me + 1e-3 * t) return fail("mgx_rccl_selftest: wrong data from rank %d (element %d)", peers[q], t);
  }
  S.h_scalar[0] = me + 1.0;
  HIPCHK(hipMemcpyAsync(S.d_scalar, S.h_scalar, sizeof(double), hipMemcpyHostToDevice, S.stream));
  if (S.ar(S.ctx, S.d_scalar, 1)) return fail("mgx_rccl_selftest: all-reduce failed: %s", mgxr_last_error());
  HIPCHK(hipMemcpyAsync(S.h_scalar, S.d_scalar, sizeof(double), hipMemcpyDeviceToHost, S.stream));
  CHK(sync_stream());
  if (S.h_scalar[0] != 0.5 * n * (n + 1)) return fail("mgx_rccl_selftest: all-reduce gave %g, expected %g", S.h_scalar[0], 0.5 * n * (n + 1));
  {  // all-gather leg (gather_3D's hook): groups of up to four consecutive ranks, the shape of the reference's colour groups
    const int g0 = me / 4 * 4, ng = std::min(4, n - g0), gc = (int)std::min<size_t>(500, S.ref_scratch_n / 8);
    int grp[4];
    for (int q = 0; q < ng; q++) grp[q] = g0 + q;
    std::vector<double> hs(gc), hr((size_t)gc * ng);
    for (int t = 0; t < gc; t++) hs[t] = 7000.0 * me + t;
    double *sb = S.ref_scratch, *rb = S.ref_scratch + gc;
    HIPCHK(hipMemcpyAsync(sb, hs.data(), gc * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipMemsetAsync(rb, 0, (size_t)gc * ng * sizeof(double), S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    if (S.ag(S.ctx, grp, ng, sb, rb, gc)) return fail("mgx_rccl_selftest: all-gather failed: %s", mgxr_last_error());
    HIPCHK(hipMemcpyAsync(hr.data(), rb, (size_t)gc * ng * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    CHK(sync_stream());
    for (int q = 0; q < ng; q++)
      for (int t = 0; t < gc; t++) if (hr[(size_t)q * gc + t] != 7000.0 * grp[q] + t) return fail("mgx_rccl_selftest: all-gather slot %d holds wrong data (element %d)", q, t);
  }
  CHK(halo_rank_coded_check("mgx_rccl_selftest"));
  return 0;
}
// which transport carries the neighbour traffic right now
const char *mgx_transport(void) {
  std::string &t = S.transport_name;
  const std::string per = S.periodic == 1 ? "i" : S.periodic == 2 ? "j" : "ij";
  if (S.nranks <= 1 && !S.native_rccl && S.periodic) t = "none (one rank; periodic " + per + ": local wrap)";
  else if (S.nranks <= 1 && !S.native_rccl) t = "none (one rank)";
  else {
    t = S.native_rccl ? std::string("RCCL, native (") + mgxr_library() + ")" : (S.ex ? "host callbacks (mgx_set_comm)" : "none");
    if (S.p2p_on) t = "peer-to-peer pushes over hipIpc-shared buffers for the cycle's halos and gathers; " + t + " for set-up halos and the norm";
    if (S.periodic) t += "; periodic " + per + ": the wrap crosses ranks like a rank seam where a level has several ranks along the direction, local wrap where it has one";
  }
  return t.c_str();
}

long long mgx_p2p_exchanges(void) { return S.n_p2p; }

int mgx_p2p_prepare(void *handles_out) {
  NEED_INIT();
  if (S.p2p_slab) return fail("mgx_p2p_prepare called twice");
  size_t off = 0;
  for (auto &L : S.lev)
    for (int d = 0; d < 8; d++) {
      const size_t c = (size_t)L.nz * ((d == 0 || d == 2) ? L.nx : ((d == 1 || d == 3) ? L.ny : 1));
      for (int par = 0; par < 2; par++) { L.p2p_off[d][par] = off; off += (c + 31) / 32 * 32; }
      L.p2p_seq = 0;
    }
  for (auto &L : S.lev) {
    L.p2p_gseq = 0; L.p2p_goff[0] = L.p2p_goff[1] = 0;
    if (!L.gather) continue;
    const size_t Ng = (size_t)L.nz * (L.vs.ny + 2) * (L.vs.nx + 2);
    for (int par = 0; par < 2; par++) { L.p2p_goff[par] = off; off += ((size_t)L.ngroup * Ng + 31) / 32 * 32; }
  }
  S.p2p_slab_n = off;
  HIPCHK(hipExtMallocWithFlags((void **)&S.p2p_slab, off * sizeof(double), hipDeviceMallocFinegrained));
  HIPCHK(hipExtMallocWithFlags((void **)&S.p2p_flags, 4096 * sizeof(unsigned long long), hipDeviceMallocFinegrained));
  HIPCHK(hipMalloc((void **)&S.p2p_counter, 64));
  HIPCHK(hipHostMalloc((void **)&S.p2p_err, 64, hipHostMallocMapped));
  *S.p2p_err = 0;
  HIPCHK(hipMemset(S.p2p_slab, 0, off * sizeof(double)));
  HIPCHK(hipMemset(S.p2p_flags, 0, 4096 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(S.p2p_counter, 0, 64));
  HIPCHK(hipDeviceSynchronize());
  hipIpcMemHandle_t h[2];
  HIPCHK(hipIpcGetMemHandle(&h[0], S.p2p_slab));
  HIPCHK(hipIpcGetMemHandle(&h[1], S.p2p_flags));
  memcpy(handles_out, h, sizeof h);
  return 0;
}

int mgx_p2p_handle_bytes(void) { return (int)(2 * sizeof(hipIpcMemHandle_t)); }

// the receive slab and the flag page of THIS instance (after mgx_p2p_prepare), for ranks that live in the same process
int mgx_p2p_local_pointers(void **slab, void **flags) {
  NEED_INIT();
  if (!S.p2p_slab) return fail("mgx_p2p_local_pointers: call mgx_p2p_prepare first");
  *slab = S.p2p_slab; *flags = S.p2p_flags;
  return 0;
}

// mgx_p2p_connect for ranks whose buffers are directly addressable (other instances of this process; memory the caller mapped
// itself): slabs[r], flags[r] = what rank r's mgx_p2p_local_pointers returned.  Nothing is opened and nothing is closed later.
int mgx_p2p_connect_pointers(void *const *slabs, void *const *flags, int nranks) {
  NEED_INIT();
  if (!S.p2p_slab) return fail("mgx_p2p_connect_pointers: call mgx_p2p_prepare first");
  if (nranks != S.nranks) return fail("mgx_p2p_connect_pointers: %d pointer pairs for %d ranks", nranks, S.nranks);
  if ((int)S.lev.size() * 16 > 1024 || (int)S.lev.size() * 8 > 3072) return fail("mgx_p2p_connect_pointers: too many levels");
  S.peer_slab.assign(nranks, nullptr); S.peer_flags.assign(nranks, nullptr);
  for (int r = 0; r < nranks; r++) { S.peer_slab[r] = (double *)slabs[r]; S.peer_flags[r] = (unsigned long long *)flags[r]; }
  S.peer_slab[S.rank] = S.p2p_slab; S.peer_flags[S.rank] = S.p2p_flags;
  for (auto &L : S.lev) {
    for (int d = 0; d < 8; d++) if (L.neighb[d] >= 0 && !S.peer_slab[L.neighb[d]]) return fail("mgx_p2p_connect_pointers: no buffers for neighbour rank %d", L.neighb[d]);
    if (L.gather) for (int q = 0; q < L.ngroup; q++) if (!S.peer_slab[L.group[q]]) return fail("mgx_p2p_connect_pointers: no buffers for group member %d", L.group[q]);
  }
  S.p2p_borrowed = true;
  S.p2p_ready = true; S.p2p_on = true;
  return 0;
}

int mgx_p2p_connect(const void *all_handles, int nranks) {
  NEED_INIT();
  if (!S.p2p_slab) return fail("mgx_p2p_connect: call mgx_p2p_prepare first");
  if (nranks != S.nranks) return fail("mgx_p2p_connect: %d handle sets for %d ranks", nranks, S.nranks);
  if ((int)S.lev.size() * 16 > 1024 || (int)S.lev.size() * 8 > 3072) return fail("mgx_p2p_connect: too many levels");
  // test hook: this rank behaves as if hipIpcOpenMemHandle had refused (a rank that fails alone while its neighbours connect)
  if (getenv("MGX_P2P_TEST_FAIL_CONNECT") && atoi(getenv("MGX_P2P_TEST_FAIL_CONNECT")) == S.rank) return fail("mgx_p2p_connect: refused on rank %d (test hook MGX_P2P_TEST_FAIL_CONNECT)", S.rank);
  S.peer_slab.assign(nranks, nullptr); S.peer_flags.assign(nranks, nullptr);
  S.peer_slab[S.rank] = S.p2p_slab; S.peer_flags[S.rank] = S.p2p_flags;
  std::vector<char> need(nranks, 0);  // only the ranks that are a neighbour on some level are opened
  for (auto &L : S.lev) {
    for (int d = 0; d < 8; d++) if (L.neighb[d] >= 0) need[L.neighb[d]] = 1;
    if (L.gather) for (int q = 0; q < L.ngroup; q++) need[L.group[q]] = 1;
  }
  const hipIpcMemHandle_t *h = (const hipIpcMemHandle_t *)all_handles;
  for (int r = 0; r < nranks; r++) {
    if (r == S.rank || !need[r]) continue;
    void *p = nullptr, *f = nullptr;
    if (hipIpcOpenMemHandle(&p, h[2 * r], hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return fail("hipIpcOpenMemHandle(slab of rank %d) failed", r); }
    S.peer_slab[r] = (double *)p;
    if (hipIpcOpenMemHandle(&f, h[2 * r + 1], hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return fail("hipIpcOpenMemHandle(flags of rank %d) failed", r); }
    S.peer_flags[r] = (unsigned long long *)f;
  }
  S.p2p_ready = true; S.p2p_on = true;
  return 0;
}

}  // extern "C"
