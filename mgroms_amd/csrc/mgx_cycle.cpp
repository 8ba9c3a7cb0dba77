// Host side of libmgx.so, cycle control: the tictoc timers, the operators (relax, residual, fine2coarse, coarse2fine), the V- and
// F-cycle and the three solve_p drivers (fp64 cycles, fp32 cycles under fp64 refinement, Krylov-accelerated).  Every operator is a HIP
// kernel launch through a wrapper of mgx_wrappers.h; which kernel serves a level is decided here.
#include "mgx_host.h"

namespace mgx_host {

// ---- mg_tictoc.f90: tic(lev,name) / toc(lev,name) / print_tictoc, timed with HIP events on the solver's stream ----

int tt_sub(const char *name) {
  for (size_t q = 0; q < S.tt_names.size(); q++) if (S.tt_names[q] == name) return (int)q;
  S.tt_names.push_back(name);
  return (int)S.tt_names.size() - 1;
}
void tic(int lev, const char *name) {
  if (!S.tictoc) return;
  TicRec r; r.lev = lev; r.sub = tt_sub(name);
  if (r.sub >= 32 || lev > 32) return;
  (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, S.stream);
  S.tt_open.push_back(r);
}
void toc(int lev, const char *name) {
  if (!S.tictoc) return;
  const int sub = tt_sub(name);
  for (int q = (int)S.tt_open.size() - 1; q >= 0; q--)
    if (S.tt_open[q].lev == lev && S.tt_open[q].sub == sub) {
      (void)hipEventRecord(S.tt_open[q].e1, S.stream);
      S.tt_done.push_back(S.tt_open[q]);
      S.tt_open.erase(S.tt_open.begin() + q);
      if (lev > S.tt_nblev) S.tt_nblev = lev;
      return;
    }
}
void tt_collect() {
  if (S.tt_done.empty()) return;
  (void)hipStreamSynchronize(S.stream);
  for (auto &r : S.tt_done) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { S.tt_time[r.lev - 1][r.sub] += ms * 1e-3; S.tt_calls[r.lev - 1][r.sub]++; }
    (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
  }
  S.tt_done.clear();
}

// ---- operators ------------------------------------------------------------------------------------
// relax(): one file-local function per smoother mode; what a colour pass reports is PASS_* of mgx_wrappers.h
namespace {

// The view a colour pass of L takes: L.v as it stands at the call -- or, on a level built from the caller's depths whose pass would generate
// slots 4 / 7 from the sigma fields the level no longer has (Level::pass_stored, mgx_choice_depths.h), L.v without its slopes: the
// stored-coefficient instance of the same pass, the same bits.  The operator and the transfers of the level keep the slopes.
struct PassView {
  LevView t; const LevView *v;
  explicit PassView(const Level &L) : v(&L.v) { if (L.pass_stored) { t = L.v; t.zy = t.zx = nullptr; v = &t; } }
};

// exact lexicographic order by hyperplanes; halo fill once per sweep (mg_relax.f90:131-141)
int relax_gs(Level &L, int lev, int nsweeps) {
  for (int it = 1; it <= nsweeps; it++) {
    if (!mgxk_relax_gs_sweep(S.stream, &L.v, S.real)) return fail("relax_method='GS': the sweep of level %d could not be launched", lev);
    S.n_launch += L.ny + 2 * L.nx - 2;
    CHK(fill_halo_js(L, L.v.p));
  }
  return 0;
}

// The reference's red-black loop is sequential (mg_relax.f90:170-186): with cmatrix='real' a column of plane i reads the
// same-colour k=1 diagonals (j+-1,i-1) already updated and (j+-1,i+1) not yet (:271-276).  Columns of one colour inside a
// plane are independent, so one launch per plane, in order, reproduces the loop bit for bit -- on one rank and, with the
// halo filled after each colour as in the reference, its decomposition-dependent result on several.
int relax_rb_exact(Level &L, int nsweeps, Sides ph) {
  for (int it = 1; it <= nsweeps; it++)
    for (int rb = 1; rb <= 2; rb++) {
      int pass = 0;
      for (int i = 1; i <= L.nx; i++) { pass = mgxk_relax_colour(S.stream, PassView(L).v, i, 1, 1, -1, rb, 1, 0, ph); S.n_launch++; }
      if (pass & PASS_TALL_STORED) S.n_tall_stored++;
      CHK(fill_halo_js(L, L.v.p, pass & PASS_MIRRORS));
    }
  return 0;
}

// Sequential-order red-black, after the parallel pass of colour rb (`pass`: what it reported) has left y in p: the walk over the planes, then
// p += g s with the mirrors (mgx_rbseq.hip), by the first of window, walk-apply, fused scan, scan + apply that serves the level.
// *mirrors (in: the pass stored them) tells on return whether the physical images of every row are in place.
int rbseq_correct(Level &L, int rb, int pass, bool closed, int *mirrors) {
  const int have_d0 = (pass & PASS_D0) ? 1 : 0;
  const Sides ph = sides_of(L);
  // the windowed walk where the level's contraction bound allows it (k_rbseq_window): one launch, no hand-off, no walk over the level
  if (S.rbseq_window && L.rbs_m > 0) {
    if (!have_d0) { mgxk_rbseq_d0(S.stream, &L.v, rb); S.n_launch++; }   // (the nz = 128 colour pass does not leave it)
  }
  const int kcut = S.rbseq_rowcut ? L.rbs_rows : L.nz;
  if (S.rbseq_window && L.rbs_m > 0 && mgxk_rbseq_window(S.stream, &L.v, rb, ph, closed ? 1 : 0, L.rbs_m, kcut)) {
    // the window stores the physical images of the rows it corrects (k < kcut) only: the rows below the cut keep those of the
    // colour pass, which the generic kernel (no register instance for this nz / matrix) does not store
    S.n_launch++; S.n_window++; *mirrors = (pass & PASS_MIRRORS) || kcut >= L.nz;
    return 0;
  }
  // small levels whose pass left d0 in u1: walk and correction in one launch, every workgroup walking for itself (k_rbseq_walk_apply)
  if (have_d0 && S.rbseq_fuse && mgxk_rbseq_walk_apply(S.stream, &L.v, rb, ph, closed ? 1 : 0)) {
    S.n_launch++; *mirrors = 1;
    return 0;
  }
  // (where an instance exists the correction runs inside the walk's launch, chasing it: option "rbseq_fuse")
  const int ran = S.rbseq_fuse ? mgxk_rbseq_scan_apply(S.stream, &L.v, rb, ph, closed ? 1 : 0, have_d0, L.rbs_flag, ++L.rbs_seq, S.kerr, S.rbseq_test_stall, (long long)S.rbseq_fuse_min) : mgxk_rbseq_scan(S.stream, &L.v, rb, have_d0);
  if (ran == 2) S.rbseq_test_stall = 0;
  // a level wider than the walk takes (ny > 2048) would have to run plane by plane: refuse loudly rather than fall back to another iteration
  if (!ran) return fail("rb_seq: level %d (ny = %d) has no scan instance; set option rb_exact or rb_seq = 0", (int)(&L - S.lev.data()) + 1, L.ny);
  if (ran == 1) { mgxk_rbseq_apply(S.stream, &L.v, rb, ph, closed ? 1 : 0); S.n_launch++; }
  S.n_launch += 2 - have_d0;
  *mirrors = 1;  // the correction stores the physical images of every column it updates
  return 0;
}

// The parallel red-black pass, one colour at a time, and behind it (seq) the correction to the reference's sequential order.
int relax_rb(Level &L, int nsweeps, Sides ph, bool seq) {
  const bool closed = all_physical(ph);
  double *const p1a = L.v.p1;
  // cmatrix='real': the k=1 diagonal neighbours have the column's own colour and must be read as they were before the
  // pass (snapshot).  On a closed level the register kernels write the next sweep's snapshot themselves (two buffers
  // swapped per sweep: a pass reads only entries of its own colour, which the other colour's pass never touches), so
  // one snapshot launch per relax call suffices; with neighbours the halo part changes after every exchange.
  const bool chain = S.rb_chain && S.real && closed && mgxk_has_reg_kernel(&L.v) && !seq;
  for (int it = 1; it <= nsweeps; it++) {
    if (chain) {
      if (it == 1) { mgxk_snapshot_k1(S.stream, &L.v); S.n_launch++; }
      L.v.p1w = (L.v.p1 == p1a) ? L.p1b : p1a;
    }
    for (int rb = 1; rb <= 2; rb++) {
      // seq on a closed level: the correction keeps the snapshot current (its colour's new bottom values and their physical images), so one
      // snapshot launch per relax call; with neighbours the halo part changes with every exchange
      if (S.real && !chain && !(seq && closed && !(it == 1 && rb == 1))) { mgxk_snapshot_k1(S.stream, &L.v); S.n_launch++; }
      // (seq, wide half-rows: the pass also leaves the walk's d0 = y(k=1) - snapshot in u1 where its kernel can -- one launch less)
      L.v.d0w = (seq && S.rbseq_d0_in_pass && (mgxk_rbseq_wants_d0(&L.v) || (S.rbseq_window && L.rbs_m > 0))) ? L.v.u1 : nullptr;
      const int pass = mgxk_relax_colour(S.stream, PassView(L).v, 1, 1, L.nx, -1, rb, S.real, S.real, ph); S.n_launch++;
      L.v.d0w = nullptr;
      if (pass & PASS_TALL_STORED) S.n_tall_stored++;
      int mirrors = (pass & PASS_MIRRORS) ? 1 : 0;
      if (seq) CHK(rbseq_correct(L, rb, pass, closed, &mirrors));
      CHK(fill_halo_js(L, L.v.p, mirrors));
    }
    if (chain) { L.v.p1 = L.v.p1w; L.v.p1w = nullptr; if (it == nsweeps) L.v.p1 = p1a; }
  }
  return 0;
}

// One colour of a four-colour sweep on a level with neighbours, halos by the pushes: the boundary part of the colour (the waves that hold a
// column next to a neighbour's halo -- what the exchange sends, and all that reads what the last exchange delivered) and the exchange behind
// it go to a second stream; the interior part runs beside them on the solver's stream and waits only for the previous colour's boundary part
// (mg_relax.f90:181,224 exchange after every colour; SURVEY 7 "split boundary columns from interior, exchange while the interior runs").
int relax_fc_overlapped(Level &L, int fc1, int fc2, Sides ph) {
  Sides ps = ph;
  HIPCHK(hipEventRecord(S.ev_a, S.stream));                 // the interior of the previous colour (and whatever came before)
  HIPCHK(hipStreamWaitEvent(S.stream2, S.ev_a, 0));
  ps.part = 1;
  const int pass = mgxk_relax_colour(S.stream2, PassView(L).v, 1 + (fc1 - 1) % 2, 2, L.nx / 2, fc2 == 1 ? 1 : 0, 0, S.real, 0, ps);
  HIPCHK(hipEventRecord(S.ev_s, S.stream2));
  { hipStream_t keep = S.stream; S.stream = S.stream2; const int rc = fill_halo_js(L, L.v.p, pass & PASS_MIRRORS); S.stream = keep; if (rc) return rc; }
  ps.part = 2;
  mgxk_relax_colour(S.stream, PassView(L).v, 1 + (fc1 - 1) % 2, 2, L.nx / 2, fc2 == 1 ? 1 : 0, 0, S.real, 0, ps);
  HIPCHK(hipStreamWaitEvent(S.stream, S.ev_s, 0));          // what follows on the solver's stream reads this colour's boundary part -- not its exchange
  S.n_launch += 2; S.n_overlap++;
  if (pass & PASS_TALL_STORED) S.n_tall_stored++;
  return 0;
}

// four colours (mg_relax.f90:193-234), one launch per colour -- or per colour pair, or two beside the exchange
int relax_fc(Level &L, int nsweeps, Sides ph) {
  const bool closed = all_physical(ph);
  // (option "periodic": every level then has a periodic side, whose fill may be a local copy with no exchange to hide -- such a level takes the one-stream pass, same bits)
  const bool ov = S.overlap && S.p2p_on && S.stream2 && !closed && !S.periodic && mgxk_has_reg_kernel(&L.v);
  for (int it = 1; it <= nsweeps; it++)
    for (int fc1 = 1; fc1 <= 2; fc1++) {
      // closed mid levels: the two colours of a plane set in one launch (mgx_relax_ks.hip)
      if (closed && mgxk_relax_ks_pair(S.stream, &L.v, fc1, L.nx / 2, S.real, ph)) { S.n_launch++; continue; }
      for (int fc2 = 1; fc2 <= 2; fc2++) {
        if (ov) { CHK(relax_fc_overlapped(L, fc1, fc2, ph)); continue; }
        const int pass = mgxk_relax_colour(S.stream, PassView(L).v, 1 + (fc1 - 1) % 2, 2, L.nx / 2, fc2 == 1 ? 1 : 0, 0, S.real, 0, ph); S.n_launch++;
        if (pass & PASS_TALL_STORED) S.n_tall_stored++;
        CHK(fill_halo_js(L, L.v.p, pass & PASS_MIRRORS));
      }
    }
  if (ov && nsweeps >= 1) {  // the call ends: the solver's stream continues behind the last exchange
    HIPCHK(hipEventRecord(S.ev_x, S.stream2));
    HIPCHK(hipStreamWaitEvent(S.stream, S.ev_x, 0));
  }
  return 0;
}

}  // namespace

// mg_relax.f90:16-47 relax ; :151-190 RB ; :193-234 FC
int relax(int lev, int nsweeps) {
  Level &L = S.lev[lev - 1];
  TicScope ts(lev, S.method == M_RB ? "relax_3D_8_RB" : (S.method == M_FC ? "relax_3D_8_FC" : "relax_3D_8_GS"));  // mg_relax.f90:128,167,209
  if (S.tictoc && S.tt_done.size() > 4096) tt_collect();
  if (S.method == M_GS) return relax_gs(L, lev, nsweeps);
  const Sides ph = sides_of(L);
  const int rbm = rb_mode(L), exact = rbm == RB_EXACT;
  // sequential-order red-black (mgx_rbseq.hip); the one-workgroup kernels of the small levels run the reference's plane loop itself
  const int seq = rbm == RB_SEQ;
  // (option "small_any_nz": the instances for nz = 3, 5, 6, 7 report 2; a timed call keeps its launch per colour pass)
  if (S.use_small && nsweeps > 0) {
    const int served = mgxk_relax_small(S.stream, &L.v, nsweeps, S.method, S.real, ph, exact ? 1 : (seq ? 2 : 0), S.small_any_nz && !S.tictoc);
    if (served) { S.n_launch++; if (served == 2) S.n_small_any++; return 0; }
  }
  // closed mid levels, four colours: the whole call in one persistent launch, one workgroup per plane (mgx_relax_ks.hip: k_relax_ksp)
  if (S.method == M_FC && all_physical(ph) && S.use_ksp && !S.ksp_down && live_instances() == 1 && mgxk_relax_ks_persist(S.stream, &L.v, nsweeps, S.real, ph, L.ksp_done, L.ksp_seq, S.kerr, S.ksp_test_stall)) {
    S.ksp_test_stall = 0;
    L.ksp_seq += (unsigned int)nsweeps; S.n_launch++;
    return 0;
  }
  if (exact) return relax_rb_exact(L, nsweeps, ph);
  return S.method == M_RB ? relax_rb(L, nsweeps, ph, seq) : relax_fc(L, nsweeps, ph);
}

// mg_relax.f90:337-383 compute_residual.  res == nullptr: the caller discards the norm (mg_solvers.f90:140),
// so neither the reduction nor the all-reduce is issued.
int residual(int lev, double *res) {
  Level &L = S.lev[lev - 1];
  TicScope ts(lev, "residual_3D_8");  // mg_relax.f90:367
  const Sides ph = sides_of(L);
  mgxk_residual(S.stream, &L.v, S.d_partial, S.d_scalar, S.real, res != nullptr, ph); S.n_launch += res ? 2 : 1;
  // the kernel wrote the physical mirrors of r; the neighbour part of r's halo is never read by the cycle (restriction
  // uses interior cells only), so the exchange is deferred until someone asks for r (mgx_get_field / mgx_fill_halo)
  if (S.exact_halos) CHK(fill_halo_js(L, L.v.r, true)); else L.r_halo_stale = true;
  if (res) { double s; CHK(global_sum(L, &s)); *res = sqrt(s); }
  return 0;
}

// mg_intergrids.f90:16-72.  with_residual: the caller is the down leg of a V-cycle, which would call compute_residual(lev)
// right before and discards both the norm and r (mg_solvers.f90:138-142): residual and restriction then run as ONE kernel
// that never writes r (mgx_resrest.hip), when the level has its matrix-free slopes; otherwise the two kernels in sequence.
int fine2coarse(int lev, bool dup_r, bool with_residual) {
  Level &F = S.lev[lev - 1], &C = S.lev[lev];
  const Sides phc = sides_of(C), none = {0, 0, 0, 0};
  bool fused = false;
  // a held pair (options "hold_odd_nz", "hold_z_levels": C.nz == F.nz): the 2-D restriction row by row (mgx_hold.hip), behind the residual as a
  // launch of its own unless the fused kernel has an instance for the pair (down)
  const bool held = held_pair(F, C);
  auto restrict = [&](const LevView *Cv, double *dst, Sides ph, double *dup, double *zero) {
    if (held) mgxk_fine2coarse_held(S.stream, &F.v, Cv, dst, ph, dup, zero); else mgxk_fine2coarse(S.stream, &F.v, Cv, dst, ph, dup, zero);
    S.n_launch++;
  };
  // returns true when the fused residual+restriction kernel took the job
  auto down = [&](const LevView *Cv, double *dst, Sides ph, double *zero) -> int {
    if (!with_residual) return 0;
    if (!S.exact_halos && !S.keep_r && !dup_r) {  // keep_r: the caller wants the reference's r, which the fused kernel never writes
      TicScope ts(lev, "residual_3D_8");
      // (a held pair with an even nz -- option "hold_z_levels" -- has a kernel of its own, mgx_resrest_held.hip; one with an odd nz keeps the two launches)
      if (held) { if (S.hold_z_fuse && mgxk_residual_restrict_held(S.stream, &F.v, Cv, dst, S.real, ph, zero, nullptr, nullptr)) { S.n_launch++; S.n_hold_z_fused++; return 1; } }
      else if (mgxk_residual_restrict(S.stream, &F.v, Cv, dst, S.real, ph, zero)) { S.n_launch++; return 1; }
    }
    return residual(lev, nullptr) ? -1 : 0;
  };
  if (!C.gather) {
    // closed level: the kernel also zeroes p_c and, for Fcycle, duplicates b_c into r_c (whole arrays through the mirrors)
    fused = all_physical(phc);
    const int d = down(&C.v, C.v.b, phc, fused ? C.v.p : nullptr);
    if (d < 0) return 1;
    if (!d) restrict(&C.v, C.v.b, phc, fused && dup_r ? C.v.r : nullptr, fused ? C.v.p : nullptr);
  } else {
    const int d = down(&C.vs, C.vs.b, none, nullptr);
    if (d < 0) return 1;
    if (!d) restrict(&C.vs, C.vs.b, none, nullptr, nullptr);
    const int Ng = C.nz * (C.vs.ny + 2) * (C.vs.nx + 2);
    if (S.p2p_on) {  // gather_3D (mg_gather.f90:95-174) as pushes into the members' gather buffers
      const unsigned long long seq = ++C.p2p_gseq;
      const int par = (int)(seq & 1), li = lev;
      int me = -1;
      for (int q = 0; q < C.ngroup; q++) if (C.group[q] == S.rank) me = q;
      if (me < 0) return fail("gather: rank %d is not in its own group on level %d", S.rank, lev + 1);
      double *dst[4]; unsigned long long *rflag[4];
      for (int q = 0; q < C.ngroup; q++) {
        // my own copy stays in ordinary device memory (C.blk): stores to the fine-grained slab are uncached and slow
        dst[q] = q == me ? C.blk : S.peer_slab[C.group[q]] + C.p2p_goff[par] + (size_t)me * Ng;
        rflag[q] = S.peer_flags[C.group[q]] + 1024 + (li * 4 + me) * 2 + par;
      }
      mgxk_gather_push(S.stream, &C.vs, C.vs.b, dst, rflag, C.ngroup, me, seq, S.p2p_counter, S.p2p_err); S.n_launch++;
      for (int q = 0; q < C.ngroup; q++) {
        unsigned long long *lflag = q == me ? nullptr : S.p2p_flags + 1024 + (li * 4 + q) * 2 + par;
        mgxk_gather_place_wait(S.stream, &C.v, C.v.b, q == me ? C.blk : S.p2p_slab + C.p2p_goff[par] + (size_t)q * Ng, C.vs.nx, C.vs.ny, q % C.ngx, q / C.ngx, lflag, seq, S.p2p_err);
        S.n_launch++;
      }
      S.n_p2p++;
    } else {
      mgxk_block_to_ref(S.stream, &C.vs, C.vs.b, C.blk); S.n_launch++;
      if (!S.ag) return fail("a gather is needed but mgx_set_comm was not called");
      if (S.ag(S.ctx, C.group, C.ngroup, C.blk, C.gbuf, Ng)) return fail("allgather callback failed");
      for (int q = 0; q < C.ngroup; q++) {
        mgxk_gather_place(S.stream, &C.v, C.v.b, C.gbuf + (size_t)q * Ng, C.vs.nx, C.vs.ny, q % C.ngx, q / C.ngx); S.n_launch++;
      }
    }
  }
  // b's halo is not read by relax/residual either: physical mirrors are in place, neighbour exchange deferred
  if (S.exact_halos || C.gather) CHK(fill_halo_js(C, C.v.b, !C.gather)); else C.b_halo_stale = true;
  if (!fused) {
    HIPCHK(hipMemsetAsync(C.v.p, 0, C.n3js * sizeof(double), S.stream));
    if (dup_r) HIPCHK(hipMemcpyAsync(C.v.r, C.v.b, C.n3js * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
  }
  return 0;
}

// mg_intergrids.f90:167-228.  keep_r: also leave the interpolated correction in the fine r, as the reference does (the C-ABI operator
// and exact_halos = 1); the cycles do not -- nothing reads it before compute_residual overwrites it.
// skip1: a four-colour relax(lev, n >= 1) follows immediately -- its first colour overwrites the (i odd, j odd) columns without reading
// them, so the prolongation leaves them alone (never together with keep_r).
int coarse2fine(int lev, bool keep_r, bool skip1) {
  Level &F = S.lev[lev - 1], &C = S.lev[lev];
  const Sides phf = sides_of(F);
  // a held pair (option "hold_odd_nz"): the 2-D prolongation row by row (mgx_hold.hip)
  const auto prolong = held_pair(F, C) ? mgxk_coarse2fine_held : mgxk_coarse2fine;
  if (!C.gather) {
    prolong(S.stream, &F.v, &C.v, C.v.p, S.linear, phf, keep_r, skip1 && !keep_r); S.n_launch++;
  } else {
    mgxk_split(S.stream, &C.v, &C.vs, C.v.p, C.vs.p, C.key % 2, C.key / 2); S.n_launch++;
    prolong(S.stream, &F.v, &C.vs, C.vs.p, S.linear, phf, keep_r, skip1 && !keep_r); S.n_launch++;
  }
  if (S.exact_halos && keep_r) CHK(fill_halo_js(F, F.v.r, true)); else F.r_halo_stale = true;
  // p = p + r over the whole array: the interior was updated by the kernel; the halo of p + halo of r
  // equals the halo fill of the updated p (both are images of the same interior cells)
  CHK(fill_halo_js(F, F.v.p, true));
  return 0;
}

// relax(lev, nsweeps) of the level below the coarsest one (a closed level the one-workgroup kernel serves), with coarse2fine(lev) folded
// in front (flags & 1) and / or compute_residual(lev) + fine2coarse(lev) folded behind (flags & 2): mgx_relax_coarse.hip.  Returns 1 when
// the fused kernel took the job (same bits as the separate operators), 0 = run them.
int relax_fused(int lev, int nsweeps, int flags) {
  if (lev >= S.nlevs || !S.use_small || !S.use_fuse || S.method == M_GS || S.tictoc || S.keep_r || S.exact_halos || !S.linear) return 0;
  Level &F = S.lev[lev - 1], &C = S.lev[lev];
  const int mode = rb_mode(F);
  if (mode == RB_EXACT) return 0;
  const Sides phf = sides_of(F), phc = sides_of(C);
  if (!all_physical(phf) || !all_physical(phc) || C.gather || held_pair(F, C)) return 0;   // (the folded transfers halve nz)
  if (!mgxk_relax_wave_fused(S.stream, &F.v, &C.v, nsweeps, S.method, S.real, phf, flags, mode)) return 0;
  S.n_launch++;
  if (flags & 1) F.r_halo_stale = true;  // what coarse2fine leaves (the correction is not stored in r inside a cycle)
  return 1;
}

// relax(nlevs, ns_coarsest) inside a cycle (mg_solvers.f90:117,144), where the coarsest level is entered with p = 0 (fine2coarse, mg_intergrids.f90:70):
// where option "coarsest_direct" allows it, one matrix-vector product with the operator the level's relax kernel built (mgx_relax_coarse.hip)
// p_zero: the caller has just restricted onto the level (Vcycle(nlevs) called as an operator relaxes whatever p it finds: the sweeps)
int coarsest_solve(bool p_zero) {
  Level &L = S.lev[S.nlevs - 1];
  const Sides ph = sides_of(L);
  const int rbm = rb_mode(L), exact = rbm == RB_EXACT, seq = rbm == RB_SEQ;
  const bool want = S.coarsest_direct == 2 || (S.coarsest_direct == 1 && seq);
  // option "small_any_nz" decides whether a coarsest level of nz = 3 has an instance (k_relax_wave<3>): part of the operator's key, and a
  // level found without an instance under the other value is asked again
  const int any = S.small_any_nz ? 1 : 0;
  if (S.cd_any != any) { S.cd_any = any; S.cd_valid = 0; if (S.cd_n < 0) S.cd_n = 0; }
  if (want && p_zero && S.nlevs >= 2 && S.use_small && !S.tictoc && S.method != M_GS && !exact && all_physical(ph) && !L.gather && S.par.ns_coarsest >= 1 && S.cd_n >= 0) {
    const int n = mgxk_coarse_direct_cells(&L.v, any), mode = seq ? 2 : 0;
    if (n > 0) {
      if (!S.cd_M) {
        CHK(dmalloc(&S.cd_pb, (size_t)2 * n * L.n3js)); CHK(dmalloc(&S.cd_M, (size_t)n * n));
        CHK(dmalloc(&S.cd_part, (size_t)mgxk_coarse_direct_slabs(n) * n));
        { double *q = nullptr; CHK(dmalloc(&q, 512)); S.cd_cnt = (unsigned int *)q; }   // one word per 64 rows, 64 bytes apart (zeroed by dmalloc)
        S.cd_n = n;
      }
      if (!S.cd_valid || S.cd_method != S.method || S.cd_mode != mode || S.cd_nsweeps != S.par.ns_coarsest) {
        if (mgxk_coarse_direct_build(S.stream, &L.v, S.par.ns_coarsest, S.method, S.real, ph, mode, S.cd_pb, (long long)L.n3js, S.cd_M, any)) {
          S.cd_valid = 1; S.cd_method = S.method; S.cd_mode = mode; S.cd_nsweeps = S.par.ns_coarsest; S.n_launch += 3;
        } else { S.cd_valid = 0; S.cd_n = -1; }   // no one-workgroup kernel for this level: the sweeps
      }
      if (S.cd_valid && mgxk_coarse_direct_apply(S.stream, &L.v, S.cd_M, S.cd_part, S.cd_cnt, ph, any)) { S.n_launch++; S.n_direct++; if (L.nz == 3) S.n_small_any++; return 0; }
    } else S.cd_n = -1;
  }
  return relax(S.nlevs, S.par.ns_coarsest);
}

// mg_solvers.f90:129-151.  lead_c2f: the caller is Fcycle, whose coarse2fine(lev1) comes right before (:119-120)
int vcycle(int lev1, bool lead_c2f) {
  for (int lev = lev1; lev <= S.nlevs - 1; lev++) {
    const bool lead = lead_c2f && lev == lev1;
    if (relax_fused(lev, S.par.ns_pre, lead ? 3 : 2)) continue;
    if (lead) CHK(coarse2fine(lev, S.exact_halos || S.keep_r, S.c2f_skip && S.method == M_FC && S.par.ns_pre >= 1));
    CHK(relax(lev, S.par.ns_pre));
    CHK(fine2coarse(lev, false, true));  // compute_residual(lev) + fine2coarse(lev)
  }
  CHK(coarsest_solve(lev1 < S.nlevs));
  for (int lev = S.nlevs - 1; lev >= lev1; lev--) {
    if (relax_fused(lev, S.par.ns_post, 1)) continue;
    CHK(coarse2fine(lev, S.exact_halos || S.keep_r, S.c2f_skip && S.method == M_FC && S.par.ns_post >= 1));
    CHK(relax(lev, S.par.ns_post));
  }
  return 0;
}

// mg_solvers.f90:155-177: partial V-cycle down to level lev2
int vcycle2(int lev1, int lev2) {
  for (int lev = lev1; lev <= lev2 - 1; lev++) {
    CHK(relax(lev, S.par.ns_pre));
    CHK(fine2coarse(lev, false, true));  // compute_residual(lev) + fine2coarse(lev)
  }
  CHK(relax(lev2, S.par.ns_coarsest));
  for (int lev = lev2 - 1; lev >= lev1; lev--) {
    CHK(coarse2fine(lev, S.exact_halos || S.keep_r, S.c2f_skip && S.method == M_FC && S.par.ns_post >= 1));
    CHK(relax(lev, S.par.ns_post));
  }
  return 0;
}

// mg_solvers.f90:104-126
// have_r2: grid(2)%r already holds the restriction of the level-1 residual (the closing compute_residual of the previous solve_p
// iteration wrote it, residual_closing below): the first fine2coarse is then grid(2)%b = grid(2)%r and grid(2)%p = 0, two small copies
// have_r2 == 2: the caller has done the whole first fine2coarse(1) itself (grid(2)%b, %r and %p are set: solve_p_krylov)
int fcycle(int have_r2) {
  TicScope ts(1, "Fcycle");  // mg_solvers.f90:108
  for (int lev = 1; lev <= S.nlevs - 1; lev++) {
    if (lev == 1 && have_r2 == 2) continue;
    if (lev == 1 && have_r2) {
      Level &C = S.lev[1];
      HIPCHK(hipMemcpyAsync(C.v.b, C.v.r, C.n3js * sizeof(double), hipMemcpyDeviceToDevice, S.stream));   // physical images included (the kernel stored them)
      HIPCHK(hipMemsetAsync(C.v.p, 0, C.n3js * sizeof(double), S.stream));
      C.b_halo_stale = true; S.n_launch += 2;
      continue;
    }
    if (lev >= 2 && S.use_chain && !S.exact_halos) {
      // the rest of the first leg (closed, un-gathered levels: a single rank, or everything below the gathers) as ONE launch, up to four levels at a time
      int dep = 0;
      const LevView *vs[5] = {&S.lev[lev - 1].v, nullptr, nullptr, nullptr, nullptr};
      bool ok = true;
      for (int q = lev - 1; q < S.nlevs && ok; q++) { const Level &Lq = S.lev[q]; ok = all_physical(sides_of(Lq)) && (q == lev - 1 || !Lq.gather); }
      if (ok) {
        // (a held pair -- option "hold_odd_nz" -- is no 8-cell sum: the chain ends above it)
        while (dep < 4 && lev + dep < S.nlevs && !held_pair(S.lev[lev - 1 + dep], S.lev[lev + dep])) { dep++; vs[dep] = &S.lev[lev - 1 + dep].v; }
        if (mgxk_restrict_chain_served(vs, dep)) {
          const Sides all = {1, 1, 1, 1};
          mgxk_restrict_chain(S.stream, vs, dep, all); S.n_launch++;
          lev += dep - 1;
          continue;
        }
      }
    }
    CHK(fine2coarse(lev, true));  // + grid(lev+1)%r = grid(lev+1)%b (mg_solvers.f90:113)
  }
  CHK(coarsest_solve(S.nlevs >= 2));
  for (int lev = S.nlevs - 1; lev >= 1; lev--) CHK(vcycle(lev, true));  // coarse2fine(lev) + Vcycle(lev), :119-120
  return 0;
}

// compute_residual(1, res) at the end of a solve_p iteration (mg_solvers.f90:65).  If the loop goes on, the next thing that happens to this r
// is Fcycle's fine2coarse(1) (:112-115): the fused residual+restriction kernel (mgx_resrest.hip) forms the norm's partial sums AND the
// restricted r in one pass, into grid(2)%r only -- grid(2)%b and %p keep what the last cycle left, should the loop stop here.  The level-1 r
// is NOT written; the caller materialises it after the loop.  Returns 1 = fused (grid(2)%r is ready), 0 = the caller runs residual(1).
int residual_closing(double *res) {
  if (!S.fuse_closing || S.nlevs < 2 || S.exact_halos || S.keep_r || S.tictoc) return 0;
  Level &F = S.lev[0], &C = S.lev[1];
  if (C.gather || (held_pair(F, C) && !S.hold_z_fuse)) return 0;
  // (levels 1 and 2 are a held pair under option "hold_z_levels": the same pass by the held pair's kernel, mgx_resrest_held.hip)
  const bool held = held_pair(F, C);
  const int np = held ? mgxk_residual_restrict_held_grid(&F.v, &C.v) : mgxk_residual_restrict_grid(&F.v, &C.v);
  if (np > S.npartial) return 0;
  const Sides phc = sides_of(C);
  if (!(held ? mgxk_residual_restrict_held(S.stream, &F.v, &C.v, C.v.r, S.real, phc, nullptr, S.d_partial, nullptr)
             : mgxk_residual_restrict_ex(S.stream, &F.v, &C.v, C.v.r, S.real, phc, nullptr, S.d_partial, nullptr))) return 0;
  if (held) S.n_hold_z_fused++;
  mgxk_reduce(S.stream, S.d_partial, np, S.d_scalar); S.n_launch += 2;
  C.r_halo_stale = true;
  double s;
  if (global_sum(F, &s)) return -1;
  *res = sqrt(s);
  return 1;
}

// Fortran's Ew.3 edit descriptor (0.dddE+ee), so that the printed history reads like the reference's (format 10, mg_solvers.f90:99)
std::string fortran_e3(double v, int width) {
  char buf[32];
  if (v == 0.0 || !std::isfinite(v)) snprintf(buf, sizeof buf, v == 0.0 ? "0.000E+00" : "%f", v);
  else {
    const double a = fabs(v);
    int e = (int)floor(log10(a)) + 1;
    long m = lround(a / pow(10.0, e) * 1000.0);
    if (m >= 1000) { m = 100; e++; }
    if (m < 100) { m *= 10; e--; }
    if (abs(e) < 100) snprintf(buf, sizeof buf, "%s0.%03ldE%c%02d", v < 0 ? "-" : "", m, e < 0 ? '-' : '+', abs(e));
    else snprintf(buf, sizeof buf, "%s0.%03ld%c%03d", v < 0 ? "-" : "", m, e < 0 ? '-' : '+', abs(e));
  }
  std::string t(buf);
  if ((int)t.size() < width) t.insert(0, width - t.size(), ' ');
  return t;
}

// What the three solve_p drivers share (mg_solvers.f90:17-101): the prints, the timer, the start (p = 0, ||b||, the first residual), the
// bookkeeping of an iteration (history, "ite = ..." line, fort.100 line) and the summary.  A driver owns what happens between two norms.
// fort.100 is closed and the timer stopped on every way out, a CHK that returns early included.
namespace {
struct SolveRun {
  Level &L = S.lev[0];
  const bool talk = S.verbose && S.rank == 0;
  double *const hist;
  std::chrono::steady_clock::time_point tstart;
  FILE *f100 = nullptr;
  double bnorm = 0.0, res0 = 0.0, rnorm0 = 0.0;   // ||b||; the relative residual of the current iterate and of the first one
  int nite = 0;
  explicit SolveRun(double *h) : hist(h) {
    if (talk) printf(" - solve p:\n");
    tic(1, "solve");  // mg_solvers.f90:45
    tstart = std::chrono::steady_clock::now();  // cpu_time(tstart) (:46); wall clock here, the work is on the GPU
  }
  SolveRun(const SolveRun &) = delete;
  ~SolveRun() { if (f100) fclose(f100); toc(1, "solve"); }
  // *rabs = ||b - A p|| of the starting iterate, r written into grid(1)%r
  int begin(double *rabs) {
    if (!S.warm_start) HIPCHK(hipMemsetAsync(L.v.p, 0, L.n3js * sizeof(double), S.stream));  // grid(1)%p = 0 (:35)
    mgxk_sumsq(S.stream, &L.v, L.v.b, S.d_partial, S.d_scalar); S.n_launch += 2;
    CHK(global_sum(L, &bnorm)); bnorm = sqrt(bnorm);
    CHK(residual(1, rabs));
    res0 = rnorm0 = *rabs / bnorm;
    if (hist) hist[0] = res0;
    f100 = talk ? fopen("fort.100", "a") : nullptr;
    if (f100) fprintf(f100, " %24.16E %d\n", res0, nite);
    return 0;
  }
  bool more(double tol, int maxite) const { return nite < maxite && res0 > tol; }
  // an iteration has ended with the relative residual rnorm
  void step(double rnorm) {
    const double conv = res0 / rnorm;
    res0 = rnorm;
    nite++;
    if (hist) hist[nite] = rnorm;
    if (talk) printf("ite = %2d: res = %s / conv = %10.3f\n", nite, fortran_e3(rnorm, 10).c_str(), conv);
    if (f100) fprintf(f100, " %24.16E %24.16E\n", rnorm, conv);
  }
  void finish(int *nite_out, double *res_out) {
    if (talk) {  // the summary block (mg_solvers.f90:83-97)
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - tstart).count();
      const double np = (double)L.npx * L.npy, ncell = (double)L.nx * L.npx * (double)L.ny * L.npy * (double)L.nz;
      const double perf = dt * np / (-log(res0 / rnorm0) / log(10.0)) / ncell;
      printf(" --- summary ---\ntime spent to solve :%8.3f s\nrescaled performance:%s\n ---------------\n", dt, fortran_e3(perf, 10).c_str());
    }
    if (nite_out) *nite_out = nite;
    if (res_out) *res_out = res0;
  }
};
}  // namespace

// mg_solvers.f90:17-101
int solve_p(double tol, int maxite, int *nite_out, double *res_out, double *hist) {
  SolveRun run(hist);
  double rnorm; CHK(run.begin(&rnorm));
  bool have_r2 = false;  // grid(2)%r = restriction of the current level-1 residual, and grid(1)%r not written (residual_closing)
  while (run.more(tol, maxite)) {
    CHK(fcycle(have_r2));
    const int fz = residual_closing(&rnorm);
    if (fz < 0) return 1;
    have_r2 = fz == 1;
    if (!fz) CHK(residual(1, &rnorm));
    run.step(rnorm / run.bnorm);
  }
  if (have_r2) CHK(residual(1, nullptr));  // grid(1)%r of the final iterate, which the fused closing residual did not write (once per solve)
  run.finish(nite_out, res_out);
  return 0;
}

// ---- mixed-precision solve_p (option "cycle_precision" = 32) ------------------------------------------------------------
// Iterative refinement around the reference's F-cycle: the fp64 loop below keeps p, r = b - A p, ||r||, the history and the stopping
// test of solve_p (the accuracy contract is solver_prec on the fp64 relative residual, mg_solvers.f90:50-80); each iteration runs the
// F-cycle in correction form, A e = s r from e = 0, on fp32 shadows of every level (mgx_mixed.hip) and adds e / s to p.  The cycle only
// has to deliver a correction good to ~1e-2 of r, which fp32 does.  Single rank only: the halo and gather callbacks carry doubles.

// the layout of LevView with 4-byte elements: the first interior column of either half-row 128-byte aligned
void make_view32(LevView32 &v, int nx, int ny, int nz) {
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.EO = 31;
  v.HO = roundup(32 + ny / 2, 32);
  v.RS = roundup(v.HO + ny / 2 + 1, 32);
  v.plane = (long long)nz * v.RS;
}
int fmalloc(float **p, size_t n) { double *q = nullptr; CHK(dmalloc(&q, (n + 1) / 2)); *p = (float *)q; return 0; }

// the combinations the fp32 cycle does not serve
int mixed_check() {
  if (S.periodic) return fail("option \"periodic\" = %d is not served by the fp32 cycles (cycle_precision = 32, krylov_precision = 32): the fp32 shadow has mirror halos only", S.periodic);
  if (S.nranks > 1) return fail("cycle_precision = 32 needs a single rank (process grid %d x %d): the halo and gather callbacks carry doubles", S.npx, S.npy);
  if (S.method == M_GS) return fail("cycle_precision = 32 does not serve relax_method = 'GS' (four colours or red-black only)");
  if (S.rb_exact) return fail("cycle_precision = 32 does not serve option rb_exact (the fp32 red-black pass is the parallel one)");
  for (int l = 1; l < S.nlevs; l++)
    if (held_pair(S.lev[l - 1], S.lev[l]))
      return fail("option \"hold_odd_nz\" = 1 holds nz = %d from level %d on, which the fp32 cycles (cycle_precision = 32, krylov_precision = 32, mixed_tail) do not serve: the transfers of the fp32 shadow halve nz", S.lev[l].nz, l);
  return 0;
}

// allocate the fp32 shadow on first use (through the allocation list: mgx_clean frees it) and convert the coefficients and pivots
// whenever the fp64 ones have changed since the last conversion
int mixed_prepare() {
  if (!S.mx_ready) {
    for (auto &L : S.lev) {
      LevView32 &v = L.v32;
      make_view32(v, L.nx, L.ny, L.nz);
      L.n3js32 = (size_t)(L.nx + 2) * v.plane;
      CHK(fmalloc(&v.e, L.n3js32)); CHK(fmalloc(&v.f, L.n3js32)); CHK(fmalloc(&v.r, L.n3js32));
      for (int s = 0; s < 8; s++) CHK(fmalloc(&v.cA[s], L.n3js32));
      CHK(fmalloc(&v.bet, L.n3js32));
      v.p1 = nullptr;
      if (S.method == M_RB && S.real) CHK(fmalloc(&v.p1, (size_t)(L.nx + 2) * v.RS));
    }
    S.mx_ready = true;
    S.mx_gen = ~0ULL;
    // the tail of the cycles: the run of coarsest levels that are all small (0: none)
    S.mx_tail_first = 0;
    for (int lev = S.nlevs; lev >= 1 && mixed_tail_small(S.lev[lev - 1].nx, S.lev[lev - 1].ny, S.lev[lev - 1].nz); lev--) S.mx_tail_first = lev;
  }
  if (S.mx_gen != S.coef_gen) {
    for (auto &L : S.lev) {
      for (int s = 0; s < 8; s++) mgxx_to32(S.stream, &L.v, &L.v32, L.v.cA[s], L.v32.cA[s], 1.0);
      mgxx_to32(S.stream, &L.v, &L.v32, L.v.bet, L.v32.bet, 1.0);   // pivots: computed in fp64 from the fp64 slots (k_pivots), rounded
      S.n_launch += 9;
    }
    S.mx_gen = S.coef_gen;
  }
  return 0;
}

// Option "mixed_tail": the level at which a cycle entered at lev1 hands over to the tail kernel (k_tail32, mgx_mixed.hip), 0 = nowhere:
// the option is off, no level is small, or the levels from there down are more than one launch takes -- the cycle then keeps its launches
// (a tail of 32768 cells at the most has at most four levels, which is what a launch takes: mgx_mixed.hip).
int tail_hand(int lev1) {
  if (!S.mixed_tail || !S.mx_tail_first) return 0;
  const int hand = std::max(lev1, S.mx_tail_first);
  return S.nlevs - hand + 1 <= mgxx_tail_max_levels() ? hand : 0;
}
// one launch of the tail kernel on levels lev .. last (tail_hand has counted them).  dM (option "mixed_direct", direct32_operator): the
// coarsest solves inside the launch are products -- nl of them in an F-cycle tail of nl levels, one in a V-cycle tail
int tail32(int lev, int last, int mode, bool lead, int n, const float *dM = nullptr, int dn = 0) {
  const LevView32 *vs[8];
  const int nl = last - lev + 1;
  if (nl < 1 || nl > 8) return fail("mixed_tail: levels %d..%d", lev, last);
  for (int q = 0; q < nl; q++) vs[q] = &S.lev[lev - 1 + q].v32;
  if (!mgxx_tail(S.stream, vs, nl, mode, lead ? 1 : 0, n, S.par.ns_pre, S.par.ns_post, S.par.ns_coarsest, S.method == M_RB, S.real, S.linear, dM, dn))
    return fail("mixed_tail: the tail kernel does not serve levels %d..%d (set option mixed_tail = 0)", lev, last);
  S.n_launch++; S.n_mixed_tail++;
  if (dM) S.n_mixed_direct += mode == TAIL_FCYCLE ? nl : 1;
  return 0;
}

// relax(lev, nsweeps) on the fp32 shadow: four colours, or the parallel red-black pass (k = 1 same-colour diagonals from a snapshot
// taken before each colour: the fp64 pass with rb_seq = 0); a small level in one launch (option "mixed_tail"); the colour pass of a level
// that is not small by the pipelined kernel (option "mixed_ring": choose_relax32, mgx_choice.h), launch for launch
int relax32(int lev, int nsweeps) {
  LevView32 &v = S.lev[lev - 1].v32;
  if (nsweeps > 0 && S.mixed_tail && S.mx_tail_first && lev >= S.mx_tail_first) return tail32(lev, lev, TAIL_RELAX, false, nsweeps);
  for (int it = 1; it <= nsweeps; it++) {
    if (S.method == M_FC) {
      for (int fc1 = 1; fc1 <= 2; fc1++)
        for (int fc2 = 1; fc2 <= 2; fc2++) { S.n_mixed_ring += mgxx_relax_pass(S.stream, &v, fc1, 2, v.nx / 2, fc2 == 1 ? 1 : 0, 0, S.real, 0, S.mixed_ring); S.n_launch++; }
    } else {
      for (int rb = 1; rb <= 2; rb++) {
        if (S.real) { mgxx_snapshot(S.stream, &v); S.n_launch++; }
        S.n_mixed_ring += mgxx_relax_pass(S.stream, &v, 1, 1, v.nx, -1, rb, S.real, S.real, S.mixed_ring); S.n_launch++;
      }
    }
  }
  return 0;
}
void coarse2fine32(int lev) { mgxx_coarse2fine(S.stream, &S.lev[lev - 1].v32, &S.lev[lev].v32, S.linear); S.n_launch++; }

// Option "mixed_direct": the operator of the coarsest solve of an fp32 cycle, *M = nullptr where the sweeps run (the option is off, a timed
// call, no sweeps, a shape the product does not serve, a level the builder has no kernel for).  B32 is the fp64 operator rounded once: the
// fp64 level's own one-workgroup relax kernel builds it from the unit vectors in its parallel colour order (mode 0, what the fp32 red-black
// restates), then one launch converts it.  Built at the first served solve, again when the coefficients have changed (coef_gen) or option
// "small_any_nz" has (it decides whether nz = 3 has a kernel).  State of its own: the fp64 direct solve (cd_*) is not touched -- its scratch
// cd_pb is borrowed where it exists, every launch being ordered by the stream.
int direct32_operator(const float **M, int *n) {
  *M = nullptr; *n = 0;
  if (!S.mixed_direct || S.tictoc || S.par.ns_coarsest < 1) return 0;
  Level &L = S.lev[S.nlevs - 1];
  const int any = S.small_any_nz ? 1 : 0;
  const int cells = mgxx_direct32_cells(L.nx, L.ny, L.nz, S.nlevs, any);
  if (!cells) return 0;
  if (S.md_gen != S.coef_gen || S.md_any != any) {
    S.md_gen = S.coef_gen; S.md_any = any; S.md_valid = 0;
    if (S.md_n != cells) {   // (a level has one size: allocated once)
      CHK(fmalloc(&S.md_M, (size_t)cells * cells)); CHK(dmalloc(&S.md_M64, (size_t)cells * cells));
      if (!S.cd_pb) CHK(dmalloc(&S.md_pb, (size_t)2 * cells * L.n3js));
      S.md_n = cells;
    }
    if (mgxk_coarse_direct_build(S.stream, &L.v, S.par.ns_coarsest, S.method, S.real, sides_of(L), 0, S.cd_pb ? S.cd_pb : S.md_pb, (long long)L.n3js, S.md_M64, any)) {
      mgxx_direct32_round(S.stream, S.md_M64, S.md_M, cells);
      S.md_valid = 1; S.n_launch += 4;
    }   // else: no one-workgroup kernel for this level, remembered until the matrix or the option changes
  }
  if (S.md_valid) { *M = S.md_M; *n = cells; }
  return 0;
}

// relax(nlevs, ns_coarsest) of a cycle on the shadow.  e_zero: the caller has just restricted onto the level, so the solve is a fixed linear
// map of f and option "mixed_direct" may serve it as one product (k_coarse_direct32); a V-cycle entered at the coarsest level as an
// operator relaxes whatever e it finds: the sweeps.
int coarsest_solve32(bool e_zero) {
  const float *M = nullptr; int n = 0;
  if (e_zero) CHK(direct32_operator(&M, &n));
  if (M && mgxx_coarse_direct32(S.stream, &S.lev[S.nlevs - 1].v32, M, S.nlevs, S.small_any_nz ? 1 : 0)) { S.n_launch++; S.n_mixed_direct++; return 0; }
  return relax32(S.nlevs, S.par.ns_coarsest);
}
// the same decision for a cycle whose coarsest solve lies inside a tail launch on levels hand .. nlevs
int tail32_cycle(int hand, int mode, bool lead) {
  const float *M = nullptr; int n = 0;
  if (hand < S.nlevs) CHK(direct32_operator(&M, &n));
  return tail32(hand, S.nlevs, mode, lead, 0, M, n);
}

// mg_solvers.f90:129-151 on the shadow; lead_c2f: Fcycle's coarse2fine(lev1) comes first (:119-120).  Option "mixed_tail": from level
// `hand` down to the coarsest relax and back up to hand's post-smoothing in one launch; the levels above keep theirs, the transfers
// between hand - 1 and hand included.
int vcycle32(int lev1, bool lead_c2f) {
  const int hand = tail_hand(lev1), bottom = hand ? hand : S.nlevs;
  for (int lev = lev1; lev <= bottom - 1; lev++) {
    if (lead_c2f && lev == lev1) coarse2fine32(lev);
    CHK(relax32(lev, S.par.ns_pre));
    mgxx_resrest(S.stream, &S.lev[lev - 1].v32, &S.lev[lev].v32, S.real); S.n_launch++;   // compute_residual(lev) + fine2coarse(lev)
  }
  if (hand) CHK(tail32_cycle(hand, TAIL_VCYCLE, lead_c2f && hand == lev1));
  else CHK(coarsest_solve32(lev1 < S.nlevs));
  for (int lev = bottom - 1; lev >= lev1; lev--) {
    coarse2fine32(lev);
    CHK(relax32(lev, S.par.ns_post));
  }
  return 0;
}

// mg_solvers.f90:104-126 on the shadow, level 1 holding (e, f) = (0, s r): the first leg restricts f (the residual of e = 0).
// Option "mixed_tail": the first leg from level `hand` on, the coarsest relax and the V-cycles that start inside the tail in one launch.
int fcycle32() {
  TicScope ts(1, "Fcycle");
  const int hand = tail_hand(1), bottom = hand ? hand : S.nlevs;
  for (int lev = 1; lev <= bottom - 1; lev++) {
    mgxx_restrict(S.stream, &S.lev[lev - 1].v32, &S.lev[lev].v32, S.lev[lev - 1].v32.f); S.n_launch++;
  }
  if (hand) CHK(tail32_cycle(hand, TAIL_FCYCLE, false));
  else CHK(coarsest_solve32(S.nlevs >= 2));
  for (int lev = bottom - 1; lev >= 1; lev--) CHK(vcycle32(lev, true));
  return 0;
}

// solve_p with fp32 cycles: the same prints, fort.100 lines, history, warm_start handling and res0 relative to ||b|| as solve_p
int solve_p_mixed(double tol, int maxite, int *nite_out, double *res_out, double *hist) {
  CHK(mixed_check());
  CHK(mixed_prepare());
  SolveRun run(hist);
  Level &L = run.L;
  double rabs; CHK(run.begin(&rabs));   // fp64 r = b - A p, written into grid(1)%r
  while (run.more(tol, maxite)) {
    // f = s r with s = 1 / ||r||: |f| <= 1, nothing underflows however small the residual has become; e = 0
    const double sc = rabs > 0.0 ? 1.0 / rabs : 1.0;
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.r, L.v32.f, sc); S.n_launch++;
    HIPCHK(hipMemsetAsync(L.v32.e, 0, L.n3js32 * sizeof(float), S.stream));
    CHK(fcycle32());
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.e, L.v.p, rabs > 0.0 ? rabs : 1.0, 1); S.n_launch++;   // p += e / s, halo images included
    CHK(residual(1, &rabs));
    S.n_mixed++;
    run.step(rabs / run.bnorm);
  }
  run.finish(nite_out, res_out);
  return 0;
}

// ---- Krylov-accelerated solve_p (option "krylov" = m) -------------------------------------------------------------------
// Right-preconditioned truncated GCR (Orthomin(m)) with M = one Fcycle from p = 0 on the right-hand side r: a fixed linear map, not a
// symmetric one (3 pre / 2 post coloured sweeps), hence GCR and not CG.  Per iteration: z = M r, q = A z, (z, q) made A^T A-orthogonal to
// the m retained pairs, p += (t / s) z, r -= (t / s) q with s = (q, q), t = (r, q).  The F-cycle reads level 1 through its view, so the
// view's p / b / r are pointed at (z, r, scratch) for the cycle and back afterwards: nothing is copied.  r of the recurrence lives in
// grid(1)%r; the scratch r of the cycle is the q of the pair in work, which is only written after the cycle.
// Option "krylov_precision" = 32: M is the fp32 F-cycle of solve_p_mixed, A e = f from e = 0 on the shadows with f = r / N, and z = N e.  GCR
// takes an inexact, even a varying, preconditioner, and N only has to keep |f| <= ~1, so N is the norm the host already holds as the
// iteration starts: the true residual's after the start and after a restart, the recurrence's otherwise (the history is monotone).  Pass 3
// leaves f for the next cycle (k_kr_update32) and pass 1 reads e (k_kr_apply32): the only conversion launch is the k_to32 of a fresh r.  The
// fp32 cycle never touches the fp64 view, so no ViewSwap around it.
// The recurrence's r drifts away from b - A p near round-off, so no convergence is reported on its word: the true residual is computed
// (compute_residual(1)) before the loop is left, and where it is not below tol it becomes r, the retained pairs are dropped
// (kr_restarts) and the loop goes on.  On every exit grid(1)%r, *res and the last hist entry are the true residual's.
struct ViewSwap {   // level 1's p / b / r as the solver owns them, put back on every way out
  LevView &v; double *p, *b, *r;
  explicit ViewSwap(LevView &w) : v(w), p(w.p), b(w.b), r(w.r) {}
  void restore() { v.p = p; v.b = b; v.r = r; }
  ~ViewSwap() { restore(); }
};

int krylov_prepare(int m) {
  Level &L = S.lev[0];
  if (!S.kr_sc) { CHK(dmalloc(&S.kr_sc, 32)); CHK(dmalloc(&S.kr_partial, (size_t)mgxq_partials(&L.v))); }
  for (; S.kr_n < m + 1; S.kr_n++) { CHK(dmalloc(&S.kr_z[S.kr_n], L.n3js)); CHK(dmalloc(&S.kr_q[S.kr_n], L.n3js)); }
  return 0;
}

// the inner products of one pass summed over the ranks: ONE call of the all-reduce hook
int krylov_allreduce(double *buf, int n) {
  if (S.nranks <= 1 || n == 0) return 0;
  if (!S.ar) return fail("an all-reduce is needed (npx*npy > 1) but mgx_set_comm was not called");
  S.n_allred++;
  if (S.ar(S.ctx, buf, n)) return fail("allreduce callback failed");
  return 0;
}

int solve_p_krylov(double tol, int maxite, int *nite_out, double *res_out, double *hist) {
  const int m = S.krylov;
  const bool lowp = S.krylov_precision == 32;
  if (lowp) { CHK(mixed_check()); CHK(mixed_prepare()); }
  CHK(krylov_prepare(m));
  SolveRun run(hist);
  Level &L = run.L;
  double rnorm; CHK(run.begin(&rnorm));   // the true residual, into grid(1)%r
  double rabs = rnorm, fnorm = 1.0;       // lowp: ||r|| as the iteration starts (see above); the shadow's f holds r / fnorm
  ViewSwap own(L.v);
  double *sc = S.kr_sc, *qq = S.kr_sc + 16;
  int kept = 0, head = 0;   // retained pairs: the `kept` slots before `head` in the ring of m + 1; head = the pair in work
  bool fresh = true, broke = false;   // fresh: grid(1)%r is the true residual of grid(1)%p
  S.kr_restarts = 0;
  for (;;) {
    while (run.more(tol, maxite)) {
      double *z = S.kr_z[head], *q = S.kr_q[head];
      const double nscale = rabs > 0.0 ? rabs : 1.0;
      if (lowp) {  // e = M f on the shadows; z is formed by pass 1
        if (fresh) { fnorm = nscale; mgxx_to32(S.stream, &L.v, &L.v32, own.r, L.v32.f, 1.0 / fnorm); S.n_launch++; }
        HIPCHK(hipMemsetAsync(L.v32.e, 0, L.n3js32 * sizeof(float), S.stream));
        CHK(fcycle32());
      } else {  // z = M r: Fcycle on (p, b) = (0, r).  The first leg restricts the view's r, the rest of the cycle may use it as scratch.
        HIPCHK(hipMemsetAsync(z, 0, L.n3js * sizeof(double), S.stream));
        L.v.p = z; L.v.b = own.r; L.v.r = own.r;
        int rc = S.nlevs >= 2 ? fine2coarse(1, true) : 0;
        L.v.r = q;
        if (!rc) rc = fcycle(2);
        own.restore();
        if (rc) return rc;
      }
      const double *zi[8], *qi[8]; int slot[8];
      for (int n = 0; n < kept; n++) { slot[n] = (head + m + 1 - kept + n) % (m + 1); zi[n] = S.kr_z[slot[n]]; qi[n] = S.kr_q[slot[n]]; }
      {
        TicScope t1(1, "krylov_apply");
        LevView zv = L.v; zv.p = z;
        if (lowp) mgxq_apply32(S.stream, &L.v, &L.v32, fnorm, z, q, qi, kept, S.kr_partial, sc, S.real);
        else mgxq_apply(S.stream, &zv, q, qi, kept, S.kr_partial, sc, S.real);
        S.n_launch += kept ? 2 : 1;
        CHK(krylov_allreduce(sc, kept));
      }
      {
        TicScope t2(1, "krylov_ortho");
        mgxq_ortho(S.stream, &L.v, z, q, own.r, zi, qi, slot, kept, sc, qq, S.kr_partial, sc + 8); S.n_launch += 2;
        CHK(krylov_allreduce(sc + 8, 2));
      }
      double s2;
      {
        TicScope t3(1, "krylov_update");
        if (lowp) { mgxq_update32(S.stream, &L.v, &L.v32, own.p, own.r, z, q, 1.0 / nscale, sc + 8, qq + head, S.kr_partial, S.d_scalar); fnorm = nscale; }
        else mgxq_update(S.stream, &L.v, own.p, own.r, z, q, sc + 8, qq + head, S.kr_partial, S.d_scalar);
        S.n_launch += 2;
        CHK(global_sum(L, &s2));   // the iteration's one host synchronisation: the stopping test
      }
      fresh = false;
      if (!(s2 >= 0.0)) { broke = true; break; }   // no step was taken (s == 0 or a non-finite scalar): p is what it was
      rabs = sqrt(s2);
      run.step(rabs / run.bnorm);
      if (lowp) S.n_kr_mixed++;
      if (kept < m) kept++;
      head = (head + 1) % (m + 1);
    }
    if (fresh) break;
    CHK(residual(1, &rnorm));   // b - A p into grid(1)%r: the word that counts
    fresh = true; rabs = rnorm;
    run.res0 = rnorm / run.bnorm;   // (not printed: the lines above are the recurrence's)
    if (hist) hist[run.nite] = run.res0;
    if (broke || run.nite >= maxite || !(run.res0 > tol)) break;
    S.kr_restarts++; kept = 0;   // the recurrence had drifted: go on from the true residual with no history
  }
  run.finish(nite_out, res_out);
  return 0;
}

// Test hook of the three passes (mgx_krylov_op, include/mgx.h): ONE pass on level 1 through the wrapper solve_p_krylov calls, on the buffers
// it uses -- the ring S.kr_z / S.kr_q after krylov_prepare(nd), S.kr_partial, the scalars in S.kr_sc, grid(1)%p and %r, the level's own view,
// S.stream and S.real.  Fields cross as host arrays (nz, 0:ny+1, 0:nx+1) by the staging of mgx_set_field / mgx_get_field, halos as given.
// The retained pair n sits in ring slot slot[n] (0..nd, distinct; nullptr = 0..nd-1) and the pair in work in the slot left free.
int krylov_op(const char *op, int nd, double *const *f, const int *slot, const double *sin, double *sout, int *path) {
  if (!op) return fail("mgx_krylov_op: op is NULL");
  const int which = streq(op, "apply") ? 1 : streq(op, "ortho") ? 2 : streq(op, "update") ? 3 : streq(op, "apply32") ? 4 : streq(op, "update32") ? 5 : 0;
  if (!which) return fail("mgx_krylov_op: unknown pass '%s' (apply, ortho, update, apply32, update32)", op);
  if (which >= 4) { CHK(mixed_check()); CHK(mixed_prepare()); }
  if (nd < 0 || nd > 8) return fail("mgx_krylov_op(%s): nd = %d retained pairs (0..8)", op, nd);
  int sl[8], head = nd, used = 0;
  for (int n = 0; n < nd; n++) {
    sl[n] = slot ? slot[n] : n;
    if (sl[n] < 0 || sl[n] > nd || (used >> sl[n] & 1)) return fail("mgx_krylov_op(%s): slot[%d] = %d (distinct values of 0..%d)", op, n, sl[n], nd);
    used |= 1 << sl[n];
  }
  if (which != 3 && which != 5) for (head = 0; used >> head & 1;) head++;
  CHK(krylov_prepare(nd));
  Level &L = S.lev[0];
  const size_t n3 = (size_t)L.nz * (L.ny + 2) * (L.nx + 2);
  auto put = [&](const double *host, double *js) -> int {
    HIPCHK(hipMemcpyAsync(S.ref_scratch, host, n3 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    mgxk_convert(S.stream, &L.v, js, S.ref_scratch, 1, 0, 0);
    return 0;
  };
  auto get = [&](double *host, double *js) -> int {
    mgxk_convert(S.stream, &L.v, js, S.ref_scratch, 1, 0, 1);
    HIPCHK(hipMemcpyAsync(host, S.ref_scratch, n3 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    return 0;
  };
  double *sc = S.kr_sc, *qq = S.kr_sc + 16, *z = S.kr_z[head], *q = S.kr_q[head];
  const double *zi[8], *qi[8];
  for (int n = 0; n < nd; n++) { zi[n] = S.kr_z[sl[n]]; qi[n] = S.kr_q[sl[n]]; }
  if (path) { int g[4]; mgxq_path(&L.v, g); path[0] = g[0]; path[1] = S.real; path[2] = g[1]; path[3] = g[2]; path[4] = g[3]; }
  if (which == 1) {          // f = z, q (out), q_1 .. q_nd; sout[0..nd-1] = (q, q_i)
    CHK(put(f[0], z));
    for (int n = 0; n < nd; n++) CHK(put(f[2 + n], S.kr_q[sl[n]]));
    LevView zv = L.v; zv.p = z;
    mgxq_apply(S.stream, &zv, q, qi, nd, S.kr_partial, sc, S.real);
    CHK(get(f[1], q));
    if (nd) HIPCHK(hipMemcpyAsync(sout, sc, nd * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else if (which == 2) {   // f = z, q (both rewritten), r, then z_1, q_1, .. z_nd, q_nd; sin[0..7] = (q, q_i), sin[8..16] = (q_i, q_i) by ring slot
    CHK(put(f[0], z)); CHK(put(f[1], q)); CHK(put(f[2], L.v.r));
    L.r_halo_stale = false;
    for (int n = 0; n < nd; n++) { CHK(put(f[3 + 2 * n], S.kr_z[sl[n]])); CHK(put(f[4 + 2 * n], S.kr_q[sl[n]])); }
    HIPCHK(hipMemcpyAsync(sc, sin, 8 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipMemcpyAsync(qq, sin + 8, 9 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    mgxq_ortho(S.stream, &L.v, z, q, L.v.r, zi, qi, sl, nd, sc, qq, S.kr_partial, sc + 8);
    CHK(get(f[0], z)); CHK(get(f[1], q));
    HIPCHK(hipMemcpyAsync(sout, sc + 8, 2 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else if (which == 4) {   // f = e (doubles that fp32 holds exactly), z, q (both out), q_1 .. q_nd; sin[0] = 1 / sigma; sout[0..nd-1] = (q, q_i)
    CHK(put(f[0], L.v.p));     // e reaches the shadow through grid(1)%p
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0);
    { const std::vector<double> nan(n3, std::nan("")); CHK(put(nan.data(), z)); CHK(sync_stream()); }   // a cell of z the pass leaves out reads back as not-a-number
    for (int n = 0; n < nd; n++) CHK(put(f[3 + n], S.kr_q[sl[n]]));
    mgxq_apply32(S.stream, &L.v, &L.v32, sin[0], z, q, qi, nd, S.kr_partial, sc, S.real);
    CHK(get(f[1], z)); CHK(get(f[2], q));
    if (nd) HIPCHK(hipMemcpyAsync(sout, sc, nd * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else if (which == 5) {   // f = p, r (both rewritten), z, q, f (rewritten: the shadow's f, promoted); sin = {s, t, sigma}; slot and sout as "update"
    CHK(put(f[4], L.v.p));     // f reaches the shadow through grid(1)%p
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.f, 1.0);
    CHK(put(f[0], L.v.p)); CHK(put(f[1], L.v.r)); CHK(put(f[2], z)); CHK(put(f[3], q));
    L.r_halo_stale = false;
    HIPCHK(hipMemcpyAsync(sc + 8, sin, 2 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipMemsetAsync(qq, 0xff, 9 * sizeof(double), S.stream));
    mgxq_update32(S.stream, &L.v, &L.v32, L.v.p, L.v.r, z, q, sin[2], sc + 8, qq + head, S.kr_partial, S.d_scalar);
    CHK(get(f[0], L.v.p)); CHK(get(f[1], L.v.r));
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.f, z, 1.0, 0);
    CHK(get(f[4], z));
    HIPCHK(hipMemcpyAsync(sout, S.d_scalar, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipMemcpyAsync(sout + 1, qq + head, sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else {                   // f = p, r (both rewritten), z, q; sin = {s, t}; the new pair's ring slot is nd; sout = {||r||^2 or -1, what was filed there}
    CHK(put(f[0], L.v.p)); CHK(put(f[1], L.v.r)); CHK(put(f[2], z)); CHK(put(f[3], q));
    L.r_halo_stale = false;
    HIPCHK(hipMemcpyAsync(sc + 8, sin, 2 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipMemsetAsync(qq, 0xff, 9 * sizeof(double), S.stream));   // not-a-numbers: a slot nobody files reads back as one
    mgxq_update(S.stream, &L.v, L.v.p, L.v.r, z, q, sc + 8, qq + head, S.kr_partial, S.d_scalar);
    CHK(get(f[0], L.v.p)); CHK(get(f[1], L.v.r));
    HIPCHK(hipMemcpyAsync(sout, S.d_scalar, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipMemcpyAsync(sout + 1, qq + head, sizeof(double), hipMemcpyDeviceToHost, S.stream));
  }
  S.n_launch += 2;
  return sync_stream();
}

// the solve_p of mgx_solve_p / mgx_solve / mgx_solve_device: fp64 cycles, fp32 cycles under fp64 refinement, or the Krylov-accelerated loop
int solve_p_opt(double tol, int maxite, int *nite_out, double *res_out, double *hist) {
  if (S.krylov > 0 && S.cycle_precision == 32)
    return fail("options \"krylov\" = %d and \"cycle_precision\" = 32 cannot be combined (fp32 cycles under the Krylov loop are not served): set one of them back", S.krylov);
  if (S.krylov > 0) return solve_p_krylov(tol, maxite, nite_out, res_out, hist);
  return S.cycle_precision == 32 ? solve_p_mixed(tol, maxite, nite_out, res_out, hist) : solve_p(tol, maxite, nite_out, res_out, hist);
}

}  // namespace mgx_host
