// Which launch serves a level outside the smoother: the operator of a level (mgx_residual.hip, pass 1 of mgx_krylov.hip) and the streaming
// Krylov passes, the transfers (mgx_transfer.hip, mgx_hold.hip, mgx_resrest_held.hip), the halo and gather transport (mgx_halo.hip), the slot conversion
// (mgx_layout.hip) and the runs of the model kernels (mgx_model.hip).  Pure host functions by the rules of mgx_choice.h, which includes this
// file: no HIP call, no state, no environment; a small result struct per group; tests/test_kernel_choice_host.py pins every answer.
#pragma once

// ---- the operator of a level: mgxk_residual, mgxk_residual_nblocks, mgxq_apply, mgxq_apply32, mgxq_path, pass 1 of mgxq_partials ----
// One wave per 64 columns of a half-row, four planes per workgroup, the two j parities apart: gx * gy * 2 workgroups as a 1-D grid
// (op_block_map, mgx_operator.h); stream: b, r and q of a level beyond the cache are streamed past it
struct OpChoice { bool mf; int gx, gy; unsigned grid; int stream; };
static inline OpChoice choose_operator(const LevShape &s) {
  OpChoice c;
  c.mf = choose_operator_mf(s);
  c.gx = ch_chunks(s.ny); c.gy = (s.nx + 3) / 4;
  c.grid = (unsigned)c.gx * c.gy * 2;
  c.stream = ch_beyond_cache(s);
  return c;
}
// Krylov passes 2 and 3 stream whole arrays, halo and padding included: CH_KR_CHUNK elements of a plane per workgroup
constexpr int CH_KR_CHUNK = 2048;
struct KrChoice { unsigned gx, gy; int stream; };
static inline KrChoice choose_kr_stream(const LevShape &s) {
  const long long plane = (long long)s.nz * s.rs;
  return {(unsigned)((plane + CH_KR_CHUNK - 1) / CH_KR_CHUNK), (unsigned)(s.nx + 2), ch_beyond_cache(s)};
}

// ---- the transfers ----
// SK of the prolongations (k_coarse2fine_run explains it): the first colour's columns are left alone when the caller promises the
// four-colour relax that overwrites them (skip1), the correction is not kept in r, and the 2 x 2 blocks tile the fine level
static inline bool ch_skip_first_colour(const LevShape &F, int keep_r, int skip1) { return skip1 && !keep_r && !(F.nx & 1) && !(F.ny & 1); }
// run: k_coarse2fine_run (tri-linear), else k_coarse2fine_nearest; held: k_coarse2fine_held<WR, SK, run>.  kc: coarse levels per lane (run only)
struct C2fChoice { bool run, wr, sk; int kc, nt; unsigned gx, gy, gz, by; };
// (WR, SK) of their instances: SK only ever without WR
template <class F> static inline void with_wr_sk(bool wr, bool sk, F &&f) {
  if (wr) f(std::true_type{}, std::false_type{});
  else if (sk) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
// skip1: the caller guarantees that a four-colour relax of the fine level follows (cycles only)
static inline C2fChoice choose_coarse2fine(const LevShape &F, const LevShape &C, int linear, int keep_r, int skip1, const Switches &sw) {
  C2fChoice c;
  c.run = linear != 0; c.wr = keep_r != 0; c.sk = false; c.kc = 0;
  c.gx = (C.ny + CH_WAVE - 1) / CH_WAVE; c.gz = C.nx;
  c.nt = ch_beyond_cache(F);
  if (!c.run) {
    c.by = C.nz >= 4 ? 4 : C.nz; c.gy = (C.nz + c.by - 1) / c.by;
    return c;
  }
  // runs of KC coarse levels per lane: long enough to amortise the three-level window, short enough to keep >= ~2 waves per SIMD
  int KC = sw.c2f_kc > 0 ? sw.c2f_kc : 16;
  const long long wav = (long long)c.gx * C.nx;
  while (KC > 1 && wav * ((C.nz + KC - 1) / KC) < 2048) KC >>= 1;
  if (KC > C.nz) KC = C.nz;
  const int nrun = (C.nz + KC - 1) / KC;
  c.kc = KC; c.by = nrun >= 4 ? 4 : nrun; c.gy = (nrun + c.by - 1) / c.by;
  if (sw.c2f_nt >= 0) c.nt = sw.c2f_nt;  // A/B: the streaming hints forced on / off
  c.sk = ch_skip_first_colour(F, keep_r, skip1);
  return c;
}
// a held pair (mgx_hold.hip): one lane per coarse cell, rows independent, no cache hints
static inline C2fChoice choose_coarse2fine_held(const LevShape &F, const LevShape &C, int linear, int keep_r, int skip1) {
  C2fChoice c;
  c.run = linear != 0; c.wr = keep_r != 0; c.sk = ch_skip_first_colour(F, keep_r, skip1); c.kc = 0; c.nt = 0;
  c.gx = (C.ny + CH_WAVE - 1) / CH_WAVE; c.gy = (C.nz + 3) / 4; c.gz = C.nx; c.by = 4;
  return c;
}
// mgxk_residual_restrict_held (mgx_resrest_held.hip: k_residual_restrict_held): the down leg of a held pair (C.nz == F.nz, C half of F in x
// and y) as one kernel that never writes r.  The operator is the fine level's own (choose_operator_mf: matrix-free with its slopes, the stored
// slots otherwise -- bmask, a user matrix, MGX_NO_MF); a wave holds the four fine columns of 16 coarse columns, a workgroup four coarse
// planes: gx * gy workgroups, which are also the norm's pairs of partials.  Declined: an odd nz (the pairs of "hold_odd_nz" keep their two
// launches, to the count), MGX_NO_RESREST and fewer than MGX_RESREST_MIN fine cells (the A/B switches of the halving pairs' fused kernel).
// grid is filled in either way: mgx_init sizes the partials by it.
constexpr int CH_HELD_COLS = 16;   // coarse columns per wave: CH_WAVE / 4
struct HeldRrChoice { bool served, mf, real, norm; unsigned gx, gy, grid; int stream; };
static inline HeldRrChoice choose_resrest_held(const LevShape &f, const LevShape &c, int real, bool want_norm, const Switches &sw) {
  HeldRrChoice r;
  r.mf = choose_operator_mf(f); r.real = real != 0; r.norm = want_norm;
  r.gx = (c.ny + CH_HELD_COLS - 1) / CH_HELD_COLS; r.gy = (c.nx + 3) / 4; r.grid = r.gx * r.gy;
  r.stream = r.mf && ch_beyond_cache(f);
  r.served = !sw.no_resrest && c.nz == f.nz && f.nz >= 2 && !(f.nz & 1) && c.nx * 2 == f.nx && c.ny * 2 == f.ny && c.nx >= 1 && c.ny >= 1 &&
             (long long)f.nx * f.ny * f.nz >= sw.resrest_min;
  return r;
}
// mgxk_fine2coarse: grid.z runs of kc coarse levels -- enough waves (8192) to hide the latency of the eight loads of a level
struct F2cChoice { int kc; unsigned gx, gy, gz; int stream; };
static inline F2cChoice choose_fine2coarse(const LevShape &F, const LevShape &C) {
  F2cChoice c;
  c.gx = (C.ny + CH_WAVE - 1) / CH_WAVE; c.gy = (C.nx + 3) / 4;
  const long long waves = (long long)c.gx * c.gy * 4;
  long long nchunk = (8192 + waves - 1) / waves;
  if (nchunk > C.nz) nchunk = C.nz;
  if (nchunk < 1) nchunk = 1;
  c.kc = (int)((C.nz + nchunk - 1) / nchunk);
  c.gz = (C.nz + c.kc - 1) / c.kc;
  c.stream = ch_beyond_cache(F);
  return c;
}
// mgxk_restrict_chain: dep restrictions from the level `finest` down in one launch, a (2^dep)^3 block of it per workgroup.  Served: two to
// four restrictions (one is k_fine2coarse's) and nx, ny, nz of the finest level multiples of 2^dep.  Which levels may be chained at all
// (closed, not gathered, no held pair) is the cycle's business.  grid is filled in either way.
struct ChainChoice { bool served; unsigned grid; };
static inline ChainChoice choose_restrict_chain(const LevShape &finest, int dep) {
  const int E = 1 << (dep < 0 ? 0 : (dep > 4 ? 4 : dep));
  ChainChoice c;
  c.served = dep >= 2 && dep <= 4 && finest.nx % E == 0 && finest.ny % E == 0 && finest.nz % E == 0;
  c.grid = (unsigned)((finest.nx / E) * (finest.ny / E) * (finest.nz / E));
  return c;
}

// ---- halo and gather transport ----
constexpr int CH_HALO_PEER = 1;   // HALO_PEER of mgx_wrappers.h: another rank; above it the rank itself or a closed side's image, 0 = nothing due
// items of direction d (0 S, 1 E, 2 N, 3 W, 4.. the corners): one per cell of the edge
static inline int ch_halo_items(const LevShape &s, int d) { return s.nz * ((d == 0 || d == 2) ? s.nx : ((d == 1 || d == 3) ? s.ny : 1)); }
// mgxk_halo_wrap: nothing to do, or one launch whose x covers the longer of the plane copy and the row entries; nt: the level is streamed
struct WrapChoice { bool none; bool nt; unsigned grid; };
static inline WrapChoice choose_halo_wrap(const LevShape &s, int im, int jm) {
  WrapChoice c;
  c.none = !im && !jm;
  const long long plane = (long long)s.nz * s.rs;
  const long long npl = im ? (plane / 2 + 255) / 256 : 0, nj = jm ? ((long long)(s.nx + 2) * s.nz + 255) / 256 : 0;
  c.grid = (unsigned)(npl > nj ? npl : nj);
  c.nt = ch_beyond_cache(s);
  return c;
}
// mgxk_halo_pack_all: blockIdx.z = direction; mixed: a direction is served by the rank itself
struct PackChoice { bool mixed; unsigned gx, gy; };
static inline PackChoice choose_halo_pack(const LevShape &s, const int *present) {
  PackChoice c;
  c.mixed = false;
  for (int d = 0; d < 8; d++) c.mixed |= present[d] > CH_HALO_PEER;
  c.gx = ((s.nx > s.ny ? s.nx : s.ny) + 63) / 64; c.gy = s.nz;
  return c;
}
// mgxk_halo_p2p: the block plan of the one-launch exchange.  Blocks blk0[d] .. blk0[d+1]-1 of a compact 1-D grid of nb blocks serve direction
// d, ipt items per thread; absent directions sit past the end (blk0[d] = nb + 1: the kernel picks the LAST d with blk0[d] <= block index).
// nreal of them serve a real peer: they push, report in and wait, so all of them must be resident together, and a waiting wave, however
// light, keeps a 512-VGPR smoother wave off its SIMD: harmless when the GPU belongs to one rank (the smoother is behind us in the
// stream), fatal when several ranks share one GPU as in the tests (the neighbour's smoother would never start).  So the grid is kept
// small -- about maxblk = 128 blocks = 512 of the 1024 SIMDs -- and longer edges give each thread several items.
// The bound: per = 256 ipt > items / maxblk (the + 1), and nreal = sum over at most 8 peer directions of ceil(n_d / per)
// < items / per + 8, hence nreal <= maxblk + 7 (8 with maxblk = 1).  Not maxblk: 128 x 1738 x 2048 gives 130 and 128 x 4096 x 4096 with eight
// peers 132; nreal <= maxblk = 128 holds for every nx, ny <= 1024 with nz <= 128 (swept in tests/test_kernel_choice_host.py).  The
// blocks of a self or mirror direction only copy: they neither push nor spin, and do not count.
// mixed: such a direction is present (k_halo_exchange<true>).  Nothing is launched where nb == 0 || nreal == 0.
struct P2pPlan { int ipt, blk0[9], nb, nreal; bool mixed; };
static inline P2pPlan choose_halo_p2p(const LevShape &s, const int *present, const Switches &sw) {
  P2pPlan c;
  const int maxblk = sw.p2p_maxblk;  // default 128
  long long items = 0;
  for (int d = 0; d < 8; d++) if (present[d] == CH_HALO_PEER) items += ch_halo_items(s, d);
  c.ipt = (int)((items + 256LL * maxblk - 1) / (256LL * maxblk)) + 1;
  if (c.ipt < sw.p2p_ipt) c.ipt = sw.p2p_ipt;  // test hook for the multi-item path
  const int per = 256 * c.ipt;
  c.nb = 0; c.nreal = 0;
  for (int d = 0; d < 8; d++) {
    c.blk0[d] = c.nb;
    const int nd = present[d] ? (ch_halo_items(s, d) + per - 1) / per : 0;
    c.nb += nd;
    if (present[d] == CH_HALO_PEER) c.nreal += nd;
  }
  c.blk0[8] = c.nb;
  for (int d = 7; d >= 0; d--) if (!present[d]) c.blk0[d] = c.nb + 1;
  c.mixed = c.nreal != c.nb;
  return c;
}
// blocks of 256 threads over n items, at most cap (0 = as many as it takes)
static inline unsigned ch_blocks(long long n, int cap) { const long long nb = (n + 255) / 256; return (unsigned)(cap && nb > cap ? cap : nb); }
// mgxk_gather_push: every wave ends with a system-scope fence and every block with an atomic: few, fat blocks (256 at most)
static inline unsigned choose_gather_push(const LevShape &s) { return ch_blocks((long long)s.nz * (s.ny + 2) * (s.nx + 2), 256); }
// mgxk_gather_place_wait: blocks that may spin stay few (128, as choose_halo_p2p's)
static inline unsigned choose_gather_place_wait(int nz, int nxc, int nyc, bool wait) { return ch_blocks((long long)nz * nyc * nxc, wait ? 128 : 0); }

// ---- k_convert_slots: tile width 128 columns while the tile fits the LDS (nz <= 128), else the largest multiple of 16 that does ----
struct ConvChoice { int tj; size_t lds; unsigned gx, gy; };
static inline ConvChoice choose_convert_slots(const LevShape &s) {
  ConvChoice c;
  c.tj = 128;
  while (c.tj > 16 && (size_t)c.tj * (s.nz + 1) * sizeof(double) > 150 * 1024) c.tj -= 16;
  c.lds = (size_t)c.tj * (s.nz + 1) * sizeof(double);
  c.gx = (s.ny + 2 + c.tj - 1) / c.tj; c.gy = s.nx + 2;
  return c;
}

// ---- mgx_model.hip: rows per block in z of the kernels over ni x nj columns of klast rows ----
struct ModelChoice { int kr; unsigned gx, gy, gz; };
static inline ModelChoice ch_model_grid(int ni, int nj, int klast, int kr) { return {kr, (unsigned)((ni + 63) / 64), (unsigned)((nj + 3) / 4), (unsigned)((klast + kr - 1) / kr)}; }
// the divergence pass: eight
static inline ModelChoice choose_model_k(int ni, int nj, int klast) { return ch_model_grid(ni, nj, klast, klast >= 16 ? 8 : klast); }
// The flux kernels and correct_uvw carry values from row to row (a run re-reads one row of its neighbour run): runs as long as possible
// while there are >= 16 384 waves to hide the load -> use chain of a row (scripts/probe/ab_model_runs.sh at 512x512x64: runs of 16 rows
// 0.86 ms for the four kernels, 32 rows 0.91, whole columns 0.91).  MGX_MODEL_KR (A/B and test hook) asks for runs of that many rows, and
// gets them: the eight-row floor is the heuristic's, so that runs of 1..7 rows -- every row, or nearly, a run start that reloads the
// carried values -- can be forced too.
static inline ModelChoice choose_model_run(int ni, int nj, int klast, const Switches &sw) {
  const long long waves = (long long)((ni + 63) / 64) * nj;
  long long nrun = sw.model_kr > 0 ? (klast + sw.model_kr - 1) / sw.model_kr : (16384 + waves - 1) / waves;
  if (nrun < 1) nrun = 1;
  if (sw.model_kr <= 0 && nrun > (klast + 7) / 8) nrun = (klast + 7) / 8;  // at least eight rows per run
  return ch_model_grid(ni, nj, klast, (int)((klast + nrun - 1) / nrun));
}
