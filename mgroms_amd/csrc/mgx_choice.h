// Which kernel serves a level: the choices of the smoother wrappers (mgx_relax.hip, mgx_relax_coarse.hip, mgx_relax_ks.hip,
// mgx_relax_tall.hip), of the sequential-order red-black walk (mgx_rbseq.hip) and of the fused residual + restriction (mgx_resrest.hip)
// as pure host functions.  Each takes the level's shape, the call's flags and the A/B switches and returns a Choice by
// value: the kernel family, the parameters of its template instance, the launch geometry, and what the wrapper reports when the launch
// succeeded.  A wrapper is mgx_before_launch(), its choose_*(), and one launcher that maps the Choice to the instance (no condition on the
// level's shape there).  Nothing here calls HIP, keeps state or reads the environment; tests/test_kernel_choice_host.py pins every answer
// (DESIGN.md 4.9).  The choices of the units outside the smoother -- operator, transfers, transport, layout, model runs -- stand in
// mgx_choice_transfer.h, included at the end.
#pragma once
#include <cstddef>
#include <type_traits>
#include "mgx_internal.h"
#include "mgx_switches.h"

// slopes: the level has zy / zx (matrix-free cross terms); d0: the pass is to write d0w; gk: the level has what the sequential-order walk needs;
// zw: it carries all nine fields from which slots 4 and 7 are generated (as define_matrices leaves it: not after bmask, a user matrix or
// MGX_NO_MF); rs: the row stride of its layout
struct LevShape { int nx, ny, nz; bool slopes, d0, gk, zw; int rs; };
static inline LevShape lev_shape(const LevView *L) {
  return {L->nx, L->ny, L->nz, L->zy != nullptr, L->d0w != nullptr, L->gk != nullptr,
          L->m4 && L->d4 && L->m7 && L->d7 && L->h2 && L->hi2 && L->ze2 && L->cffw && L->csw, L->RS};
}

enum KernelFamily {
  KF_NONE,                               // nothing of this wrapper serves the call
  KF_WAVE, KF_REG, KF_TINY, KF_SMALL,    // a whole relax call in one workgroup: k_relax_wave, k_relax_reg, k_relax_tiny, k_relax_small
  KF_KS, KF_KS2,                         // k-split colour pass and colour pair: k_relax_ks, k_relax_ks2
  KF_NZ, KF_TALL, KF_TALL_ST, KF_COLOUR, // a colour pass: k_relax_nz, k_relax_tall, k_relax_tall_st, k_relax_colour
  KF_GS, KF_GS_ANY,                      // a hyperplane of the Gauss-Seidel sweep: k_relax_gs_front, k_relax_gs_front_any
  KF_RB_SCAN, KF_RB_SCAN_FUSED,          // the sequential-order walk over a level, alone or with the correction in its launch: k_rbseq_scan
  KF_RB_WALK_APPLY, KF_RB_WINDOW, KF_RB_APPLY,  // walk + correction of a small level, the windowed walk, the correction alone: k_rbseq_walk_apply, _window, _apply
  KF_RR_FLAT, KF_RR_WALK,                // residual + restriction, a wave per S fine rows or walking up the column: k_residual_restrict_flat, k_residual_restrict
  KF_RELAX32, KF_RELAX32R,               // the fp32 colour pass, row by row or with its rows in register rings: k_relax32, k_relax32r (mgx_mixed.hip)
  KF_DIRECT32,                           // the coarsest solve of an fp32 cycle as one product: k_coarse_direct32 (mgx_mixed.hip)
};

struct Choice {
  int family = KF_NONE;
  // the instance: NZ; MAXT (k_relax_reg, k_relax_small), NT (k_relax_wave) or NW (k_relax_ks, k_relax_ks2); D (k_relax_nz, tall) or H (k_relax_ks)
  int nz = 0, nt = 0, d = 0;
  bool mf = false, stream = false, fz = false, seq = false;
  // the launch: grid.x (gy: grid.y), block, dynamic LDS bytes, and the block map's gx (colour passes: negative = plain block order)
  unsigned grid = 1, gy = 1, bx = 1, by = 1;
  size_t lds = 0;
  int gx = 0;
  int ret = 0;        // what the wrapper reports when the launch went through
  int ask_wave = -1;  // mgxk_relax_small: >= 0 = mgxk_relax_wave is asked first, with this `any`; the call then reports wave_ret
  int wave_ret = 0;
};

constexpr int CH_WAVE = 64;   // lanes of a wave
static inline bool ch_closed(const Sides &ph) { return ph.S && ph.E && ph.N && ph.W; }
static inline int ch_chunks(int ny) { return (ny / 2 + CH_WAVE - 1) / CH_WAVE; }   // waves along a colour's half-row

// ---- run-time values as template arguments (the launchers) ----
// f(std::integral_constant<int, NZ>) for the NZ of the list that equals nz; false = none does
template <int... NZ, class F> static inline bool with_nz(int nz, F &&f) { return ((nz == NZ && (f(std::integral_constant<int, NZ>{}), true)) || ...); }
template <int... V, class F> static inline bool with_int(int v, F &&f) { return with_nz<V...>(v, static_cast<F &&>(f)); }   // the same for any other parameter
template <class F> static inline void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// (REAL, SNAP) and (REAL, SEQ) of the kernels: the second only ever with the first
template <class F> static inline void with_real_and(bool real, bool second, F &&f) {
  if (real && second) f(std::true_type{}, std::true_type{});
  else if (real) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::false_type{});
}
// (MF, ST): streaming hints only on the matrix-free instances
template <class F> static inline void with_mf_stream(bool mf, bool stream, F &&f) { with_real_and(mf, stream, static_cast<F &&>(f)); }

// ---- mgxk_relax_wave, mgxk_relax_wave_fused, mgxk_coarse_direct_build: k_relax_wave ----
// A closed level of <= 256 columns with nz = 2 (the coarsest grid of every BASELINE configuration) as one wave, or of <= 1024 columns with
// nz = 2 / 4 (the 32x32x4 level above it) as four waves, or -- nz = 2 only -- of <= 2048 columns as eight waves: the 64x32x2 coarsest grid
// that eight GPUs gather (4x2 ranks of 512x512x64: its 40 sweeps took 436 us in k_relax_small, which re-reads every operand through L2, a
// fifth of a V-cycle on every rank).
// mode (red-black with cmatrix='real' only): 0 = parallel colour passes, 1 = the bit-exact plane loop (not here: k_relax_reg), 2 = the
// reference's sequential order by the walk (k_relax_wave's seq)
// flags: transfers folded in (nz = 4 only); nbatch: independent solves, one workgroup each
// any (option "small_any_nz"): nz = 3 is served too -- four columns of three rows per lane, up to 256 blocks of 2x2 columns; never with folded transfers
static inline Choice choose_wave(const LevShape &s, int method, int real, const Sides &ph, int mode, int flags, int nbatch, int any, const Switches &sw) {
  Choice c;
  const bool nz3 = any && s.nz == 3 && !(flags & 3);
  if (sw.no_wave || (s.nz != 2 && s.nz != 4 && !nz3) || method == 0 || (mode == 1 && method == 1 && real)) return c;
  const bool seq = mode == 2 && method == 1 && real;
  if (seq && s.ny / 2 > CH_WAVE) return c;  // the walk keeps a half-row on the lanes of one wave; wider levels: k_relax_reg's plane loop
  const int nblk = (s.nx / 2) * (s.ny / 2);
  if (!ch_closed(ph) || (s.nx & 1) || (s.ny & 1) || nblk > (s.nz == 2 ? 8 : 4) * CH_WAVE) return c;
  size_t bytes = ((size_t)s.nz + 1) * (s.nx + 2) * (s.ny + 2) * sizeof(double);
  if (seq) {  // p, the snapshot, the operand quads (+ a zero quad), g, the register walk's d0 / s rows: interiors only
    bytes = ((2 * (size_t)s.nz + 5) * s.nx * s.ny + 4 + 64 * 18) * sizeof(double);
    if (bytes > 160 * 1024) return c;
  }
  if ((flags & 3) && s.nz != 4) return c;
  c.family = KF_WAVE; c.nz = s.nz; c.fz = (flags & 3) != 0; c.seq = seq;
  c.nt = nblk <= CH_WAVE ? 64 : (nblk <= 4 * CH_WAVE || s.nz != 2 ? 256 : 512);
  c.grid = nbatch; c.bx = c.nt; c.lds = bytes; c.ret = 1;
  return c;
}
// relax(lev, nsweeps) with coarse2fine(lev) folded in front (flags & 1) and / or compute_residual(lev) + fine2coarse(lev) folded behind
// (flags & 2); coarse = level lev+1 (closed, exactly half the size, not gathered), nullptr = none
static inline Choice choose_wave_fused(const LevShape &s, const LevShape *coarse, int nsweeps, int method, int real, const Sides &ph, int flags, int mode, const Switches &sw) {
  if (sw.no_wave_fuse || !coarse || coarse->nx * 2 != s.nx || coarse->ny * 2 != s.ny || coarse->nz * 2 != s.nz || nsweeps < 0) return Choice();
  return choose_wave(s, method, real, ph, mode, flags, 1, 0, sw);
}
// cells of a level the direct solve serves (a closed level of the one-workgroup kernel, at most 2048 cells), 0 = none; any: nz = 3 too
static inline int choose_coarse_direct_cells(const LevShape &s, int any) {
  const long long n = (long long)s.nx * s.ny * s.nz;
  return ((s.nz == 2 || s.nz == 4 || (any && s.nz == 3)) && n <= 2048 && !(s.nx & 1) && !(s.ny & 1)) ? (int)n : 0;
}

// ---- mgxk_relax_small: what serves a small level where k_relax_wave does not ----
// mode (red-black with cmatrix='real'): 0 = parallel colour passes (snapshot), 1 = the reference's plane loop bit for bit (rb_exact), 2 = the
// same order by the walk of mgx_rbseq.hip where a kernel has it (k_relax_wave), else the plane loop
// any (option "small_any_nz"): a closed level of at most 1024 columns with nz = 3, 5, 6 or 7 and even nx, ny is served too, and the call then
// reports 2 -- nz = 3 by k_relax_wave where it takes the mode, every other case by k_relax_reg up to 256 columns and by k_relax_small above
// (a 512- or 1024-thread k_relax_reg would have 128 or 64 registers per thread for 16 nz coefficients: the operands are re-read through L2)
static inline Choice choose_small(const LevShape &s, int method, int real, const Sides &ph, int mode, int any, const Switches &sw) {
  Choice c;
  const bool closed = ch_closed(ph), exact = mode != 0;
  const int ncols = s.nx * s.ny;
  const size_t reg_bytes = ((size_t)s.nz + 1) * (s.nx + 2) * (s.ny + 2) * sizeof(double);   // k_relax_reg: p and the k=1 snapshot, halo included
  const unsigned reg_threads = (ncols + 63) / 64 * 64;
  c.nz = s.nz;
  if (any && (s.nz == 3 || (s.nz >= 5 && s.nz <= 7))) {
    if (!closed || method == 0 || (s.nx & 1) || (s.ny & 1) || ncols > 1024) return c;
    if (s.nz == 3) { c.ask_wave = 1; c.wave_ret = 2; }  // not the plane loop of rb_exact, nor the walk of a half-row wider than a wave
    // Declined by measurement (profiles/small_any_nz_time.json): the sequential order at speed where only the plane loop could
    // serve it -- 2 nx barrier steps per sweep with one plane's columns at work lose against the colour pass and its walk, or only draw with
    // them -- except nz = 5 in one wave (8 x 8 x 5: 57-63 us against 98-99 for 3 sweeps); and 'simple' red-black at nz = 6, 7 above 256
    // columns (k_relax_small at 32 x 32 x 7: 961-977 us against 877-901 for 40 sweeps; at nz = 6 a draw)
    if (method == 1 && real && mode == 2 && !(s.nz == 5 && ncols <= 64)) return c;
    if (method == 1 && !real && s.nz >= 6 && ncols > 256) return c;
    c.nt = 256; c.ret = 2;
    if (ncols <= 256) { c.family = KF_REG; c.bx = reg_threads; c.lds = reg_bytes; }
    else { c.family = KF_SMALL; c.bx = 256; }
    return c;
  }
  c.ask_wave = 0; c.wave_ret = 1;  // <= 256 columns, nz = 2: the whole level in one wave
  c.ret = 1;
  // one thread per column, coefficients in registers, p in LDS
  if (!sw.no_reg && closed && method != 0 && ((s.nz == 2 && ncols <= 1024) || (s.nz == 4 && ncols <= 256))) {
    c.family = KF_REG; c.nt = s.nz == 2 ? 1024 : 256; c.bx = reg_threads; c.lds = reg_bytes;
    return c;
  }
  // everything in LDS? (11 arrays of the compact level + the k=1 snapshot)
  const size_t n3 = (size_t)(s.nx + 2) * (s.ny + 2) * s.nz, tiny_bytes = (11 * n3 + (size_t)(s.nx + 2) * (s.ny + 2)) * sizeof(double);
  const int ncol = method == 2 ? (s.nx / 2) * (s.ny / 2) : s.nx * (s.ny / 2);   // columns of a colour
  if (!sw.no_tiny && !(exact && method == 1 && real) && tiny_bytes <= 64 * 1024 && closed && (s.nz == 2 || s.nz == 4)) {
    c.family = KF_TINY; c.bx = ncol <= 64 ? 64 : 256; c.lds = tiny_bytes;
    return c;
  }
  // (Measured and dropped: one cooperative launch per relax call with a grid-wide barrier between colour passes on the
  // 1024-16384-column levels -- cg grid.sync and a hand-written atomic barrier both cost more than the kernel boundary
  // they replace: V-cycle 2.81 -> 3.03 ms.)
  // one CU streams ~25-50 GB/s: worth it only while the level is launch-bound, not bandwidth-bound (measured:
  // 16x16x2 and 32x32x4 win, 64x64x8 loses 2x against separate launches over 256 CUs).  A 2-level-deep coarsest grid
  // is still launch-bound at 1024 columns per colour (the gathered 64x32x2 grid of an 8-GPU run): 1024 threads.
  if (!closed) return c;
  if (s.nz == 2 && ncol > 256 && ncol <= 1024) { c.family = KF_SMALL; c.nt = 1024; c.bx = 1024; return c; }
  if (ncol > 256 || s.nz > 8) return c;
  // 32x32x8 (fifth level of an nz = 128 hierarchy), four colours: two colour-pair launches per sweep (k_relax_ks2, 5.9 us each) beat this
  // kernel's 22-32 us per sweep, which re-reads every operand through L2
  if (s.nz == 8 && method == 2 && s.slopes && ncol > 64 && s.ny / 2 <= CH_WAVE) return c;
  if (s.nz != 2 && s.nz != 4 && s.nz != 8) return c;
  c.family = KF_SMALL; c.nt = 256; c.bx = ncol <= 64 ? 64 : 256;
  return c;
}

// ---- the colour passes ----
// the launch geometry the register-resident passes share (k_relax_nz, k_relax_tall, k_relax_tall_st): one wave per 64 columns of a plane
static inline void ch_pass_geometry(Choice &c, const LevShape &s, int nplanes, const Switches &sw) {
  const int gx0 = ch_chunks(s.ny);
  c.gx = sw.no_xcd ? -gx0 : gx0;
  // two planes per workgroup only when there are plenty of workgroups (it halves the number of CUs a small level uses)
  c.by = gx0 * nplanes >= 2048 ? 2 : 1;
  c.bx = CH_WAVE; c.grid = gx0 * ((nplanes + c.by - 1) / c.by);
}
// streaming (nontemporal) hints only when the level cannot live in the 256 MB Infinity Cache between passes:
// measured +14 % on the 1.2 GB level 1, -20 % on the 150 MB level 2 which is otherwise re-read from cache
// (level_streams of mgx_device.h, the per-launch form of the hint, is this function)
static inline bool ch_beyond_cache(const LevShape &s) { return (double)s.nx * s.ny * s.nz * 72.0 > 256e6; }
static inline int ch_pass_ret(const LevShape &s, int real, int snap) { return (real && snap && s.d0) ? PASS_MIRRORS | PASS_D0 : PASS_MIRRORS; }

// mgxk_relax_ks: the mid levels, rows split over the waves of a workgroup
static inline Choice choose_ks(const LevShape &s, int nplanes, int real, int snap, const Switches &sw) {
  Choice c;
  if (sw.no_ks || !s.slopes || (s.nz != 32 && s.nz != 16 && !(s.nz == 8 && sw.ks8) && !(s.nz == 64 && sw.ks64 && !snap))) return c;
  const int gx0 = ch_chunks(s.ny);
  // worth it only while a colour has fewer waves than the chip has SIMDs (1024); a bandwidth-bound level keeps one wave per column set
  if (gx0 * nplanes > 512) return c;
  // the level must live in the caches (no streaming hints here)
  c.family = KF_KS; c.nz = s.nz; c.gx = sw.no_xcd ? -gx0 : gx0;
  // measured (256x256x32 / 128x128x16, four-colour sweep): 8 waves 47.0 / 21.6 us, 4 waves 53.3 / 23.3, row by row 57.6 / 28.2
  c.nt = s.nz != 64 && sw.ks_nw == 4 ? 4 : 8;
  c.d = s.nz == 64 ? 2 : 1;   // H; at nz = 64 the 96 KB of dynamic LDS are above the 64 KB a kernel gets without asking
  c.grid = gx0 * nplanes; c.bx = CH_WAVE; c.by = c.nt; c.lds = (size_t)3 * s.nz * CH_WAVE * sizeof(double);
  c.ret = ch_pass_ret(s, real, snap);
  return c;
}
// mgxk_relax_ks_pair: both colours of the planes i0, i0+2, ... of a four-colour sweep in one launch (closed level, one column set per plane)
static inline Choice choose_ks_pair(const LevShape &s, int nplanes, const Sides &ph, const Switches &sw) {
  Choice c;
  if (sw.no_ks || sw.no_ks2 || !s.slopes || !ch_closed(ph) || (s.ny & 1) || s.ny / 2 > CH_WAVE) return c;
  if (s.nz != 16 && s.nz != 8) return c;
  c.family = KF_KS2; c.nz = s.nz; c.nt = 8; c.grid = nplanes; c.bx = CH_WAVE; c.by = 8; c.ret = 1;
  return c;
}
// mgxk_relax_tall: nz = 128 (BASELINE config 5), 96 and 80, lower 64 rows through LDS: the matrix-free form where the level has its slopes,
// the stored-coefficient form where it has not (PASS_TALL_STORED: what relax() counts as "tall_stored_passes")
static inline Choice choose_tall(const LevShape &s, int nplanes, const Switches &sw) {
  Choice c;
  if ((s.nz != 128 && s.nz != 96 && s.nz != 80) || sw.no_tall) return c;
  c.family = s.slopes ? KF_TALL : KF_TALL_ST; c.nz = s.nz; c.mf = s.slopes; c.d = 3;  // look-ahead rows of both forms
  ch_pass_geometry(c, s, nplanes, sw);
  c.stream = ch_beyond_cache(s);
  c.lds = (size_t)c.by * 64 * CH_WAVE * sizeof(double);  // the lower 64 rows' forward values: 32 KB per wave
  c.ret = s.slopes ? PASS_MIRRORS : PASS_MIRRORS | PASS_TALL_STORED;
  return c;
}
// the nz of the register-resident instances of the colour pass (k_relax_nz): the powers of two, and the vertical sizes that are not (ROMS /
// CROCO users choose nz for their physics) with their coarser levels; nz = 80, 96, 128 are mgxk_relax_tall's.
// -DMGX_QUICK: only the nz = 64 instantiations (resource-usage checks of the level-1 kernel in seconds)
#ifdef MGX_QUICK
#define REG_NZ_LIST 64
#else
#define REG_NZ_LIST 2, 4, 8, 16, 32, 64, 12, 20, 24, 40, 48
#endif
// gam(k) of the matrix-free k_relax_nz waits in LDS instead of registers (GL, relax_col_mf): read by the kernel and by the choice that sizes its LDS
constexpr bool ch_gam_in_lds(int nz, bool mf) { return mf && nz == 64; }
template <int NZ, bool MF> constexpr bool gam_in_lds = ch_gam_in_lds(NZ, MF);
// look-ahead depth D of k_relax_nz (rows of loads in flight): read by the choice and by the launcher that names the instance
// measured: NZ=16 6.3 us/pass at D=2 vs 9.3 at D=3; NZ>=32 flat for D=2..5
constexpr int ch_colour_depth(int nz) { return nz >= 32 ? 3 : (nz >= 8 ? 2 : 1); }
// mgxk_relax_colour behind mgxk_relax_ks: the register-resident pass, the tall-column pass (asked through mgxk_relax_tall; refused there,
// the generic column takes the pass) or the generic column
static inline Choice choose_colour_generic(const LevShape &s, int nplanes) {
  Choice c;
  c.family = KF_COLOUR; c.grid = ch_chunks(s.ny); c.gy = (nplanes + 3) / 4; c.bx = CH_WAVE; c.by = 4; c.ret = 0;   // four planes per workgroup
  return c;
}
static inline Choice choose_colour(const LevShape &s, int nplanes, int real, int snap, const Switches &sw) {
  Choice c;
  const bool reg = with_nz<REG_NZ_LIST>(s.nz, [](auto) {});
  if (!reg) {
#ifndef MGX_QUICK
    c = choose_tall(s, nplanes, sw);
    if (c.family != KF_NONE) return c;
#endif
    return choose_colour_generic(s, nplanes);
  }
  c.family = KF_NZ; c.nz = s.nz;
  c.d = ch_colour_depth(s.nz);
  ch_pass_geometry(c, s, nplanes, sw);
  c.mf = s.slopes && s.nz >= 16;  // matrix-free cross terms on the bandwidth-bound levels
  c.stream = c.mf && ch_beyond_cache(s);
  c.lds = ch_gam_in_lds(s.nz, c.mf) ? (size_t)c.by * s.nz * CH_WAVE * sizeof(double) : 0;  // 32 KB per wave (GL, relax_col_mf)
  c.ret = ch_pass_ret(s, real, snap);
  return c;
}
// mgxk_has_reg_kernel: does the colour pass of this level store its own mirrors and chained snapshots?
static inline bool choose_has_reg_kernel(const LevShape &s, const Switches &sw) {
  const int f = choose_colour(s, 1, 0, 0, sw).family;
  return f == KF_NZ || f == KF_TALL || f == KF_TALL_ST;
}

// mgxk_relax_gs_sweep: hyperplane t = j + 2 i of the sweep -- register-resident columns for nz a power of two <= 64, any nz otherwise;
// grid = 0: the hyperplane holds no column
static inline Choice choose_gs_front(const LevShape &s, int t) {
  Choice c;
  int ilo = (t - s.ny + 1) / 2; if (ilo < 1) ilo = 1;
  int ihi = (t - 1) / 2; if (ihi > s.nx) ihi = s.nx;
  c.family = with_nz<2, 4, 8, 16, 32, 64>(s.nz, [](auto) {}) ? KF_GS : KF_GS_ANY;
  c.nz = s.nz; c.grid = ihi < ilo ? 0 : (ihi - ilo + 1 + CH_WAVE - 1) / CH_WAVE; c.bx = CH_WAVE; c.ret = 1;
  return c;
}

// ---- the operator of a level (mgxk_residual, mgxq_apply, mgxq_apply32, mgxq_path): matrix-free cross terms or the stored slots ----
static inline bool choose_operator_mf(const LevShape &s) { return s.slopes && s.nz >= 3; }

// ---- mgx_rbseq.hip: red-black in the reference's sequential order ----
struct RbChoice {
  int family = KF_NONE;
  // the instance: CPL, D, FULL, NW, D0IN of k_rbseq_scan (fused: FUSE = 2 with the snapshot written, else 1); KU of k_rbseq_apply; CPL, KR of k_rbseq_window
  int cpl = 0, d = 0, nw = 1, ku = 0, kr = 0;
  bool full = false, d0in = false;
  bool d0_first = false;   // k_rbseq_d0 runs in front of the walk: nobody has left d0 in u1
  // the launch and its scalar arguments
  unsigned grid = 1, gy = 1, gz = 1, bx = CH_WAVE, by = 1;
  size_t lds = 0;
  int nhelp = 0, nt = 0, nchunk = 0, nkz = 0, nworkers = 0;   // (nchunk: waves along a half-row -- k_rbseq_window's nch)
  int pb = 0, xmap = 0, prio = 0, kcut = 0;
  int ret = 0;
};
constexpr int RBF_CH = 8;     // planes per hand-off word of the fused walk (its ring holds whole chunks), RBF_WPB: waves of its workgroups
constexpr int RBF_WPB = 4;
constexpr int RBW_MAXM = 48;  // the windowed walk's longest warm-up (planes)

// rows per correction wave: enough waves to fill the chip on the large levels, whole columns on the small ones
static inline void ch_rbseq_apply_shape(const LevShape &s, int &ku, int &kr) {
  const int nyh = s.ny / 2, nz = s.nz;
  // (ku divides nz: an odd coarse level -- nz = 3 or 5 below nz = 24, 40, 48, 80, 96 -- takes one row at a time, or a wave would write
  // the row above its column's top, i.e. the bottom row of the next plane)
  ku = nz % 8 == 0 ? 8 : (nz % 4 == 0 ? 4 : (nz % 2 == 0 ? 2 : 1));
  kr = nz;
  const long long waves = (long long)ch_chunks(s.ny) * s.nx;
  while (kr > ku && kr % 2 == 0 && (kr / 2) % ku == 0 && waves * (nz / kr) < 4096) kr /= 2;
}
// mgxk_rbseq_apply: the correction (c) as a launch of its own
static inline RbChoice choose_rbseq_apply(const LevShape &s) {
  RbChoice c;
  c.family = KF_RB_APPLY;
  ch_rbseq_apply_shape(s, c.ku, c.kr);
  c.grid = ch_chunks(s.ny); c.gy = (s.nx + 3) / 4; c.gz = s.nz / c.kr; c.by = 4;
  c.nt = ch_beyond_cache(s);
  return c;
}

// Does the walk form d0 itself?  Small half-rows: one wave does (the level lives in L2; the walk is bound by its dependent chain, not by its
// requests) -- but half-rows of 65..128 columns whose pass wrote d0 read it: three requests and a store per plane, 16 planes of look-ahead
// instead of 8 with five: level 2 of 512x512x64 20.5 -> ~16 us per colour, Vcycle 3.12 -> 3.08 ms; MGX_RBSEQ_NO_D0_MID: A/B
static inline bool ch_rbseq_forms_d0(const LevShape &s, int have_d0, const Switches &sw) {
  const int nyh = s.ny / 2;
  return nyh <= 2 * CH_WAVE && !sw.rbseq_d0_kernel && !(have_d0 && sw.rbseq_d0_mid && nyh > CH_WAVE);
}
// the levels k_rbseq_walk_apply is made for
static inline bool ch_rbseq_walk_apply_size(const LevShape &s) { return s.ny / 2 <= CH_WAVE && s.nx <= 128; }
// the fused launch counts planes in 13 bits of its progress word
static inline bool ch_rbseq_fuse_planes(const LevShape &s) { return s.nx < (1 << 13); }
// The deepest ring of a row of the walk's ladder (CPL columns per lane, NW waves, d0 formed or read): D * (loads + stores per plane) < 63
// (vmcnt); the ring of a launch is the first of DMAX, 4, 2 that divides nx.  Read by the choice and by the launcher that names the instances.
constexpr int ch_rbseq_dmax(int cpl, int nw, bool d0in) {
  // d0 formed at CPL = 1: y, snapshot, the multiplier pair, the store of u -- 4 operations per plane, 16 planes deep
  return d0in ? (cpl == 1 ? 16 : 8) : (nw > 1 || cpl <= 2 ? 16 : (cpl == 4 ? 8 : (cpl == 8 ? 4 : 2)));
}
// mgxk_rbseq_scan, mgxk_rbseq_scan_apply: (b), d0 and the walk -- and, fuse (the caller has the hand-off words, an error word and a device
// whose placement suits; min_cells: cells of a colour from which on it wants the fused launch), the correction (c) inside the walk's launch
// where an instance exists (ret 2 then).  ret 0: the level has no instance (no gk, odd nx, more than 1024 columns per half-row): the
// caller runs the planes one by one.
static inline RbChoice choose_rbseq_scan(const LevShape &s, int have_d0, bool fuse, long long min_cells, const Switches &sw) {
  RbChoice c;
  const int nyh = s.ny / 2, nx = s.nx;
  if (!s.gk || nyh > 16 * CH_WAVE || (nx & 1)) return c;
  // helper workgroups that pull the walk's operands into its L2 (k_rbseq_scan): one per ~32 KB of operands, at most 32 (one per compute unit of an XCD)
  // Measured (512x512x64, rocprofv3): level 1 (4.2 MB of operands, HBM-resident) one wave 88.4 us without helpers, 59.7 with 32; two waves
  // (a barrier per plane) 73; levels 2-4 (1 MB and less) 20.9 / 11.0 / 7.6 us with or without them -- there the walk is bound by the ~190
  // cycles a plane step costs to issue (4-5 memory instructions, the dependent DPP + FMA chain), and a few dozen extra workgroups only add
  // launch time (level 4: 9.0 against 7.6).  So: helpers from 2 MB of operands on.
  const long long opbytes = (long long)nx * nyh * 32;
  c.nhelp = opbytes >= (2LL << 20) ? (int)((opbytes + 131071) / 131072) : 0;
  if (c.nhelp > 32) c.nhelp = 32;
  if (c.nhelp > nx) c.nhelp = nx;
  // the row of the ladder
  if (ch_rbseq_forms_d0(s, have_d0, sw)) { c.d0in = true; c.cpl = nyh <= CH_WAVE ? 1 : 2; }
  else {
    c.d0_first = !have_d0;   // (the colour pass may have written it: LevView::d0w)
    // wide half-rows: the requests of ONE wave (at most 63 in flight) do not cover the latency of a level that lives in HBM: several waves
    // (256 columns per half-row: ONE wave with the helpers beats two waves with a barrier per plane, 59.7 against 73 us; wider half-rows
    // -- 512 and 1024 columns, BASELINE config 5 -- would need 16 / 32 memory instructions per plane in one wave: several waves there, unmeasured)
    if (nyh <= CH_WAVE) c.cpl = 1;
    else if (nyh <= 2 * CH_WAVE) c.cpl = 2;
    else if (nyh == 8 * CH_WAVE) { c.cpl = 2; c.nw = 4; }
    else if (nyh == 16 * CH_WAVE) { c.cpl = 2; c.nw = 8; }
    else c.cpl = nyh <= 4 * CH_WAVE ? 4 : (nyh <= 8 * CH_WAVE ? 8 : 16);
  }
  const int dmax = ch_rbseq_dmax(c.cpl, c.nw, c.d0in);
  c.d = nx % dmax == 0 ? dmax : (nx % 4 == 0 ? 4 : 2);
  c.full = nyh == c.cpl * CH_WAVE * c.nw;
  // the correction inside the walk's launch: instances for full half-rows of one walking wave, the deepest ring in whole chunks, nz a multiple of 8
  // ... and where it pays: the correction of a colour is 24 B per cell; below ~100 MB it takes less than what the hand-off adds (the
  // forwarding waves lag the walk by 2-5 us, the last workers finish ~4 us later: 256x256x32, 0.111 ms per sweep fused against 0.099)
  int ku, kr;
  ch_rbseq_apply_shape(s, ku, kr);
  const bool can_fuse = fuse && ku == 8 && (long long)(nx + 2) * s.rs * 8 < (1LL << 31) && (long long)nx * nyh * s.nz >= min_cells;
  if (can_fuse && c.nw == 1 && c.full && c.d == dmax && dmax % RBF_CH == 0) {
    c.family = KF_RB_SCAN_FUSED;
    // eight rows per worker: what a worker does after its word is set -- 16 stores with the mirrors, ~1.4 us per eight rows under load --
    // is the tail of the launch behind the walk's last plane (level-1 sweep at 512x512x64 with 32 / 16 / 8 rows: 0.346 / 0.345-0.357 / 0.339 ms)
    c.kr = 8; c.nt = ch_beyond_cache(s); c.nchunk = ch_chunks(s.ny); c.nkz = s.nz / c.kr; c.nworkers = nx * c.nchunk * c.nkz;
    // workgroup b holds RBF_WPB workers unless b % 8 == 0 (those: the walk with its forwarding waves, the helpers, nothing)
    const int per = 7 * RBF_WPB, octets = (c.nworkers + per - 1) / per;
    c.grid = 8 * (octets > c.nhelp + 3 ? octets : c.nhelp + 3); c.bx = CH_WAVE * RBF_WPB; c.ret = 2;
    return c;
  }
  c.family = KF_RB_SCAN; c.grid = 1 + 8 * c.nhelp; c.bx = CH_WAVE * c.nw; c.ret = 1;
  return c;
}
// mgxk_rbseq_walk_apply: (b) + (c) of a small level in ONE launch; needs d0 in u1 (the colour pass wrote it)
static inline RbChoice choose_rbseq_walk_apply(const LevShape &s, const Switches &sw) {
  RbChoice c;
  if (sw.no_rbseq_walk_apply || !s.gk || !ch_rbseq_walk_apply_size(s) || (s.nx & 1) || s.nz < 4 || (s.nz & 3)) return c;
  c.family = KF_RB_WALK_APPLY; c.d = 16;   // DW: planes of look-ahead
  c.pb = s.nx > 64 ? (s.nx + 63) / 64 : 1; c.grid = (s.nx + c.pb - 1) / c.pb; c.bx = 256;
  c.lds = (size_t)(s.nx + c.d + 1) * 64 * sizeof(double);
  c.nt = ch_beyond_cache(s); c.ret = 1;
  return c;
}
// mgxk_rbseq_wants_d0: does the walk of this level read d0 from u1 rather than form it itself?  Then the colour pass should write it
// (LevView::d0w).  Wide half-rows: k_rbseq_scan reads it; small levels: k_rbseq_walk_apply needs it where no workgroup of its launch writes.
// By the two predicates the choices above stand on, not by their families: it also says yes where neither then serves the level.
static inline bool choose_rbseq_wants_d0(const LevShape &s, const Switches &sw) {
  return s.gk && (!ch_rbseq_forms_d0(s, 1, sw) || ch_rbseq_walk_apply_size(s));
}
// mgxk_rbseq_window: (b) + (c) by the windowed walk; m: planes of warm-up (mgxk_rbseq_window_planes), kcut: rows the correction reaches
static inline RbChoice choose_rbseq_window(const LevShape &s, int m, int kcut, const Switches &sw) {
  RbChoice c;
  const int nyh = s.ny / 2, nz = s.nz;
  if (!s.gk || m < 1 || m > RBW_MAXM || nyh < 1 || (s.ny & 1) || s.nx > 65535) return c;
  int kr = nz % 64 == 0 ? 16 : (nz % 32 == 0 ? 8 : (nz % 16 == 0 ? 4 : (nz % 8 == 0 ? 2 : (nz % 4 == 0 ? 1 : 0))));
  if (!kr || nz / (4 * kr) > 65535) return c;
  if (kcut < 1 || kcut > nz) kcut = nz;
  // the rows the correction reaches, spread over the four row waves of a workgroup (16 of 64 rows: four rows per wave rather than one wave with all
  // sixteen and three idle), and only the row groups that hold any are launched
  while (kr > 1 && 4 * (kr / 2) >= kcut) kr /= 2;
  c.family = KF_RB_WINDOW; c.kr = kr; c.kcut = kcut;
  // the walking wave at raised priority (s_setprio 3): level-1 sweep 0.3075-0.3150 -> 0.2989-0.3073 ms (three runs each, alternating); MGX_RBW_PRIO=0: A/B
  c.prio = sw.rbw_prio;
  c.nt = ch_beyond_cache(s); c.cpl = nyh <= CH_WAVE ? 1 : 2; c.nchunk = ch_chunks(s.ny); c.nkz = (kcut + 4 * kr - 1) / (4 * kr);
  c.xmap = !sw.rbseq_window_no_xmap && s.nx % 8 == 0 && (long long)c.nchunk * s.nx * c.nkz < (1LL << 31);
  if (c.xmap) c.grid = c.nchunk * s.nx * c.nkz;
  else { c.grid = c.nchunk; c.gy = s.nx; c.gz = c.nkz; }
  c.bx = 320; c.ret = 1;
  return c;
}

// ---- mgx_resrest.hip: mgxk_residual_restrict_ex ----
struct RrChoice {
  int family = KF_NONE;
  int s = 0, aw = 0, ar = 0;   // S of k_residual_restrict_flat; AW, AR of k_residual_restrict
  bool real = false, norm = false, zw = false;
  unsigned grid = 0, by = 1;   // workgroups (= the norm's pairs of partials): filled in whether or not the launch is served -- define_matrices sizes the partials by it
  int gx = 0, gy = 0;
};
// served: matrix-free slopes present, even nz, a coarse level of half the size, from resrest_min fine cells on
static inline RrChoice choose_resrest(const LevShape &f, const LevShape &c, int real, bool want_norm, const Switches &sw) {
  RrChoice r;
  const long long cells = (long long)f.nx * f.ny * f.nz;
  const bool served = !sw.no_resrest && f.slopes && f.nz >= 2 && !(f.nz & 1) && c.nx * 2 == f.nx && c.ny * 2 == f.ny && cells >= sw.resrest_min;
  r.real = real; r.norm = want_norm;
  r.gx = (c.ny + 31) / 32;
  if (cells <= sw.resrest_flat_max) {  // no walk: one wave per S fine rows, one round trip
    r.s = sw.resrest_flat_s >= 4 && f.nz >= 4 ? 4 : 2;
    r.grid = (unsigned)r.gx * c.nx * ((f.nz + r.s - 1) / r.s);
    if (served) r.family = KF_RR_FLAT;
    return r;
  }
  r.by = 4; r.gy = (c.nx + r.by - 1) / r.by; r.grid = r.gx * r.gy;
  // resrest_ahead = 10 * AW + AR, default 11 (A/B: scripts/probe/ab_resrest_ahead.sh -- 11, 12, 21 within 5 % of each other once the requests are unconditional)
  r.aw = sw.resrest_ahead == 21 ? 2 : 1; r.ar = sw.resrest_ahead == 12 ? 2 : 1;
  // slots 4 and 7 generated: when the level carries what the smoother's ZW form needs; the instance without the norm at the default
  // look-ahead only (the others have no registers for it)
  r.zw = r.aw == 1 && r.ar == 1 && !sw.resrest_no_zw && !want_norm && f.zw;
  if (served) r.family = KF_RR_WALK;
  return r;
}

// ---- mgx_mixed.hip: mgxx_relax_pass, the colour pass of the fp32 cycles ----
static inline LevShape lev_shape32(const LevView32 *L) { return {L->nx, L->ny, L->nz, false, false, false, false, L->RS}; }
// the nz of the instances of k_relax32r (option "mixed_ring"); the register instances of k_relax32, every other nz taking its generic form
#define RING_NZ_LIST 16, 20, 24, 32, 40, 48, 64
#define RELAX32_NZ_LIST 2, 4, 8, 16, 32, 64
// look-ahead depth D of k_relax32r: 19 loads per row and at most 63 in flight per wave, so 3 rows is the most a ring can hold ahead; the
// fp64 answer (ch_colour_depth) from nz = 16 on.  Measured at 512x512x64: D = 2 on every level is a draw with this.
// Read by the choice and by the launcher that names the instance, as ch_colour_depth is: D is a function of NZ alone.
constexpr int ch_ring_depth(int nz) { return nz >= 32 ? 3 : 2; }
// ch_beyond_cache counts the 72 B per cell of the fp64 pass; the fp32 pass moves half of that.  Measured: without the hints the level-1
// passes of an iteration at 512x512x64 take 0.19-0.21 ms more.
static inline bool ch_ring_beyond_cache(const LevShape &s) { return (double)s.nx * s.ny * s.nz * 36.0 > 256e6; }
// ring (option "mixed_ring"): a level that is not small (mixed_tail_small: the small ones are launch-bound, and the tail kernel owes them
// k_relax32's bits) and whose nz has an instance takes k_relax32r in the geometry of the fp64 register passes; anything else, and every
// level with ring = 0, k_relax32 with four planes per workgroup.  ret: 1 = the pass counts as a "mixed_ring_passes"
static inline Choice choose_relax32(const LevShape &s, int nplanes, int real, int snap, int ring, const Switches &sw) {
  Choice c;
  if (ring && with_nz<RING_NZ_LIST>(s.nz, [](auto) {}) && !mixed_tail_small(s.nx, s.ny, s.nz)) {
    c.family = KF_RELAX32R; c.nz = s.nz; c.d = ch_ring_depth(s.nz);
    ch_pass_geometry(c, s, nplanes, sw);
    c.stream = ch_ring_beyond_cache(s);
    c.ret = 1;
    return c;
  }
  c.family = KF_RELAX32; c.nz = with_nz<RELAX32_NZ_LIST>(s.nz, [](auto) {}) ? s.nz : 0;
  c.grid = ch_chunks(s.ny); c.gy = (nplanes + 3) / 4; c.bx = CH_WAVE; c.by = 4;
  return c;
}

// ---- mgx_mixed.hip: mgxx_coarse_direct32, the coarsest solve of the fp32 cycles as one product (option "mixed_direct") ----
// cells of the coarsest level (shape s) of a hierarchy of nlevs levels that the product serves, 0 = the sweeps: the rule of the fp64 direct
// solve (choose_coarse_direct_cells) on a level that is entered from a restriction, i.e. not the only one
static inline int choose_mixed_direct_cells(const LevShape &s, int nlevs, int any) { return nlevs >= 2 ? choose_coarse_direct_cells(s, any) : 0; }
// The product e = B f of n rows is cut into tiles of 64 rows and, along the columns, into S slabs of cps columns whose partial sums meet in
// LDS: S is as many as 8192 partial sums hold for the padded row count, 16 at the most -- a function of n alone, and with it the order in
// which the terms of a row are added (direct32_rows), whatever launch runs the items.
constexpr int DIRECT32_MAX_N = 2048, DIRECT32_PART = 8192, DIRECT32_MAX_SLABS = 16;
// (constexpr: the kernel reads them too)
constexpr int ch_direct32_tiles(int n) { return (n + CH_WAVE - 1) / CH_WAVE; }
constexpr int ch_direct32_slabs(int n) { const int s = DIRECT32_PART / (ch_direct32_tiles(n) * CH_WAVE); return s < DIRECT32_MAX_SLABS ? s : DIRECT32_MAX_SLABS; }
// the stand-alone launch: one workgroup per tile of 64 rows, one wave per slab
static inline Choice choose_coarse_direct32(const LevShape &s, int nlevs, int any) {
  Choice c;
  const int n = choose_mixed_direct_cells(s, nlevs, any);
  if (!n) return c;
  c.family = KF_DIRECT32; c.nz = s.nz; c.nt = n; c.d = ch_direct32_slabs(n);
  c.grid = ch_direct32_tiles(n); c.bx = CH_WAVE * c.d; c.ret = 1;
  return c;
}

// ---- the units outside the smoother: operator, transfers, transport, layout, model runs ----
#include "mgx_choice_transfer.h"
