// Which kernel smooths a level: the choices of the smoother wrappers (mgx_relax.hip, mgx_relax_coarse.hip, mgx_relax_ks.hip,
// mgx_relax_tall.hip) as pure host functions.  Each takes the level's shape, the call's flags and the A/B switches and returns a Choice by
// value: the kernel family, the parameters of its template instance, the launch geometry, and what the wrapper reports when the launch
// succeeded.  A wrapper is mgx_before_launch(), its choose_*(), and one launcher that maps the Choice to the instance (no condition on the
// level's shape there).  Nothing here calls HIP, keeps state or reads the environment; tests/test_kernel_choice_host.py pins every answer
// (DESIGN.md 4.9).
#pragma once
#include <cstddef>
#include <type_traits>
#include "mgx_internal.h"
#include "mgx_switches.h"

struct LevShape { int nx, ny, nz; bool slopes, d0; };   // slopes: the level has zy / zx (matrix-free cross terms); d0: the pass is to write d0w
static inline LevShape lev_shape(const LevView *L) { return {L->nx, L->ny, L->nz, L->zy != nullptr, L->d0w != nullptr}; }

enum KernelFamily {
  KF_NONE,                               // nothing of this wrapper serves the call
  KF_WAVE, KF_REG, KF_TINY, KF_SMALL,    // a whole relax call in one workgroup: k_relax_wave, k_relax_reg, k_relax_tiny, k_relax_small
  KF_KS, KF_KS2,                         // k-split colour pass and colour pair: k_relax_ks, k_relax_ks2
  KF_NZ, KF_TALL, KF_TALL_ST, KF_COLOUR, // a colour pass: k_relax_nz, k_relax_tall, k_relax_tall_st, k_relax_colour
  KF_GS, KF_GS_ANY,                      // a hyperplane of the Gauss-Seidel sweep: k_relax_gs_front, k_relax_gs_front_any
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
