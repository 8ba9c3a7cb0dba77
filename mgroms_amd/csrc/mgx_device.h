// Device helpers shared by the HIP translation units of libmgx.so.
#pragma once
#include "mgx_internal.h"
#include "mgx_choice.h"

#define WAVE 64
// Cache policy.  A level that cannot live in the 256 MB Infinity Cache (level 1 of the 512x512x64 problem: 1.2 GB)
// is streamed: what a pass reads exactly once, and what it writes, carries the non-temporal hint so that it does not
// evict the lines that ARE re-read inside the pass (the other j-half of a row, the i+-1 planes shared by two waves).
// Measured on the level-1 four-colour sweep: 0.35 -> 0.29 ms (loads alone 0.32, store alone 0.31).  Levels that fit
// the cache keep the default policy (the hint costs 20 % there), and so do loads whose lines another block of the same
// launch re-reads (the residual's two j-parities).  Chosen at compile time (ST) or per launch (level_streams).
#define NT_LOAD(ptr) __builtin_nontemporal_load(ptr)
#define NT2_STORE(v, ptr) __builtin_nontemporal_store(v, ptr)
template <bool NT> __device__ __forceinline__ double ld_stream(const double *p) { return NT ? NT_LOAD(p) : *p; }
__device__ __forceinline__ void st_rt(double *p, double v, int nt) { if (nt) __builtin_nontemporal_store(v, p); else *p = v; }
__device__ __forceinline__ double ld_rt(const double *p, int nt) { return nt ? __builtin_nontemporal_load(p) : *p; }
static inline int level_streams(const LevView *L) { return ch_beyond_cache(lev_shape(L)); }   // one threshold: mgx_choice.h

// positions c, jm, jp of columns j, j-1, j+1 inside a row of the JS layout (mgx_internal.h): j = 2 jh + 1 (jodd) or 2 jh + 2
#define COL_POS(L, jh, jodd, c, jm, jp)                                 \
  {                                                                     \
    if (jodd) { c = L.HO + jh; jm = L.EO + jh; jp = jm + 1; }           \
    else      { c = L.EO + jh + 1; jm = L.HO + jh; jp = jm + 1; }       \
  }

// The physical-boundary images of column (j, i): homogeneous Neumann mirror incl. the corner where two physical sides meet
// (mg_mpi_exchange.f90:509-537,552-597).  The lane that owns a column stores them with it, which removes the halo kernel after a
// pass.  COL_IMAGES declares which images the column has and where they sit; COL_STORE and COL_SNAPSHOT use them.  Macros, like
// the column pass of mgx_relax_common.h and for its reason: as forceinline functions over a struct they moved the register
// allocation of their callers (profiles/relax_mf_single_source_isa.json, "function_form_rejected", has the figures).
#define COL_IMAGES(L, i, j, ph)                                                                                              \
  const bool mS = ph.S && j == 1, mN = ph.N && j == L.ny, mW = ph.W && i == 1, mE = ph.E && i == L.nx;                       \
  const int cS = L.EO, cN = jpos(L, L.ny + 1);                                                                               \
  const long long oW = 0, oE = (long long)(L.nx + 1) * L.plane;
// row ro of the column in p (plane offset o) with its images; ST: the column's own cell with the non-temporal hint
#define COL_STORE(ST, p, o, ro, c, v)                                                                                        \
  {                                                                                                                          \
    if (ST) NT2_STORE(v, p + o + ro + c); else p[o + ro + c] = v;                                                            \
    if (mS) p[o + ro + cS] = v;                                                                                              \
    if (mN) p[o + ro + cN] = v;                                                                                              \
    if (mW) { p[oW + ro + c] = v; if (mS) p[oW + ro + cS] = v; if (mN) p[oW + ro + cN] = v; }                                \
    if (mE) { p[oE + ro + c] = v; if (mS) p[oE + ro + cS] = v; if (mN) p[oE + ro + cN] = v; }                                \
  }
// next sweep's k=1 snapshot entry of this column (and its physical mirrors): no snapshot launch per pass.
// A mirrored halo cell is read (as a k=1 diagonal) only by columns of the OTHER colour, i.e. by the next pass of this
// same sweep, which must see it updated: mirrors go to the buffer being read as well (no column of this pass reads them,
// except a corner column its own corner, after which it is the one to overwrite it).
#define SNAP_MIRROR(idx) { w1[idx] = v1; r1[idx] = v1; }
#define COL_SNAPSHOT(L, RS, i, c, v)                                                                                          \
  {                                                                                                                          \
    double *w1 = L.p1w, *r1 = L.p1;                                                                                          \
    const long long so = (long long)i * RS, sW = 0, sE = (long long)(L.nx + 1) * RS;                                  \
    const double v1 = v;                                                                                                     \
    w1[so + c] = v1;                                                                                                         \
    if (mS) SNAP_MIRROR(so + cS)                                                                                             \
    if (mN) SNAP_MIRROR(so + cN)                                                                                             \
    if (mW) { SNAP_MIRROR(sW + c) if (mS) SNAP_MIRROR(sW + cS) if (mN) SNAP_MIRROR(sW + cN) }                                \
    if (mE) { SNAP_MIRROR(sE + c) if (mS) SNAP_MIRROR(sE + cS) if (mN) SNAP_MIRROR(sE + cN) }                                \
  }

// the images alone of a value that a kernel outside the smoother has just stored at a[i * plane + ro + c]
__device__ __forceinline__ void mirror_store(const LevView &L, double *__restrict__ a, const long long ro, const int j, const int i,
                                             const int c, const double v, const Sides ph) {
  const bool mS = ph.S && j == 1, mN = ph.N && j == L.ny, mW = ph.W && i == 1, mE = ph.E && i == L.nx;
  if (!(mS | mN | mW | mE)) return;
  const int cS = L.EO, cN = jpos(L, L.ny + 1);
  const long long o = (long long)i * L.plane + ro, oW = ro, oE = (long long)(L.nx + 1) * L.plane + ro;
  if (mS) a[o + cS] = v;
  if (mN) a[o + cN] = v;
  if (mW) { a[oW + c] = v; if (mS) a[oW + cS] = v; if (mN) a[oW + cN] = v; }
  if (mE) { a[oE + c] = v; if (mS) a[oE + cS] = v; if (mN) a[oE + cN] = v; }
}

// A rejected launch (more LDS or registers than this ROCm / device grants) must not pass for a completed colour pass: wrappers that
// have a generic fallback end in `return mgx_launched();` -- 0 = the launch was refused, nothing ran, the caller falls back; whatever
// has no fallback is caught by the sticky-error check of the next synchronising call (sync_stream in mgx_comm.cpp).
// hipGetLastError() is sticky per thread for ANY earlier HIP call (an ignored attribute call, the caller's own runtime use): a wrapper that
// ends in mgx_launched() starts with mgx_before_launch(), which moves whatever is pending into mgx_pending_error (reported by the next
// synchronising call) so that mgx_launched() sees the status of THIS launch only.
extern thread_local hipError_t mgx_pending_error;  // mgx_comm.cpp
static inline void mgx_before_launch() { const hipError_t e = hipGetLastError(); if (e != hipSuccess && mgx_pending_error == hipSuccess) mgx_pending_error = e; }
static inline int mgx_launched() { return hipGetLastError() == hipSuccess ? 1 : 0; }

// The sum of r^2 of a residual norm, carried as an unevaluated pair hi + lo (Knuth's two-sum: the rounding error of every addition to
// hi is exact and goes to lo; compiled with -ffp-contract=off and without reassociation).  The pair holds the sum to ~2^-100, so its
// rounded value does not depend on how a kernel groups the cells: k_residual, k_residual_mf and the fused residual + restriction
// (mgx_resrest.hip), whose lanes, waves and workgroups cut the level differently, leave the same norm.  Each term is one cell's rounded
// r * r.  Partials: hi at partial[idx], lo at partial[n + idx], n = the launch's workgroups; k_reduce_partials_dd closes them.
__device__ __forceinline__ void dd_add(double &hi, double &lo, const double t) {
  const double s = hi + t, bb = s - hi;
  lo = lo + ((hi - (s - bb)) + (t - bb));
  hi = s;
}
__device__ __forceinline__ void dd_merge(double &hi, double &lo, const double ohi, const double olo) {
  const double s = hi + ohi, bb = s - hi;
  lo = (lo + olo) + ((hi - (s - bb)) + (ohi - bb));
  hi = s;
}

static inline dim3 col_grid(int ncol_half, int nplanes, int z = 1) { return dim3((ncol_half + WAVE - 1) / WAVE, (nplanes + 3) / 4, z); }

// ---- helpers shared by the smoother translation units ---------------------------------------------------------------
// A quotient whose divisor is a per-column constant: the divisor's reciprocal is refined once with the two Newton steps of the hardware
// division sequence (v_rcp_f64, fma, fma, fma, fma) and each quotient then takes the sequence's last three operations (mul, fma, fma) --
// the same operations on the same values as `/` while no operand needs v_div_scale's rescaling (depths, metric factors: normal range),
// hence the same bits, at 3 instructions instead of ~11 per division.
#define RCP_REF(b) ({ const double b_ = (b); double r_ = __builtin_amdgcn_rcp(b_); double e_ = __builtin_fma(-b_, r_, 1.0); r_ = __builtin_fma(r_, e_, r_); \
                      e_ = __builtin_fma(-b_, r_, 1.0); __builtin_fma(r_, e_, r_); })
#define DIVC(a, b, rb) ({ const double a_ = (a); const double q_ = a_ * (rb); const double e_ = __builtin_fma(-(b), q_, a_); __builtin_fma(e_, (rb), q_); })
// zw(kk, column q) by its generating formula (mg_zr_zw.f90:140-145): ONE text for the colour passes (MF_ROW, mgx_relax_common.h) and the
// residual + restriction (mgx_resrest.hip), whose generated slots 4 / 7 must be the same bits.  In scope: the sigma tables cffw, csw and
// h, hinv, zeta of the caller's columns as hh[], hv[], hz[].
#define ZW_GEN(kk, q) ({ const double z0_ = cffw[(kk)-1] + csw[(kk)-1] * hh[q]; z0_ * hh[q] * hv[q] + hz[q] * (1. + z0_ * hv[q]); })
// An interior row of a generated slot 4 or 7 (mg_define_matrix.f90:532-534,549-551) from the depths ZW_GEN made: hi_ / lo_ = zw(k+1) / zw(k)
// of the two columns the coupling joins, in the reference's order; m, d = the coupling's 2-D factors, r = RCP_REF(d).  qrt in scope.
#define SLOT47_GEN(hi_a, lo_a, hi_b, lo_b, m, d, r) DIVC(qrt * ((hi_a) - (lo_a) + (hi_b) - (lo_b)) * (m), (d), (r))

// ---- the row: what the bit parity of every fp64 kernel hangs on ------------------------------------------------------------
// The right-hand side of row k of column (j, i) is B minus its twelve off-column products, subtracted one by one in the reference's
// order (mg_relax.f90:262-301 for the smoother; :464-509 for the residual, where B = b minus the own-column terms, which stand in
// front of the same twelve).  ONE text for every fp64 kernel; DESIGN.md 2.1 lists who expands it.  T<n> is slot n of the cell
// itself times the neighbour it couples to, T<n>M the mirrored coupling that the symmetric storage keeps at the j+1 / i+1 neighbour:
//   T3 = cA(3,k,j,i) p(k+1,j-1,i)   T3M = cA(3,k-1,j+1,i) p(k-1,j+1,i)     T6 = cA(6,k,j,i) p(k+1,j,i-1)   T6M = cA(6,k-1,j,i+1) p(k-1,j,i+1)
//   T4 = cA(4,k,j,i) p(k,j-1,i)     T4M = cA(4,k,j+1,i) p(k,j+1,i)         T7 = cA(7,k,j,i) p(k,j,i-1)     T7M = cA(7,k,j,i+1) p(k,j,i+1)
//   T5 = cA(5,k,j,i) p(k-1,j-1,i)   T5M = cA(5,k+1,j+1,i) p(k+1,j+1,i)     T8 = cA(8,k,j,i) p(k-1,j,i-1)   T8M = cA(8,k+1,j,i+1) p(k+1,j,i+1)
// Row 1 has no k-1 terms and row nz no k+1 terms; the k = 1 horizontal diagonals of cmatrix = 'real' (:271-276, :475-479) stay a
// statement of their own behind the first row.  A site writes its thirteen arguments once, as a term list (#define X_TERMS B, T3, ...),
// and keeps its own `if (k == 1) ... else if (k < nz) ... else` ladder of statements: as one ?: expression the kernels whose k is a
// run-time value compiled differently.  The forwarders are variadic so that a term list is expanded before the arguments are counted.
#define ROW_RHS_FIRST_(B, T3, T3M, T4, T4M, T5, T5M, T6, T6M, T7, T7M, T8, T8M) ((B) - (T3) - (T4) - (T4M) - (T5M) - (T6) - (T7) - (T7M) - (T8M))
#define ROW_RHS_MID_(B, T3, T3M, T4, T4M, T5, T5M, T6, T6M, T7, T7M, T8, T8M) \
  ((B) - (T3) - (T3M) - (T4) - (T4M) - (T5) - (T5M) - (T6) - (T6M) - (T7) - (T7M) - (T8) - (T8M))
#define ROW_RHS_LAST_(B, T3, T3M, T4, T4M, T5, T5M, T6, T6M, T7, T7M, T8, T8M) ((B) - (T3M) - (T4) - (T4M) - (T5) - (T6M) - (T7) - (T7M) - (T8))
#define ROW_RHS_FIRST(...) ROW_RHS_FIRST_(__VA_ARGS__)
#define ROW_RHS_MID(...) ROW_RHS_MID_(__VA_ARGS__)
#define ROW_RHS_LAST(...) ROW_RHS_LAST_(__VA_ARGS__)
// The twelve products by the names that the column texts share; both lists bind locals of the texts that expand them.
// ST_TERMS, stored slots: a3 .. a8 (the cell's own slots, read at ko), the windows pjm_*, pim_* and the neighbours' products m3_m .. n8_p
// as LOAD_ROW left them, in relax_col_any (mgx_relax.hip) and OP_COLUMN (mgx_operator.h).
// MF_TERMS, matrix-free: c3 .. c8m of MF_CROSS_COEF, slots 4 / 7 of the cell and of its j+1 / i+1 neighbour (a4o, a4jp, a7o, a7ip) and the
// windows pjm_*, pjp_*, pim_*, pip_*, in MF_ROW (mgx_relax_common.h), OP_COLUMN_MF (mgx_operator.h) and RR_* (mgx_resrest.hip).
#define ST_TERMS(ko) a3[ko] * pjm_p, m3_m, a4[ko] * pjm_0, m4_0, a5[ko] * pjm_m, m5_p, a6[ko] * pim_p, n6_m, a7[ko] * pim_0, n7_0, a8[ko] * pim_m, n8_p
#define MF_TERMS c3 * pjm_p, c3m * pjp_m, a4o * pjm_0, a4jp * pjp_0, c5 * pjm_m, c5m * pjp_p, c6 * pim_p, c6m * pip_m, a7o * pim_0, a7ip * pip_0, c8 * pim_m, c8m * pip_p
// The eight matrix-free cross coefficients of a row (mgx_relax_common.h explains them): own slots 3, 5, 6, 8 and the mirrored ones, from
// the own slopes of rows k-1 / k+1 (zy_m, zy_p, zx_m, zx_p) and the j-1 / j+1 / i-1 / i+1 neighbours' slopes of row k.  qrt in scope.
#define MF_CROSS_COEF(zy_m, zy_p, zyjm, zyjp, zx_m, zx_p, zxim, zxip)                                                              \
  const double c3 = qrt * (zy_p + zyjm), c3m = qrt * (zyjp + zy_m), c5 = -qrt * (zy_m + zyjm), c5m = -qrt * (zyjp + zy_p);          \
  const double c6 = qrt * (zx_p + zxim), c6m = qrt * (zxip + zx_m), c8 = -qrt * (zx_m + zxim), c8m = -qrt * (zxip + zx_p);
// The k = 1 same-colour diagonals (mg_relax.f90:271-276): their four coefficients, and with them the four values of p, which a red-black
// pass reads from the snapshot taken before it (SNAP): K1_SNAP_ADDR declares where they are, q1[sm / sp + jm / jp].
// In scope: L, p, a5, a8, i, RS, o, om, op, c, jm, jp.
#define K1_COEF(e1, e2, e3, e4) { e1 = a5[o + c]; e2 = a5[op + jm]; e3 = a8[o + c]; e4 = a8[op + jp]; }
#define K1_SNAP_ADDR(SNAP)                                                                                                       \
  const double *__restrict__ q1 = SNAP ? L.p1 : p;                                                                               \
  const long long s = SNAP ? (long long)i * RS : o, sm = SNAP ? s - RS : om, sp = SNAP ? s + RS : op;
#define K1_DIAG(SNAP, d1, d2, d3, d4, e1, e2, e3, e4)                                                                             \
  {                                                                                                                              \
    K1_SNAP_ADDR(SNAP)                                                                                                           \
    d1 = q1[sm + jp]; d2 = q1[sp + jm]; d3 = q1[sm + jm]; d4 = q1[sp + jp];                                                      \
    K1_COEF(e1, e2, e3, e4)                                                                                                      \
  }
// The j-1 and j+1 neighbours of a column sit side by side in the other half-row (jp = jm + 1): ONE 16-byte load per lane fetches
// both, instead of two 8-byte loads whose wave-wide footprints overlap by 63/64 (half the wave-level requests for these streams;
// 8-byte alignment only: gfx950 global loads do not need natural alignment)
#define LD_PAIR(ptr, A, B) { double2 t2_; __builtin_memcpy(&t2_, (ptr), 16); A = t2_.x; B = t2_.y; }

// the value of the neighbouring lane across the whole wave (DPP wave shifts of gfx9: one v_mov_b32_dpp per half, no LDS)
__device__ __forceinline__ double wave_shr1(double x) {  // lane n takes lane n-1's value, lane 0 takes 0
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_shl1(double x) {  // lane n takes lane n+1's value, lane 63 takes 0
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

