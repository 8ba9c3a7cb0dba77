// What the colour-pass kernels of the z-line smoother share (mgx_relax.hip, mgx_relax_tall.hip, mgx_relax_ks.hip): the XCD-aware
// block map, the one definition of the matrix-free column pass and, at the end, the one of the stored-coefficient column pass
// (COL_POS, COL_IMAGES: mgx_device.h).
#pragma once
#include "mgx_device.h"

// XCD-aware block -> (j-chunk bx, plane group ig) map of a 1-D grid of gx * nunit blocks.  Blocks are dealt round-robin over the
// 8 XCDs (b and b+8 share one), each with its own 4 MB L2.  Give every XCD a contiguous range of planes: the pass over plane i and
// the pass over plane i+2 both read p and the slopes of plane i+1.  Where a block holds two waves they take two consecutive planes
// of the colour (nunit = plane pairs), so those two readers also sit on one CU (speed only; any placement gives the same result).
// gx < 0: MGX_NO_XCD=1, the plain map (A/B measurements); gx comes back positive.  A macro for the reason given below.
#define XCD_BLOCK_MAP(nunit, gx, bx, ig)                                             \
  {                                                                                  \
    if (gx < 0) { gx = -gx; ig = blockIdx.x / gx; bx = blockIdx.x - ig * gx; }       \
    else if ((nunit & 7) == 0) {                                                     \
      const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;                       \
      ig = xcd * (nunit >> 3) + local / gx;                                          \
      bx = local - (local / gx) * gx;                                                \
    } else { ig = blockIdx.x / gx; bx = blockIdx.x - ig * gx; }                      \
  }

// ------------------------------------------------------------------------------------------------
// The matrix-free column pass: ONE text for relax_col_mf (mgx_relax.hip, nz <= 64) and relax_col_mf_tall (mgx_relax_tall.hip).
// Every fp64 smoother has a bit-parity duty towards the reference, which rests on the rhs of a row being formed from the same terms
// in the same order everywhere: a fix or a new vertical size is made here, once.  Macros and not a function template over a state
// struct because both callers sit at the edge of the register file (500 of 512 VGPRs, no scratch) and must compile to the
// instructions they had as separate texts; even the block map above, as a function with reference arguments, reordered operands.
//
// Matrix-free cross terms.  Away from the special k=1 diagonals, slots 3,5,6,8 are sums of two slope values:
//   cA3(k,j,i) =  qrt*(ZY(k+1,j,i) + ZY(k,j-1,i))     cA5(k,j,i) = -qrt*(ZY(k-1,j,i) + ZY(k,j-1,i))
//   cA6(k,j,i) =  qrt*(ZX(k+1,j,i) + ZX(k,j,i-1))     cA8(k,j,i) = -qrt*(ZX(k-1,j,i) + ZX(k,j,i-1))
// (mg_define_matrix.f90:357-359,397-399,519-555,584-606) with ZY = ((hlf*(zr(k,j+1,i)-zr(k,j-1,i)))/dy)*dx and
// ZX likewise in i.  A column update needs slots 3,5 of itself AND of its j+1 neighbour (6,8: i+1): four stored
// values per direction, but only three slope values (own column window + one row of each neighbour).  Rebuilding
// the four coefficients in registers with the reference's own expression gives bit-identical values and removes
// 2 of the 19 streams of the colour pass (16 B per updated cell).  Slot 2 and the k=1 diagonal terms stay stored.
// Used when the matrix came from define_matrices (not after mgx_set_field(cA)).
// ZW: the interior rows of slots 4 and 7 (own and of the j+1 / i+1 neighbour: four streams) are rebuilt from the interface depths
// zw of the column and of its four face neighbours with the reference's expressions (mg_define_matrix.f90:532-534,549-551; the 2-D
// factors come precomputed, k_zw_js), and those depths are not streamed either: the sigma coordinate generates them,
// zw(k,j,i) = z0*h*hinv + zeta*(1.+z0*hinv) with z0 = cffw(k) + csw(k)*h (mg_zr_zw.f90:140-145), from three 2-D values per column
// (h, hinv, zeta: loaded once) and two table entries per row that are the same for every lane (scalar loads).  Same expressions,
// bit-identical values (the halo columns too: h and zeta carry the same mirror / exchange rules as zw), FOUR streams less, at seven
// flops per depth and four fp64 divisions per row under the loads.  Rows 1 and nz of slots 4 / 7 have other formulas
// (:361-372,:577-590): they read the stored slots.
// ZG (with ZW): the column's OWN slopes are not streamed either.  zy(k,j,i) = ((hlf*(zr(k,j+1,i)-zr(k,j-1,i)))/dy(j,i))*dx(j,i), zx likewise in
// i (mg_define_matrix.f90:358,398), need zr of the four face neighbours, whose h, hinv, zeta ZW holds already: zr = z0*h*hinv +
// zeta*(1.+z0*hinv), z0 = cffr(k)+csr(k)*h (mg_zr_zw.f90:112-122) -- four depths, two slopes per row, TWO streams less (the slopes of the
// face neighbours, which would need zr of the second ring, stay streamed).  All six divisors of the generated coefficients (dy, dx of the
// column; the four of slots 4 / 7) are per-column constants: DIVC (mgx_device.h).
// Pivots: d(k) = cA(1,k,j,i) is minus the sum of the fourteen couplings of the row, added in the order of mg_define_matrix.f90:632-639
// (bit-identical to the stored value; rows 1 and nz, which have their own formulas :619-627,:642-654, are read: two rows of the stored
// slot 1), then tridiag's recurrence (mg_relax.f90:322-326) -- no bet stream from HBM.
//
// The caller has in scope: NZ, D (look-ahead rows), REAL, SNAP, ST, ZW, ZG, PAIR (compile-time); L, i, c, jm, jp; and two sinks,
//   MF_G_PUT(k, v)  gam(k) = a2(k)*bet(k-1), k = 2 .. NZ
//   MF_X_PUT(k, v, a2k, betk)  the forward value of row k, k = 1 .. NZ, with the row's a2 and pivot (the tall pass keeps one of
//   each to link its register half to its LDS half).
// PAIR: the j-1 / j+1 neighbours by one 16-byte load (LD_PAIR, mgx_device.h) or by two loads, each in the order its caller measured.
// MF_PROLOGUE(XN, GN) declares the column's pointers, factors, load rings, x[XN], g[GN] and lane, and fills the rings;
// MF_ROW(k) is one forward row, to be called for k = 1 .. NZ in order from fully unrolled loops (k a constant after unrolling).
// ------------------------------------------------------------------------------------------------
#define MF_NB_LOAD(q)                                                                                     \
  if ((q) <= NZ) {                                                                                        \
    const long long ro_ = (long long)((q)-1) * RS; const int s_ = (q) % RN;                               \
    if (PAIR) LD_PAIR(p + o + ro_ + jm, r_pjm[s_], r_pjp[s_]) else r_pjm[s_] = p[o + ro_ + jm];           \
    r_pim[s_] = p[om + ro_ + c];                                                                          \
    if (!PAIR) r_pjp[s_] = p[o + ro_ + jp];                                                               \
    r_pip[s_] = p[op + ro_ + c];                                                                          \
    if (PAIR) LD_PAIR(zy + o + ro_ + jm, r_zyjm[s_], r_zyjp[s_])                                          \
    else { r_zyjm[s_] = *(zy + o + ro_ + jm); r_zyjp[s_] = *(zy + o + ro_ + jp); }                        \
    r_zxim[s_] = *(zx + om + ro_ + c); r_zxip[s_] = *(zx + op + ro_ + c);                                 \
    if (!ZW) { r_a4[s_] = *(a4 + o + ro_ + jp); r_a7[s_] = *(a7 + op + ro_ + c); }                        \
  }
#define MF_OW_LOAD(q)                                                                                     \
  if ((q) <= NZ) {                                                                                        \
    const long long ko_ = o + (long long)((q)-1) * RS + c; const int s_ = (q) % RO;                       \
    o_b[s_] = ld_stream<ST>(b + ko_); o_a2[s_] = ld_stream<ST>(a2 + ko_);                                 \
    if (!ZW) { o_a4[s_] = ld_stream<ST>(a4 + ko_); o_a7[s_] = ld_stream<ST>(a7 + ko_); }                  \
    if (!ZG) { o_zy[ZG ? 0 : s_] = ld_stream<ST>(zy + ko_); o_zx[ZG ? 0 : s_] = ld_stream<ST>(zx + ko_); } \
  }
// zr(kk, column q) by its generating formula (mg_zr_zw.f90:112-122); own slopes of row kk from the four face neighbours
#define ZR_GEN(kk, q) ({ const double z0_ = cffr[(kk)-1] + csr[(kk)-1] * hh[q]; z0_ * hh[q] * hv[q] + hz[q] * (1. + z0_ * hv[q]); })
#define OWN_SLOPES(kk, ZY, ZX) { const double zn1_ = ZR_GEN(kk, 1), zn2_ = ZR_GEN(kk, 2), zn3_ = ZR_GEN(kk, 3), zn4_ = ZR_GEN(kk, 4); \
    ZY = DIVC(hlf * (zn2_ - zn1_), gdy, rdy) * gdx; ZX = DIVC(hlf * (zn4_ - zn3_), gdx, rdx) * gdy; }
// ZW_GEN: zw(kk, column q) by its generating formula, shared with the residual + restriction (mgx_device.h)

#define MF_PROLOGUE(XN, GN)                                                                                     \
  const long long RS = L.RS;                                                                              \
  double *__restrict__ p = L.p;                                                                           \
  const double *__restrict__ b = L.b;                                                                     \
  const double *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1], *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4], \
               *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7], *__restrict__ bet = L.bet,                    \
               *__restrict__ zy = L.zy, *__restrict__ zx = L.zx;                                          \
  const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;                         \
  const double qrt = 0.25, hlf = 0.5;                                                                     \
  constexpr int RN = D + 2;  /* rows k .. k+1+D are live at iteration k (row k is still read after the look-ahead load is issued) */ \
  constexpr int RO = D + 2;  /* own rows are needed one row early (zy(k+1), zx(k+1)) */                   \
  double r_pjm[RN], r_pim[RN], r_pjp[RN], r_pip[RN], r_zyjm[RN], r_zyjp[RN], r_zxim[RN], r_zxip[RN], r_a4[RN], r_a7[RN]; \
  double o_b[RO], o_a2[RO], o_a4[RO], o_a7[RO], o_zy[ZG ? 1 : RO], o_zx[ZG ? 1 : RO];                     \
  double x[XN], g[GN];  /* the forward values and gam that stay in registers (the sinks' business) */     \
  const int lane = threadIdx.x;                                                                           \
  /* the diagonal of the first and the last row */                                                        \
  const double dg1 = a1[o + c], dgn = a1[o + (long long)(NZ - 1) * RS + c];                               \
  /* ZW: generated zw of the column and of its j-1, j+1, i-1, i+1 neighbours, rows k and k+1; h, hinv, zeta of the five columns; */ \
  /* stored slots 4 and 7 of the first and the last row; the per-column factors of the interior formula and the refined */ \
  /* reciprocals of its divisors (RCP_REF, mgx_device.h); ZG: dx, dy of the column and their reciprocals */ \
  double zw0[5], zw1[5], hh[5], hv[5], hz[5];                                                             \
  const double *__restrict__ cffw = L.cffw, *__restrict__ csw = L.csw, *__restrict__ cffr = L.cffr, *__restrict__ csr = L.csr; \
  double r4c = 0, r4p = 0, r7c = 0, r7p = 0, gdx = 1, gdy = 1, rdx = 0, rdy = 0;                          \
  double a4_1 = 0, a4j_1 = 0, a7_1 = 0, a7i_1 = 0, a4_n = 0, a4j_n = 0, a7_n = 0, a7i_n = 0;              \
  double m4c = 0, m4p = 0, d4c = 1, d4p = 1, m7c = 0, m7p = 0, d7c = 1, d7p = 1;                          \
  if (ZW) {                                                                                               \
    const long long rn = (long long)(NZ - 1) * RS;                                                        \
    a4_1 = a4[o + c]; a4j_1 = a4[o + jp]; a7_1 = a7[o + c]; a7i_1 = a7[op + c];                           \
    a4_n = a4[o + rn + c]; a4j_n = a4[o + rn + jp]; a7_n = a7[o + rn + c]; a7i_n = a7[op + rn + c];       \
    const long long q2 = (long long)i * RS;                                                               \
    m4c = L.m4[q2 + c]; m4p = L.m4[q2 + jp]; d4c = L.d4[q2 + c]; d4p = L.d4[q2 + jp];                     \
    m7c = L.m7[q2 + c]; m7p = L.m7[q2 + RS + c]; d7c = L.d7[q2 + c]; d7p = L.d7[q2 + RS + c];             \
    const long long cq[5] = {q2 + c, q2 + jm, q2 + jp, q2 - RS + c, q2 + RS + c};  /* the column, j-1, j+1, i-1, i+1 */ \
    _Pragma("unroll") for (int q = 0; q < 5; q++) { hh[q] = L.h2[cq[q]]; hv[q] = L.hi2[cq[q]]; hz[q] = L.ze2[cq[q]]; } \
    r4c = RCP_REF(d4c); r4p = RCP_REF(d4p); r7c = RCP_REF(d7c); r7p = RCP_REF(d7p);                       \
    if (ZG) { gdx = L.dx2[q2 + c]; gdy = L.dy2[q2 + c]; rdx = RCP_REF(gdx); rdy = RCP_REF(gdy); }         \
  }                                                                                                       \
  /* k = 1 horizontal-diagonal terms (mg_relax.f90:271-276); red-black reads them from the snapshot taken before the pass */ \
  double d1 = 0, d2 = 0, d3 = 0, d4 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;                                  \
  if (REAL) K1_DIAG(SNAP, d1, d2, d3, d4, e1, e2, e3, e4)                                                 \
  _Pragma("unroll") for (int q = 1; q <= 1 + D; q++) { MF_NB_LOAD(q) }                                    \
  _Pragma("unroll") for (int q = 1; q <= 1 + D; q++) { MF_OW_LOAD(q) }                                    \
  /* three-row windows (k-1, k, k+1) of the neighbour columns' p and of the own slopes */                 \
  double pjm_m = 0, pjm_0 = r_pjm[1 % RN], pjm_p = 0, pim_m = 0, pim_0 = r_pim[1 % RN], pim_p = 0;        \
  double pjp_m = 0, pjp_0 = r_pjp[1 % RN], pjp_p = 0, pip_m = 0, pip_0 = r_pip[1 % RN], pip_p = 0;        \
  double zy_m = 0, zy_0 = 0, zy_p = 0, zx_m = 0, zx_0 = 0, zx_p = 0;                                      \
  if (ZG) OWN_SLOPES(1, zy_0, zx_0)                                                                       \
  else { zy_0 = o_zy[ZG ? 0 : 1 % RO]; zx_0 = o_zx[ZG ? 0 : 1 % RO]; }                                    \
  double xv = 0.0, betp = 0.0;

#define MF_ROW(k)                                                                                         \
  {                                                                                                       \
    MF_NB_LOAD(k + 1 + D)                                                                                 \
    MF_OW_LOAD(k + 1 + D)                                                                                 \
    if (k < NZ) {                                                                                         \
      const int s1 = (k + 1) % RN, t1 = (k + 1) % RO;                                                     \
      pjm_p = r_pjm[s1]; pim_p = r_pim[s1]; pjp_p = r_pjp[s1]; pip_p = r_pip[s1];                         \
      if (ZG) OWN_SLOPES(k + 1, zy_p, zx_p)                                                               \
      else { zy_p = o_zy[ZG ? 0 : t1]; zx_p = o_zx[ZG ? 0 : t1]; }                                        \
    }                                                                                                     \
    const int s = k % RO, n = k % RN;                                                                     \
    const double zyjm = r_zyjm[n], zyjp = r_zyjp[n], zxim = r_zxim[n], zxip = r_zxip[n];                  \
    /* the eight cross coefficients of this row, rebuilt from the slopes: own slots 3,5,6,8 and the mirrored ones stored at */ \
    /* the j+1 / i+1 neighbours */                                                                        \
    MF_CROSS_COEF(zy_m, zy_p, zyjm, zyjp, zx_m, zx_p, zxim, zxip)                                         \
    double a4o, a4jp, a7o, a7ip;  /* slots 4 and 7 of the cell and of its j+1 / i+1 neighbour */          \
    if (!ZW) { a4o = o_a4[s]; a4jp = r_a4[n]; a7o = o_a7[s]; a7ip = r_a7[n]; }                            \
    else if (k == 1) { a4o = a4_1; a4jp = a4j_1; a7o = a7_1; a7ip = a7i_1; }                              \
    else if (k == NZ) { a4o = a4_n; a4jp = a4j_n; a7o = a7_n; a7ip = a7i_n; }                             \
    else {                                                                                                \
      if (k == 2) { _Pragma("unroll") for (int q = 0; q < 5; q++) zw0[q] = ZW_GEN(2, q); }                \
      _Pragma("unroll") for (int q = 0; q < 5; q++) zw1[q] = ZW_GEN(k + 1, q);                            \
      const double wo0 = zw0[0], wop1 = zw1[0];                                                           \
      a4o = SLOT47_GEN(wop1, wo0, zw1[1], zw0[1], m4c, d4c, r4c);                                         \
      a4jp = SLOT47_GEN(zw1[2], zw0[2], wop1, wo0, m4p, d4p, r4p);                                        \
      a7o = SLOT47_GEN(wop1, wo0, zw1[3], zw0[3], m7c, d7c, r7c);                                         \
      a7ip = SLOT47_GEN(zw1[4], zw0[4], wop1, wo0, m7p, d7p, r7p);                                        \
      _Pragma("unroll") for (int q = 0; q < 5; q++) zw0[q] = zw1[q];                                      \
    }                                                                                                     \
    double dk, betk;  /* the pivots (header comment) */                                                   \
    if (k == 1) dk = dg1;                                                                                 \
    else if (k == NZ) dk = dgn;                                                                           \
    else dk = -o_a2[s] - o_a2[(k + 1) % RO] - a4o - a4jp - a7o - a7ip - c6 - c6m - c8 - c8m - c3 - c3m - c5 - c5m; \
    if (k == 1) betk = 1.0 / dk;                                                                          \
    else { const double gk = o_a2[s] * betp; MF_G_PUT(k, gk) betk = 1.0 / (dk - o_a2[s] * gk); }          \
    betp = betk;                                                                                          \
    double rhs;                                                                                           \
    if (k == 1) {                                                                                         \
      rhs = ROW_RHS_FIRST(o_b[s], MF_TERMS);                                                              \
      if (REAL) rhs = rhs - e1 * d1 - e2 * d2 - e3 * d3 - e4 * d4;                                        \
      xv = rhs * betk;                                                                                    \
    } else if (k < NZ) {                                                                                  \
      rhs = ROW_RHS_MID(o_b[s], MF_TERMS);                                                                \
      xv = (rhs - o_a2[s] * xv) * betk;                                                                   \
    } else {                                                                                              \
      rhs = ROW_RHS_LAST(o_b[s], MF_TERMS);                                                               \
      xv = (rhs - o_a2[s] * xv) * betk;                                                                   \
    }                                                                                                     \
    MF_X_PUT(k, xv, o_a2[s], betk)                                                                        \
    pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p;                                           \
    pjp_m = pjp_0; pjp_0 = pjp_p; pip_m = pip_0; pip_0 = pip_p;                                           \
    zy_m = zy_0; zy_0 = zy_p; zx_m = zx_0; zx_0 = zx_p;                                                   \
  }

// ------------------------------------------------------------------------------------------------
// The stored-coefficient column pass: ONE text for relax_col_nz (mgx_relax.hip, nz <= 64) and relax_col_st_tall
// (mgx_relax_tall.hip): slots 2-8 and the pivots bet as define_matrices or mgx_set_field(cA) left them, nothing regenerated (masked
// domains, user matrices, MGX_NO_MF).  The rhs of a row after mg_relax.f90:262-301: ROW_RHS_* (mgx_device.h) on SC_TERMS.  Macros for the
// reason given above; the instances of relax_col_nz compile to the instructions they had when this text stood in their function.
//
// The caller has in scope: NZ, D (look-ahead rows), REAL, SNAP, ST (compile-time); L, i, c, jm, jp; and two sinks,
//   SC_G_PUT(k, v)  gam(k) = a2(k)*bet(k-1), k = 2 .. NZ
//   SC_X_PUT(k, v)  the forward value of row k, k = 1 .. NZ.
// SC_PROLOGUE(XN, GN) declares the column's pointers, load rings, x[XN], g[GN] and fills the rings; SC_ROW(k) is one forward row, to
// be called for k = 1 .. NZ in order from fully unrolled loops.
// ------------------------------------------------------------------------------------------------
#define SC_NB_LOAD(q)                                                            \
  if ((q) <= NZ) {                                                               \
    const long long ro_ = (long long)((q)-1) * RS; const int s_ = (q) % RN;      \
    r_pjm[s_] = p[o + ro_ + jm]; r_pim[s_] = p[om + ro_ + c];                    \
    r_pjp[s_] = p[o + ro_ + jp]; r_pip[s_] = p[op + ro_ + c];                    \
    r_a3[s_] = a3[o + ro_ + jp]; r_a4[s_] = a4[o + ro_ + jp]; r_a5[s_] = a5[o + ro_ + jp]; \
    r_a6[s_] = a6[op + ro_ + c]; r_a7[s_] = a7[op + ro_ + c]; r_a8[s_] = a8[op + ro_ + c]; \
  }
#define SC_OW_LOAD(q)                                                            \
  if ((q) <= NZ) {                                                               \
    const long long ko_ = o + (long long)((q)-1) * RS + c; const int s_ = (q) % RO; \
    o_b[s_] = ld_stream<ST>(b + ko_); o_a2[s_] = ld_stream<ST>(a2 + ko_); o_a3[s_] = ld_stream<ST>(a3 + ko_); o_a4[s_] = ld_stream<ST>(a4 + ko_); o_a5[s_] = ld_stream<ST>(a5 + ko_); \
    o_a6[s_] = ld_stream<ST>(a6 + ko_); o_a7[s_] = ld_stream<ST>(a7 + ko_); o_a8[s_] = ld_stream<ST>(a8 + ko_); o_bet[s_] = ld_stream<ST>(bet + ko_); \
  }
// products of a raw neighbour row (computed when the row is first needed)
#define SC_NB_USE(q, PJM, PIM, M3, M4, M5, N6, N7, N8)                           \
  { const int s_ = (q) % RN; PJM = r_pjm[s_]; PIM = r_pim[s_];                   \
    M3 = r_a3[s_] * r_pjp[s_]; M4 = r_a4[s_] * r_pjp[s_]; M5 = r_a5[s_] * r_pjp[s_]; \
    N6 = r_a6[s_] * r_pip[s_]; N7 = r_a7[s_] * r_pip[s_]; N8 = r_a8[s_] * r_pip[s_]; }

#define SC_PROLOGUE(XN, GN)                                                                               \
  const long long RS = L.RS;                                                                              \
  double *__restrict__ p = L.p;                                                                           \
  const double *__restrict__ b = L.b;                                                                     \
  const double *__restrict__ a2 = L.cA[1], *__restrict__ a3 = L.cA[2], *__restrict__ a4 = L.cA[3],        \
               *__restrict__ a5 = L.cA[4], *__restrict__ a6 = L.cA[5], *__restrict__ a7 = L.cA[6],        \
               *__restrict__ a8 = L.cA[7], *__restrict__ bet = L.bet;                                     \
  const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;                         \
  constexpr int RN = D + 1;  /* raw neighbour rows in flight */                                           \
  constexpr int RO = D + 1;  /* raw own rows in flight */                                                 \
  double r_pjm[RN], r_pim[RN], r_pjp[RN], r_pip[RN], r_a3[RN], r_a4[RN], r_a5[RN], r_a6[RN], r_a7[RN], r_a8[RN]; \
  double o_b[RO], o_a2[RO], o_a3[RO], o_a4[RO], o_a5[RO], o_a6[RO], o_a7[RO], o_a8[RO], o_bet[RO];        \
  double x[XN], g[GN];  /* the forward values and gam that stay in registers (the sinks' business) */     \
  /* k = 1 horizontal-diagonal terms (issued first: independent of everything else); red-black reads them from the snapshot */ \
  double d1 = 0, d2 = 0, d3 = 0, d4 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;                                  \
  if (REAL) K1_DIAG(SNAP, d1, d2, d3, d4, e1, e2, e3, e4)                                                 \
  /* neighbour rows 1..1+D and own rows 1..D */                                                           \
  _Pragma("unroll") for (int q = 1; q <= 1 + D; q++) { SC_NB_LOAD(q) }                                    \
  _Pragma("unroll") for (int q = 1; q <= D; q++) { SC_OW_LOAD(q) }                                        \
  double pjm_m = 0, pjm_0, pjm_p, pim_m = 0, pim_0, pim_p;                                                \
  double m3_m = 0, m3_0, m4_0, m5_p, n6_m = 0, n6_0, n7_0, n8_p, m3_p, m4_p, n6_p, n7_p, dum5, dum8;      \
  SC_NB_USE(1, pjm_0, pim_0, m3_0, m4_0, dum5, n6_0, n7_0, dum8)                                          \
  (void)dum5; (void)dum8;                                                                                 \
  double xv = 0.0, betp = 0.0;

// row k of SC_ROW as the arguments of ROW_RHS_* (mgx_device.h): own slots from the ring, the neighbours' products of SC_NB_USE
#define SC_TERMS o_b[s], o_a3[s] * pjm_p, m3_m, o_a4[s] * pjm_0, m4_0, o_a5[s] * pjm_m, m5_p, o_a6[s] * pim_p, n6_m, o_a7[s] * pim_0, n7_0, o_a8[s] * pim_m, n8_p
#define SC_ROW(k)                                                                                         \
  {                                                                                                       \
    /* keep the pipeline full */                                                                          \
    SC_NB_LOAD(k + 1 + D)                                                                                 \
    SC_OW_LOAD(k + D)                                                                                     \
    if (k < NZ) { SC_NB_USE(k + 1, pjm_p, pim_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p) }                    \
    const int s = k % RO;                                                                                 \
    double rhs;                                                                                           \
    /* gam(k) = dd(k-1)*bet(k-1) (mg_relax.f90:325), from values already in registers: no gam stream from HBM */ \
    if (k > 1) SC_G_PUT(k, o_a2[s] * betp)                                                                \
    betp = o_bet[s];                                                                                      \
    if (k == 1) {                                                                                         \
      rhs = ROW_RHS_FIRST(SC_TERMS);                                                                      \
      if (REAL) rhs = rhs - e1 * d1 - e2 * d2 - e3 * d3 - e4 * d4;                                        \
      xv = rhs * o_bet[s];                                                                                \
    } else if (k < NZ) {                                                                                  \
      rhs = ROW_RHS_MID(SC_TERMS);                                                                        \
      xv = (rhs - o_a2[s] * xv) * o_bet[s];                                                               \
    } else {                                                                                              \
      rhs = ROW_RHS_LAST(SC_TERMS);                                                                       \
      xv = (rhs - o_a2[s] * xv) * o_bet[s];                                                               \
    }                                                                                                     \
    SC_X_PUT(k, xv)                                                                                       \
    /* rotate the three-row window */                                                                     \
    pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p;                                           \
    m3_m = m3_0; m3_0 = m3_p; m4_0 = m4_p; n6_m = n6_0; n6_0 = n6_p; n7_0 = n7_p;                         \
  }
