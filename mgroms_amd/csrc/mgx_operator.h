// The level-1 operator, ONE text per form: the 15-point product of compute_residual (mg_relax.f90:421-515) from the stored slots and with
// matrix-free cross terms, for the residual kernels (mgx_residual.hip: k_residual, k_residual_mf) and pass 1 of the Krylov loop
// (mgx_krylov.hip: k_kr_apply, k_kr_apply_mf), which is the same operator on b = 0 with the sign turned.  Both have a bit-parity duty that
// rests on a row being formed from the same terms in the same order: the own-column terms stand here, once, and the twelve off-column
// terms behind them are ROW_RHS_* of mgx_device.h, the text that the smoothers expand as well.  With them, the block map of
// these launches and the block reduction of the kernels that leave one partial sum per workgroup.  The column texts and the reduction are
// macros with caller-supplied hooks, for the reason given in mgx_relax_common.h: the callers must compile to the instructions they had
// as separate texts (profiles/operator_single_source_isa.json).
#pragma once
#include "mgx_device.h"

// The launch of an operator kernel (choose_operator, mgx_choice_transfer.h): f(MF, REAL) names the instance of the caller's pair of kernels
#define OP_BLOCK dim3(WAVE, 4)
template <class F> static inline void op_launch(const OpChoice &c, int real, F &&f) {
  with_bool(c.mf, [&](auto MF) { with_bool(real != 0, [&](auto REAL) { f(MF, REAL); }); });
}

// XCD-aware block -> (j-chunk bx, plane group by, j parity bz) map of a 1-D grid of gx * gy * 2 blocks: each XCD owns a contiguous range
// of plane groups, as with XCD_BLOCK_MAP (mgx_relax_common.h, which explains why).  It differs from that map in its unit: the two
// j-parities of a plane group (bz = 0: odd j, 1: even j) run back to back on the same XCD, since they read the same rows; and it has no
// plain-map switch (spelt through XCD_BLOCK_MAP, that switch's branch stays in the kernels: 17 instructions more each).  A function and
// not a macro because this is the form that leaves all four callers as they were: written out in k_kr_apply, the same text allocates
// two more VGPRs there (the profile has the figures), while the residual kernels compile to the same instructions either way.
__device__ __forceinline__ void op_block_map(int gx, int gy, int &bx, int &by, int &bz) {
  const int per = gx * 2;
  int grp, local;
  if ((gy & 7) == 0) { const int xcd = blockIdx.x & 7; local = blockIdx.x >> 3; grp = xcd * (gy >> 3) + local / per; local -= (local / per) * per; }
  else { grp = blockIdx.x / per; local = blockIdx.x - grp * per; }
  by = grp; bz = local / gx; bx = local - bz * gx;
}

// Sum of one per-lane acc over the workgroup -> partial[idx]: wave shuffle, then LDS across the waves of the block in index order
// (deterministic).  Every lane of the block must arrive.
#define OP_BLOCK_SUM(acc, partial, idx)                                                                                                      \
  {                                                                                                                                          \
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);                                                                 \
    __shared__ double red[16];                                                                                                               \
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, w = tid >> 6;                                                                    \
    if ((tid & 63) == 0) red[w] = acc;                                                                                                       \
    __syncthreads();                                                                                                                         \
    if (tid == 0) {                                                                                                                          \
      double s = 0.0;                                                                                                                        \
      const int nw = (blockDim.x * blockDim.y + 63) >> 6;                                                                                    \
      for (int q = 0; q < nw; q++) s += red[q];                                                                                              \
      partial[idx] = s;                                                                                                                      \
    }                                                                                                                                        \
  }

// The same for a sum carried as a pair (dd_add, mgx_device.h): hi -> partial[idx], lo -> partial[n + idx], n = the launch's workgroups
#define OP_BLOCK_SUM_DD(acc, acl, partial, idx, n)                                                                                           \
  {                                                                                                                                          \
    for (int off = 32; off > 0; off >>= 1) { const double oh_ = __shfl_down(acc, off, 64), ol_ = __shfl_down(acl, off, 64); dd_merge(acc, acl, oh_, ol_); } \
    __shared__ double red[32];                                                                                                               \
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, w = tid >> 6;                                                                    \
    if ((tid & 63) == 0) { red[w] = acc; red[16 + w] = acl; }                                                                                \
    __syncthreads();                                                                                                                         \
    if (tid == 0) {                                                                                                                          \
      double s = 0.0, sl = 0.0;                                                                                                              \
      const int nw = (blockDim.x * blockDim.y + 63) >> 6;                                                                                    \
      for (int q = 0; q < nw; q++) dd_merge(s, sl, red[q], red[16 + q]);                                                                     \
      partial[idx] = s; partial[(n) + (idx)] = sl;                                                                                           \
    }                                                                                                                                        \
  }

// ------------------------------------------------------------------------------------------------
// The column from the stored slots: rr(k) = rhs(k) - (A p)(k), k = 1 .. nz, one lane = one (j, i) column.
// The caller has in scope: REAL (compile-time); L, i, jh, jodd, c, jm, jp; and three hooks,
//   PV(pl, ro, kr, pos)  the value of p at plane offset pl (o, om, op), row offset ro = kr * RS (kr = the row, from 0), position pos
//                     (c, jm, jp), every argument spelt by its name here: OP_P reads L.p; pass 1 of the Krylov loop with an fp32
//                     preconditioner (mgx_krylov.hip) promotes the cycle's fp32 result instead, which lives in another layout, and
//                     finds it by those names.  With OP_P the text is, token for token, what it was with p[...] written out.
//   RHS(ko)           the row's right-hand side (ko = the row's offset in a level-1 array)
//   SINK(ro, ko, rr)  the row's sink (ro = the row's offset inside its plane; jcol = the column's j is in scope, declared where
//                     the residual has always computed it: earlier, its kernel allocates registers differently; pc_0 = the column's
//                     own p of this row, in either column text)
// ------------------------------------------------------------------------------------------------
#define OP_P(pl, ro, kr, pos) p[pl + ro + pos]
#define OP_P2(pl, ro, kr, pos, A, B) LD_PAIR(p + pl + ro + pos, A, B)
#define LOAD_ROW(PV, q, PJM, PIM, PC, A2, M3, M4, M5, N6, N7, N8)                                                                            \
  {                                                                                                                                          \
    const long long ro = (long long)((q)-1) * RS;                                                                                            \
    PJM = PV(o, ro, (q)-1, jm); PIM = PV(om, ro, (q)-1, c); PC = PV(o, ro, (q)-1, c); A2 = a2[o + ro + c];                                   \
    const double pj_ = PV(o, ro, (q)-1, jp), pi_ = PV(op, ro, (q)-1, c);                                                                     \
    M3 = a3[o + ro + jp] * pj_; M4 = a4[o + ro + jp] * pj_; M5 = a5[o + ro + jp] * pj_;                                                      \
    N6 = a6[op + ro + c] * pi_; N7 = a7[op + ro + c] * pi_; N8 = a8[op + ro + c] * pi_;                                                      \
  }
#define OP_COLUMN(PV, RHS, SINK)                                                                                                             \
  {                                                                                                                                          \
    const long long RS = L.RS;                                                                                                               \
    const int nz = L.nz;                                                                                                                     \
    const double *__restrict__ p = L.p;                                                                                                      \
    const double *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1], *__restrict__ a3 = L.cA[2],                                         \
                 *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4], *__restrict__ a6 = L.cA[5],                                         \
                 *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7];                                                                     \
    const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;                                                          \
    double pjm_m, pjm_0, pjm_p, pim_m, pim_0, pim_p, pc_m, pc_0, pc_p, a2_0, a2_p;                                                           \
    double m3_m, m3_0, m4_0, m5_p, n6_m, n6_0, n7_0, n8_p, m3_p, m4_p, n6_p, n7_p;                                                           \
    double dum5, dum8;                                                                                                                       \
    LOAD_ROW(PV, 1, pjm_0, pim_0, pc_0, a2_0, m3_0, m4_0, dum5, n6_0, n7_0, dum8);                                                           \
    LOAD_ROW(PV, 2, pjm_p, pim_p, pc_p, a2_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);                                                           \
    (void)dum5; (void)dum8;                                                                                                                  \
    /* k = 1 (:464-482) */                                                                                                                   \
    double rr = ROW_RHS_FIRST(RHS(o + c) - a1[o + c] * pc_0 - a2_p * pc_p, ST_TERMS(o + c));                                                 \
    if (REAL)                                                                                                                                \
      rr = rr - a5[o + c] * PV(om, 0, 0, jp) - a5[op + jm] * PV(op, 0, 0, jm) - a8[o + c] * PV(om, 0, 0, jm) - a8[op + jp] * PV(op, 0, 0, jp); \
    const int jcol = jodd ? 2 * jh + 1 : 2 * jh + 2;  /* the column's j, for a sink that stores the physical images */                       \
    SINK(0, o + c, rr)                                                                                                                       \
    for (int k = 2; k <= nz - 1; k++) {  /* (:484-496) */                                                                                    \
      pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p; pc_m = pc_0; pc_0 = pc_p; a2_0 = a2_p;                                     \
      m3_m = m3_0; m3_0 = m3_p; m4_0 = m4_p; n6_m = n6_0; n6_0 = n6_p; n7_0 = n7_p;                                                          \
      LOAD_ROW(PV, k + 1, pjm_p, pim_p, pc_p, a2_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);                                                     \
      const long long ko = o + (long long)(k - 1) * RS + c;                                                                                  \
      rr = ROW_RHS_MID(RHS(ko) - a1[ko] * pc_0 - a2_0 * pc_m - a2_p * pc_p, ST_TERMS(ko));                                                   \
      SINK((long long)(k - 1) * RS, ko, rr)                                                                                                  \
    }                                                                                                                                        \
    {  /* k = nz (:498-509) */                                                                                                               \
      pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p; pc_m = pc_0; pc_0 = pc_p; a2_0 = a2_p;                                     \
      m3_m = m3_0; m4_0 = m4_p; n6_m = n6_0; n7_0 = n7_p;                                                                                    \
      const long long ko = o + (long long)(nz - 1) * RS + c;                                                                                 \
      rr = ROW_RHS_LAST(RHS(ko) - a1[ko] * pc_0 - a2_0 * pc_m, ST_TERMS(ko));                                                                \
      SINK((long long)(nz - 1) * RS, ko, rr)                                                                                                 \
    }                                                                                                                                        \
  }

// ------------------------------------------------------------------------------------------------
// The column with matrix-free cross terms (see mgx_relax_common.h): 17 streams per cell instead of 22.  The diagonal of the interior rows
// is rebuilt from the fourteen couplings the row holds anyway (mg_define_matrix.f90:632-639, summed in the reference's order: the same
// bits as the stored slot 1 -- as the smoother and the fused residual+restriction do); rows 1 and nz, whose formula differs, read the
// stored one.  The j-1 / j+1 neighbours of p and zy sit side by side in the other half-row: one 16-byte load each.  What only this lane
// reads (a2, the right-hand side) is streamed past the caches on a level that does not fit them.
// The caller has in scope: REAL (compile-time); L, i, c, jm, jp, stream; PV as above, PV2(pl, ro, kr, pos, A, B) = the values at pos and
// pos + 1 into A and B (OP_P2: one 16-byte load), and two hooks,
//   RHS_LOAD(ko)      the request for the row's right-hand side, issued one step ahead with the row's own values (a load or a constant)
//   SINK(ro, ko, rr)  the row's sink
// ------------------------------------------------------------------------------------------------
#define LOAD_WIN(PV, PV2, q, PC, PJM, PIM, PJP, PIP, ZY, ZX, A2)                                                                                      \
  { const long long ro = (long long)(((q) <= nz ? (q) : nz) - 1) * RS;                                                                       \
    const int kr = ((q) <= nz ? (q) : nz) - 1;                                                                                               \
    PC = PV(o, ro, kr, c); PV2(o, ro, kr, jm, PJM, PJP) PIM = PV(om, ro, kr, c); PIP = PV(op, ro, kr, c);                                    \
    ZY = *(zy + o + ro + c); ZX = *(zx + o + ro + c); A2 = ld_rt(a2 + o + ro + c, stream); }
#define LOAD_ROWV(RHS_LOAD, q, ZYJM, ZYJP, ZXIM, ZXIP, A4O, A4JP, A7O, A7IP, BK)                                                             \
  { const long long ro = (long long)(((q) <= nz ? (q) : nz) - 1) * RS, ko = o + ro + c;                                                      \
    LD_PAIR(zy + o + ro + jm, ZYJM, ZYJP) ZXIM = zx[om + ro + c]; ZXIP = zx[op + ro + c];                                                    \
    A4O = *(a4 + ko); A4JP = a4[o + ro + jp]; A7O = *(a7 + ko); A7IP = a7[op + ro + c]; BK = RHS_LOAD(ko); }
// MF_TERMS (mgx_device.h) with the cross coefficients spelt where they are used, for rows 1 and nz of OP_COLUMN_MF: named first
// (MF_CROSS_COEF), they reach the compiler in another order and the three kernels of this text (six instances) compile differently
// (DESIGN.md 2.1).  Like the other term lists it stays defined: OP_COLUMN_MF expands it where a kernel expands OP_COLUMN_MF.
#define MF_TERMS_INLINE (qrt * (zy_p + zyjm)) * pjm_p, (qrt * (zyjp + zy_m)) * pjp_m, a4o * pjm_0, a4jp * pjp_0, (-qrt * (zy_m + zyjm)) * pjm_m, \
                        (-qrt * (zyjp + zy_p)) * pjp_p, (qrt * (zx_p + zxim)) * pim_p, (qrt * (zxip + zx_m)) * pip_m, a7o * pim_0, a7ip * pip_0, \
                        (-qrt * (zx_m + zxim)) * pim_m, (-qrt * (zxip + zx_p)) * pip_p
#define OP_COLUMN_MF(PV, PV2, RHS_LOAD, SINK)                                                                                               \
  {                                                                                                                                          \
    const long long RS = L.RS;                                                                                                               \
    const int nz = L.nz;                                                                                                                     \
    const double *__restrict__ p = L.p;                                                                                                      \
    const double *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1], *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4],             \
                 *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7], *__restrict__ zy = L.zy, *__restrict__ zx = L.zx;                   \
    const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;                                                          \
    const double qrt = 0.25;                                                                                                                 \
    /* Every request is unconditional (rows past the top clamped to nz, never used) and issued ONE STEP before its first use: the window row */ \
    /* k+2 and the own-row values of k+1 are in flight while row k is computed.  (A request inside `if (k + 2 <= nz)` made the number of */  \
    /* outstanding loads path-dependent: the compiler then waits for vmcnt(0) at every step and the look-ahead is void.) */                  \
    double pc_m = 0, pc_0, pc_p, pc_n, pjm_m = 0, pjm_0, pjm_p, pjm_n, pim_m = 0, pim_0, pim_p, pim_n, pjp_m = 0, pjp_0, pjp_p, pjp_n, pip_m = 0, pip_0, pip_p, pip_n; \
    double zy_m = 0, zy_0, zy_p, zy_n, zx_m = 0, zx_0, zx_p, zx_n, a2_0, a2_p, a2_n;                                                         \
    double zyjm, zyjp, zxim, zxip, a4o, a4jp, a7o, a7ip, bk, zyjm_n, zyjp_n, zxim_n, zxip_n, a4o_n, a4jp_n, a7o_n, a7ip_n, bk_n;             \
    /* rows 1 and nz: stored diagonal; row 1: the k = 1 diagonal slots and the four corner values of p (cmatrix = 'real', mg_relax.f90:475-479) */ \
    const double d_first = a1[o + c], d_last = a1[o + (long long)(nz - 1) * RS + c];                                                         \
    double e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0, e6 = 0, e7 = 0;                                                                   \
    if (REAL) { e0 = a5[o + c]; e1 = PV(om, 0, 0, jp); e2 = a5[op + jm]; e3 = PV(op, 0, 0, jm); e4 = a8[o + c]; e5 = PV(om, 0, 0, jm); e6 = a8[op + jp]; e7 = PV(op, 0, 0, jp); } \
    LOAD_WIN(PV, PV2, 1, pc_0, pjm_0, pim_0, pjp_0, pip_0, zy_0, zx_0, a2_0)                                                                          \
    LOAD_ROWV(RHS_LOAD, 1, zyjm, zyjp, zxim, zxip, a4o, a4jp, a7o, a7ip, bk)                                                                 \
    LOAD_WIN(PV, PV2, 2, pc_p, pjm_p, pim_p, pjp_p, pip_p, zy_p, zx_p, a2_p)                                                                 \
    for (int k = 1; k <= nz; k++) {                                                                                                          \
      const long long ro = (long long)(k - 1) * RS, ko = o + ro + c;                                                                         \
      LOAD_WIN(PV, PV2, k + 2, pc_n, pjm_n, pim_n, pjp_n, pip_n, zy_n, zx_n, a2_n)                                                           \
      LOAD_ROWV(RHS_LOAD, k + 1, zyjm_n, zyjp_n, zxim_n, zxip_n, a4o_n, a4jp_n, a7o_n, a7ip_n, bk_n)                                         \
      double rr;                                                                                                                             \
      if (k == 1) {                                                                                                                          \
        rr = ROW_RHS_FIRST(bk - d_first * pc_0 - a2_p * pc_p, MF_TERMS_INLINE);                                                              \
        if (REAL) rr = rr - e0 * e1 - e2 * e3 - e4 * e5 - e6 * e7;                                                                           \
      } else if (k < nz) {                                                                                                                   \
        MF_CROSS_COEF(zy_m, zy_p, zyjm, zyjp, zx_m, zx_p, zxim, zxip)                                                                        \
        const double dk = -a2_0 - a2_p - a4o - a4jp - a7o - a7ip - c6 - c6m - c8 - c8m - c3 - c3m - c5 - c5m;  /* = cA(1,k,j,i), mg_define_matrix.f90:632-639 */ \
        rr = ROW_RHS_MID(bk - dk * pc_0 - a2_0 * pc_m - a2_p * pc_p, MF_TERMS);                                                              \
      } else {                                                                                                                               \
        rr = ROW_RHS_LAST(bk - d_last * pc_0 - a2_0 * pc_m, MF_TERMS_INLINE);                                                                \
      }                                                                                                                                      \
      SINK(ro, ko, rr)                                                                                                                       \
      pc_m = pc_0; pc_0 = pc_p; pc_p = pc_n; pjm_m = pjm_0; pjm_0 = pjm_p; pjm_p = pjm_n; pim_m = pim_0; pim_0 = pim_p; pim_p = pim_n;       \
      pjp_m = pjp_0; pjp_0 = pjp_p; pjp_p = pjp_n; pip_m = pip_0; pip_0 = pip_p; pip_p = pip_n;                                              \
      zy_m = zy_0; zy_0 = zy_p; zy_p = zy_n; zx_m = zx_0; zx_0 = zx_p; zx_p = zx_n; a2_0 = a2_p; a2_p = a2_n;                                \
      zyjm = zyjm_n; zyjp = zyjp_n; zxim = zxim_n; zxip = zxip_n; a4o = a4o_n; a4jp = a4jp_n; a7o = a7o_n; a7ip = a7ip_n; bk = bk_n;         \
    }                                                                                                                                        \
  }
