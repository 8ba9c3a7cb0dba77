// Down leg of the V-cycle in one kernel: residual r = b - A p of the fine level (mg_relax.f90:421-515) and its restriction to
// the coarse right-hand side, b_c = sum of the 8 fine r (mg_intergrids.f90:139-162), without r ever leaving the chip.
//
// Vcycle discards the residual norm (mg_solvers.f90:140) and the r of the down leg is dead: nothing but fine2coarse reads
// it, and coarse2fine overwrites it on the way up (mg_intergrids.f90:387-448).  Separately the two operators issue 18 + 1
// loads per fine cell (every neighbour value fetched again by every lane that needs it), write r and read it back, and
// stream the stored diagonal.  Here one lane owns one fine plane of a COARSE column (two fine columns jA, jB; lanes 0-31 of a
// wave take plane iA, lanes 32-63 plane iB of the same 32 coarse columns), walks it bottom to top with three-row windows in
// registers, shares the pair's p / slope / coefficient values between its two residuals (24 loads per row = 12 per
// cell), rebuilds the diagonal from the couplings (as the smoother does, mgx_relax.hip), and the 8-cell sum is closed with
// the partner lane's two values (one cross-lane exchange per row): no r traffic, no diagonal stream, one launch.
// Measured (rocprofv3, MI355X): 512x512x64 211-224 us against 279 + 36 for the two kernels (round 2: 236-250 with guarded look-ahead);
// levels of up to 256x256x64 cells take k_residual_restrict_flat below (256x256x32: 24 us against 47 + 13).
// The residuals expand ROW_RHS_* and MF_CROSS_COEF (mgx_device.h) and the 8-term sum keeps the reference's order: b_c is bit-identical to
// compute_residual followed by fine2coarse.  Matrix-free cross terms (needs the slopes zy, zx: the matrix must be the one
// define_matrices built); other cases keep the two separate kernels.  The norm of the closing residual (NORM) is bit-identical too:
// here and in k_residual / k_residual_mf the sum of r^2 is carried as a pair and rounded once (dd_add, mgx_device.h), so the way a
// kernel groups the cells does not reach it.
// ZW (the walking form without the norm, where the level carries the 2-D factors and sigma tables of the smoother's ZW form): the
// interior rows of slots 4 and 7 are not streamed either but generated from the depth formula, with the smoother's expressions
// (ZW_GEN, SLOT47_GEN, RCP_REF, DIVC of mgx_device.h, which MF_ROW of mgx_relax_common.h expands too) -- same bits, 755 MB moved instead of 1005 (FETCH x 2 + WRITE)
// and 197-199 us instead of 216-219 at 512x512x64.  The kernel then issues ~650 instructions per row on its one wave per SIMD: it is
// bound by issue, not by its 3.8 TB/s, which is why a quarter less traffic buys a tenth of the time (profiles/resrest_zw.json).
#include "mgx_switches.h"
#include "mgx_device.h"
#include "mgx_choice.h"

namespace {

// One lane = one fine plane (iA for lanes 0-31, iB for lanes 32-63 of the wave) of a coarse column: two fine columns jA, jB.
// values of one fine row needed with their k-1 / k+1 neighbours (three-row windows)
struct RowW {
  double P[4];      // p of the own plane at j = jA-1, jA, jB, jB+1
  double Pm[2];     // p of plane i-1 at jA, jB
  double Pp[2];     // p of plane i+1
  double ZY4[4];    // slopes zy of the own plane at jA-1, jA, jB, jB+1 (the inner two with their k-1 / k+1 neighbours)
  double ZX[2];     // own slopes zx at jA, jB
  double A2[2];     // slot 2 (couples k with k-1)
};
// values needed at the row itself only
struct RowR {
  double ZXm[2];    // zx of plane i-1 at jA, jB
  double ZXp[2];    // zx of plane i+1
  double A4[3];     // slot 4 at jA, jB, jB+1
  double A7[2];     // slot 7 own plane at jA, jB
  double A7p[2];    // slot 7 of plane i+1
  double B[2];
};

struct Geo {
  long long o, om, op;  // plane offsets of i, i-1, i+1
  int c[4];             // row positions of jA-1, jA, jB, jB+1
};

// jA-1 and jB sit side by side in the even half-row, jA and jB+1 in the odd one (c[2] = c[0] + 1, c[3] = c[1] + 1): one 16-byte
// load per pair instead of two 8-byte loads whose wave-wide footprints overlap
__device__ __forceinline__ void load_w(RowW &w, const LevView &F, const Geo &g, const long long ro) {
  const double *__restrict__ p = F.p, *__restrict__ zy = F.zy, *__restrict__ zx = F.zx, *__restrict__ a2 = F.cA[1];
  LD_PAIR(p + g.o + ro + g.c[0], w.P[0], w.P[2])
  LD_PAIR(p + g.o + ro + g.c[1], w.P[1], w.P[3])
  LD_PAIR(zy + g.o + ro + g.c[0], w.ZY4[0], w.ZY4[2])
  LD_PAIR(zy + g.o + ro + g.c[1], w.ZY4[1], w.ZY4[3])
#pragma unroll
  for (int jj = 0; jj < 2; jj++) {
    const long long e = g.o + ro + g.c[jj + 1];
    w.Pm[jj] = p[g.om + ro + g.c[jj + 1]]; w.Pp[jj] = p[g.op + ro + g.c[jj + 1]];
    w.ZX[jj] = zx[e]; w.A2[jj] = a2[e];
  }
}

// ZW: without slots 4 and 7 (the walking form generates them, k_residual_restrict)
template <bool ZW = false>
__device__ __forceinline__ void load_r(RowR &r, const LevView &F, const Geo &g, const long long ro) {
  const double *__restrict__ b = F.b, *__restrict__ zx = F.zx, *__restrict__ a4 = F.cA[3], *__restrict__ a7 = F.cA[6];
  if (!ZW) {
    LD_PAIR(a4 + g.o + ro + g.c[1], r.A4[0], r.A4[2])
    r.A4[1] = a4[g.o + ro + g.c[2]];
  }
#pragma unroll
  for (int jj = 0; jj < 2; jj++) {
    const int c = g.c[jj + 1];
    r.ZXm[jj] = zx[g.om + ro + c]; r.ZXp[jj] = zx[g.op + ro + c];
    if (!ZW) { r.A7[jj] = a7[g.o + ro + c]; r.A7p[jj] = a7[g.op + ro + c]; }
    r.B[jj] = b[g.o + ro + c];
  }
}
// slots 4 and 7 of one row alone (ZW: rows 1 and nz, whose formulas differ, stay stored)
__device__ __forceinline__ void load_s(RowR &r, const LevView &F, const Geo &g, const long long ro) {
  const double *__restrict__ a4 = F.cA[3], *__restrict__ a7 = F.cA[6];
  LD_PAIR(a4 + g.o + ro + g.c[1], r.A4[0], r.A4[2])
  r.A4[1] = a4[g.o + ro + g.c[2]];
#pragma unroll
  for (int jj = 0; jj < 2; jj++) { const int c = g.c[jj + 1]; r.A7[jj] = a7[g.o + ro + c]; r.A7p[jj] = a7[g.op + ro + c]; }
}

// the value of lane ^ m, every lane of the wave active: what __shfl_xor(x, m, 64) moves, without its width test, whose operands the
// walking form's ZW instance has no registers to keep
__device__ __forceinline__ double lane_xor(double x, int m) {
  const int idx = (__lane_id() ^ m) << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(idx, __double2loint(x)), hi = __builtin_amdgcn_ds_bpermute(idx, __double2hiint(x));
  return __hiloint2double(hi, lo);
}
#define RR_XOR(x, m) (ZW ? lane_xor(x, m) : __shfl_xor(x, m, 64))

}  // namespace

// grid: 1-D, gx j-chunks of 32 coarse columns x gy groups of blockDim.y coarse planes, XCD-aware as k_relax_nz.
// One wave per SIMD (AW = AR = 1: four window rows + two row buffers, ~450 registers with the requests kept ahead of their use;
// squeezed to 256 registers for two waves per SIMD it spills and loses: 250 vs 236 us at 512x512x64 in round 2).
// ZW: 496 registers, no scratch, 18 KB of LDS -- six depth columns per lane (two more come from the partner lane), both depth rows of a
// step generated at the step, row nz's stored values parked in LDS; AW = AR = 1 and no NORM (neither fits beside it).
// NORM: also the sum of r^2 over the block's fine cells, as a pair -> partial[blockIdx.x], partial[gridDim.x + blockIdx.x] (the closing compute_residual of a solve_p iteration,
// mg_solvers.f90:65, whose r the next Fcycle restricts first thing, :112-115: one pass over the level instead of two and no r written).
// dup: a second destination of the coarse sums (Fcycle's grid(lev+1)%r = grid(lev+1)%b, :113).
template <bool REAL, int AW, int AR, bool NORM = false, bool ZW = false>
__global__ __launch_bounds__(256, 1) void k_residual_restrict(LevView F, LevView C, double *__restrict__ dst, Sides ph, double *__restrict__ zero, int gx, int gy,
                                                             double *__restrict__ partial = nullptr, double *__restrict__ dup = nullptr) {
  __shared__ double red_ss[8];  // the waves' sums of r^2, pairs (dd_add, mgx_device.h): hi 0-3, lo 4-7
  // ZW without NORM only: with the lane's sum of r^2 beside everything else the form does not fit the registers, and with that sum kept
  // in LDS (one read and one write per row) it fits and loses: solve_p 296.1 against 297.5 it/s (profiles/resrest_zw.json)
  static_assert(!(ZW && NORM), "the closing residual of solve_p streams its slots");
  // ZW: what the registers have no room to carry up the column, one entry per lane (nobody else's: no barrier): what the prologue reads
  // and row nz alone needs, the stored slots 4 / 7 of that row (0-6) and its diagonal (7, 8)
  __shared__ double park[ZW ? 9 * 256 : 1];
  const double *parked = park + threadIdx.y * 64 + threadIdx.x;
  double ss = 0.0, sl = 0.0;
  int bx, by;
  if ((gy & 7) == 0) { const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3; by = xcd * (gy >> 3) + local / gx; bx = local - (local / gx) * gx; }
  else { by = blockIdx.x / gx; bx = blockIdx.x - by * gx; }
  const int half = threadIdx.x >> 5;                     // 0: fine plane iA = 2 i2 - 1, 1: iB = 2 i2
  int j2 = 1 + bx * 32 + (threadIdx.x & 31);
  const int i2 = 1 + by * blockDim.y + threadIdx.y;
  if (i2 > C.nx) {                                       // wave-uniform
    if (NORM) { if ((threadIdx.x & 63) == 0) { red_ss[threadIdx.y] = 0.0; red_ss[4 + threadIdx.y] = 0.0; } __syncthreads(); }  // wave 0 always has a plane: it closes the block's sum
    return;
  }
  const bool live = j2 <= C.ny;
  if (!live) j2 = C.ny;                                  // ragged chunk: dead lanes shadow a live column (they take part in the shuffles), store nothing
  const int nz = F.nz;
  const long long RS = F.RS;
  Geo g;
  g.o = (long long)(2 * i2 - 1 + half) * F.plane; g.om = g.o - F.plane; g.op = g.o + F.plane;
  g.c[1] = F.HO + (j2 - 1); g.c[2] = F.EO + j2; g.c[0] = F.EO + (j2 - 1); g.c[3] = F.HO + j2;  // jA = 2 j2 - 1 (odd), jB = 2 j2 (even)
  const double qrt = 0.25;
  const double *__restrict__ a1 = F.cA[0], *__restrict__ a5 = F.cA[4], *__restrict__ a8 = F.cA[7];

  // last row: stored diagonal (its formula differs, mg_define_matrix.f90:642-654)
  double dlast[2];
#pragma unroll
  for (int jj = 0; jj < 2; jj++) dlast[jj] = a1[g.o + (long long)(nz - 1) * RS + g.c[jj + 1]];
  // first row: stored diagonal, the k = 1 diagonal slots and the four corner values of p (horizontal diagonals of cmatrix = 'real',
  // mg_relax.f90:475-479) -- requested before the rows, so that the first step does not wait for the look-ahead behind them
  double dedge[2], e[2][8];
#pragma unroll
  for (int jj = 0; jj < 2; jj++) {
    const int c = g.c[jj + 1], jm = g.c[jj], jp = g.c[jj + 2];
    dedge[jj] = a1[g.o + c];
    if (REAL) {
      e[jj][0] = a5[g.o + c]; e[jj][1] = F.p[g.om + jp]; e[jj][2] = a5[g.op + jm]; e[jj][3] = F.p[g.op + jm];
      e[jj][4] = a8[g.o + c]; e[jj][5] = F.p[g.om + jm]; e[jj][6] = a8[g.op + jp]; e[jj][7] = F.p[g.op + jp];
    }
  }
  // ZW: the stored slots 4 / 7 of rows 1 and nz (their formulas differ, mg_define_matrix.f90:361-372, 577-590); h, hinv, zeta of the
  // six depth columns (0-3: jA-1, jA, jB, jB+1 of the own plane; 4, 5: jA, jB of the FAR plane, i-1 for half 0 and i+1 for half 1);
  // the column factors of slots 4 (jA, jB, jB+1) and 7 (own plane, plane i+1) with the refined reciprocals of their divisors
  double hh[6], hv[6], hz[6];
  double m4[3], d4[3], r4[3], m7[2], d7[2], r7[2], m7p[2], d7p[2], r7p[2];
  const double *__restrict__ cffw = F.cffw, *__restrict__ csw = F.csw;
  RowR S1;
  if (ZW) {
    RowR Sn;
    load_s(S1, F, g, 0);
    load_s(Sn, F, g, (long long)(nz - 1) * RS);
    const long long q2 = (long long)(2 * i2 - 1 + half) * RS, qf = half ? q2 + RS : q2 - RS;
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
      hh[4 + jj] = F.h2[qf + g.c[jj + 1]]; hv[4 + jj] = F.hi2[qf + g.c[jj + 1]]; hz[4 + jj] = F.ze2[qf + g.c[jj + 1]];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) { hh[q] = F.h2[q2 + g.c[q]]; hv[q] = F.hi2[q2 + g.c[q]]; hz[q] = F.ze2[q2 + g.c[q]]; }
#pragma unroll
    for (int q = 0; q < 3; q++) { m4[q] = F.m4[q2 + g.c[q + 1]]; d4[q] = F.d4[q2 + g.c[q + 1]]; r4[q] = RCP_REF(d4[q]); }
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
      m7[jj] = F.m7[q2 + g.c[jj + 1]]; d7[jj] = F.d7[q2 + g.c[jj + 1]]; r7[jj] = RCP_REF(d7[jj]);
      m7p[jj] = F.m7[q2 + RS + g.c[jj + 1]]; d7p[jj] = F.d7[q2 + RS + g.c[jj + 1]]; r7p[jj] = RCP_REF(d7p[jj]);
    }
    double *mine = park + threadIdx.y * 64 + threadIdx.x;
#pragma unroll
    for (int q = 0; q < 3; q++) mine[q * 256] = Sn.A4[q];
#pragma unroll
    for (int jj = 0; jj < 2; jj++) { mine[(3 + jj) * 256] = Sn.A7[jj]; mine[(5 + jj) * 256] = Sn.A7p[jj]; mine[(7 + jj) * 256] = dlast[jj]; }
  }
  // Look-ahead: the window rows are requested AW steps and the rows' own values AR steps before their first use (A/B of the depths,
  // scripts/probe/ab_resrest_ahead.sh: (1,1) 224 us, (1,2) 233, (2,1) 225 -- once the requests are unconditional, below, the depth is
  // not what bounds the kernel).
  constexpr int NWB = 3 + AW, NRB = 1 + AR;  // buffers: rows k-1, k, k+1 + AW ahead; row k + AR ahead
  constexpr int U = (NWB % NRB == 0) ? NWB : NWB * NRB;  // steps after which both rotations are back where they started
  static_assert(U <= 12, "unroll");
  RowW W[NWB];
  RowR R[NRB];
  // before the peeled k = 1 step: W[0 .. AW+1] = rows 1 .. AW+2, R[NRB-1] = row 1, R[0 .. AR-2] = rows 2 .. AR.
  // Every request is UNCONDITIONAL (rows past the top are clamped to nz and never used): a request inside a branch makes the number of
  // outstanding loads path-dependent, the compiler then waits for vmcnt(0) at every step and the look-ahead is void (measured: one memory
  // round trip per row, whatever AW / AR).
#pragma unroll
  for (int q = 0; q < AW + 2; q++) load_w(W[q], F, g, (long long)(q + 1 <= nz ? q : nz - 1) * RS);
  load_r<ZW>(R[NRB - 1], F, g, 0);
#pragma unroll
  for (int q = 0; q < AR - 1; q++) load_r<ZW>(R[q], F, g, (long long)(q + 2 <= nz ? q + 1 : nz - 1) * RS);
  double z = 0.0;
  const long long oc = (long long)i2 * C.plane + jpos(C, j2);

  // one fine row k: Wm / W0 / Wp hold rows k-1, k, k+1; Wn receives row k+1+AW and Rn row k+AR while row k is computed
#define RR_LOADS(k, Wn, Rn)                                                                                                 \
    load_w(Wn, F, g, (long long)((k) + 1 + AW <= nz ? (k) + AW : nz - 1) * RS);                                              \
    load_r<ZW>(Rn, F, g, (long long)((k) + AR <= nz ? (k) + AR - 1 : nz - 1) * RS);
#define RR_CELL_IN(Wm, W0, Wp, R0, S4, S7, S7P)                                                                                        \
      const double pc_m = Wm.P[jj + 1], pc_0 = W0.P[jj + 1], pc_p = Wp.P[jj + 1];                                            \
      const double pjm_m = Wm.P[jj], pjm_0 = W0.P[jj], pjm_p = Wp.P[jj];                                                     \
      const double pjp_m = Wm.P[jj + 2], pjp_0 = W0.P[jj + 2], pjp_p = Wp.P[jj + 2];                                         \
      const double pim_m = Wm.Pm[jj], pim_0 = W0.Pm[jj], pim_p = Wp.Pm[jj];                                                  \
      const double pip_m = Wm.Pp[jj], pip_0 = W0.Pp[jj], pip_p = Wp.Pp[jj];                                                  \
      const double zy_m = Wm.ZY4[jj + 1], zy_p = Wp.ZY4[jj + 1], zx_m = Wm.ZX[jj], zx_p = Wp.ZX[jj];                         \
      const double zyjm = W0.ZY4[jj], zyjp = W0.ZY4[jj + 2];                                                                \
      const double zxim = R0.ZXm[jj], zxip = R0.ZXp[jj];                                                                    \
      const double a4o = S4[jj], a4jp = S4[jj + 1], a7o = S7[jj], a7ip = S7P[jj];                                            \
      const double a2_0 = W0.A2[jj], a2_p = Wp.A2[jj];                                                                      \
      MF_CROSS_COEF(zy_m, zy_p, zyjm, zyjp, zx_m, zx_p, zxim, zxip)                                                         \
      (void)pc_m; (void)pjm_m; (void)pjp_m; (void)pim_m; (void)pip_m; (void)c3m; (void)c5; (void)c6m; (void)c8; (void)a2_0;
  /* fine2coarse_3D (mg_intergrids.f90:149-160): (k,jA,iA) + (k,jA,iB) + (k,jB,iA) + (k,jB,iB), then the same of k+1;
     the iB values come from the partner lane (lane ^ 32) */
#define RR_SUM(k, r)                                                                                                        \
    if (NORM && live) { dd_add(ss, sl, r[0] * r[0]); dd_add(ss, sl, r[1] * r[1]); }                                         \
    const double rA_B = RR_XOR(r[0], 32), rB_B = RR_XOR(r[1], 32);                                                          \
    if ((k) & 1) z = r[0] + rA_B + r[1] + rB_B;                                                                             \
    else {                                                                                                                  \
      z = z + r[0] + rA_B + r[1] + rB_B;                                                                                    \
      if (half == 0 && live) {                                                                                              \
        const long long rc = (long long)(((k) >> 1) - 1) * C.RS;                                                            \
        dst[oc + rc] = z;                                                                                                   \
        mirror_store(C, dst, rc, j2, i2, jpos(C, j2), z, ph);                                                               \
        if (dup) { dup[oc + rc] = z; mirror_store(C, dup, rc, j2, i2, jpos(C, j2), z, ph); }                                 \
        if (zero) { zero[oc + rc] = 0.0; mirror_store(C, zero, rc, j2, i2, jpos(C, j2), 0.0, ph); }                          \
      }                                                                                                                     \
    }
  /* interior rows, mg_relax.f90:484-496; diagonal = minus the sum of the fourteen couplings (mg_define_matrix.f90:632-639) */
#define RR_GENERAL(rr, R0)                                                                                                  \
      {                                                                                                                     \
        const double dk = -a2_0 - a2_p - a4o - a4jp - a7o - a7ip - c6 - c6m - c8 - c8m - c3 - c3m - c5 - c5m;               \
        rr = ROW_RHS_MID(R0.B[jj] - dk * pc_0 - a2_0 * pc_m - a2_p * pc_p, MF_TERMS);                                       \
      }
  /* last row, :498-509 (stored diagonal) */
#define RR_LAST(rr, R0, DL) { rr = ROW_RHS_LAST(R0.B[jj] - (DL) * pc_0 - a2_0 * pc_m, MF_TERMS); }
  /* first row, :464-482 (stored diagonal; E = the row's four k = 1 diagonal slots, each followed by its corner value of p) */
#define RR_FIRST(rr, R0, DE, E)                                                                                             \
      {                                                                                                                     \
        rr = ROW_RHS_FIRST(R0.B[jj] - (DE) * pc_0 - a2_p * pc_p, MF_TERMS);                                                 \
        if (REAL) rr = rr - E[0] * E[1] - E[2] * E[3] - E[4] * E[5] - E[6] * E[7];                                          \
      }
  /* ZW: zw of row kk (mg_zr_zw.f90:140-145, ZW_GEN of mgx_device.h) at jA-1, jA, jB, jB+1 of the own plane (zo) and at jA, jB of planes
     i-1 (zm) and i+1 (zp).  One of the two is the partner's plane (lane ^ 32: i+1 for half 0, i-1 for half 1), whose depths are the
     partner's own zo[1], zo[2]; the far one is generated here.  A select, not a branch: both halves take part in the exchange. */
#define RR_ZW_ROW(kk, zo, zm, zp)                                                                                           \
    {                                                                                                                       \
      const int kz_ = (kk);  /* the caller's row expression may name q */                                                   \
      _Pragma("unroll") for (int q = 0; q < 4; q++) zo[q] = ZW_GEN(kz_, q);                                                  \
      _Pragma("unroll") for (int jj = 0; jj < 2; jj++) {                                                                     \
        double zf_;                                                                                                         \
        zf_ = ZW_GEN(kz_, 4 + jj);                                                                                                       \
        const double zx_ = lane_xor(zo[jj + 1], 32);                                                                        \
        zm[jj] = half ? zx_ : zf_; zp[jj] = half ? zf_ : zx_;                                                               \
      }                                                                                                                     \
    }
  /* ZW: slots 4 and 7 of row k (a4 at jA, jB, jB+1; a7 at jA, jB of the own plane and of plane i+1), not streamed: the interior formula
     (mg_define_matrix.f90:532-534, 549-551: SLOT47_GEN of mgx_device.h, which MF_ROW expands too), on zw of rows k and k+1 -- both generated at
     the step: a carried row k costs 16 registers that the walk does not have; row nz from where the prologue parked it */
#define RR_SLOTS(k)                                                                                                         \
    double s4[3], s7[2], s7p[2];                                                                                            \
    if (!ZW) ;                                                                                                              \
    else if ((k) < nz) {                                                                                                    \
      double zlo[4], zlm[2], zlp[2], zhi[4], zhm[2], zhp[2];                                                                \
      RR_ZW_ROW(k, zlo, zlm, zlp)                                                                                           \
      RR_ZW_ROW((k) + 1, zhi, zhm, zhp)                                                                                     \
      _Pragma("unroll") for (int q = 0; q < 3; q++) s4[q] = SLOT47_GEN(zhi[q + 1], zlo[q + 1], zhi[q], zlo[q], m4[q], d4[q], r4[q]); \
      _Pragma("unroll") for (int jj = 0; jj < 2; jj++) {                                                                     \
        s7[jj] = SLOT47_GEN(zhi[jj + 1], zlo[jj + 1], zhm[jj], zlm[jj], m7[jj], d7[jj], r7[jj]);                             \
        s7p[jj] = SLOT47_GEN(zhp[jj], zlp[jj], zhi[jj + 1], zlo[jj + 1], m7p[jj], d7p[jj], r7p[jj]);                         \
      }                                                                                                                     \
    } else { _Pragma("unroll") for (int q = 0; q < 3; q++) s4[q] = parked[q * 256];                                          \
             _Pragma("unroll") for (int jj = 0; jj < 2; jj++) { s7[jj] = parked[(3 + jj) * 256]; s7p[jj] = parked[(5 + jj) * 256]; } }
#define RR_STEP(k, Wm, W0, Wp, Wn, R0, Rn)                                                                                  \
  {                                                                                                                         \
    RR_LOADS(k, Wn, Rn)                                                                                                     \
    RR_SLOTS(k)                                                                                                             \
    double r[2];                                                                                                            \
    _Pragma("unroll") for (int jj = 0; jj < 2; jj++) {                                                                     \
      RR_CELL_IN(Wm, W0, Wp, R0, (ZW ? s4 : R0.A4), (ZW ? s7 : R0.A7), (ZW ? s7p : R0.A7p))                                      \
      double rr;                                                                                                            \
      if ((k) < nz) RR_GENERAL(rr, R0)                                                                                       \
      else RR_LAST(rr, R0, ZW ? parked[(7 + jj) * 256] : dlast[jj])                                                         \
      r[jj] = rr;                                                                                                           \
    }                                                                                                                       \
    RR_SUM(k, r)                                                                                                            \
  }
  {  // k = 1 (mg_relax.f90:464-482), peeled
    RR_LOADS(1, W[AW + 2], R[AR - 1])
    const RowR &R1 = ZW ? S1 : R[NRB - 1];
    double r[2];
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
      RR_CELL_IN(W[0], W[0], W[1], R[NRB - 1], R1.A4, R1.A7, R1.A7p)
      double rr;
      RR_FIRST(rr, R[NRB - 1], dedge[jj], e[jj])
      r[jj] = rr;
    }
    RR_SUM(1, r)
  }
  // rows 2 .. nz, U steps per trip: at step q of a trip rows k-1, k, k+1 sit in W[q], W[q+1], W[q+2] (mod NWB) and row k's own values in
  // R[q mod NRB].  Whole trips run without a branch around a step; the last nz - 1 mod U rows follow, guarded (the rotation is back at 0).
  int k = 2;
  for (; k + U - 1 <= nz; k += U) {
#pragma unroll
    for (int q = 0; q < U; q++) RR_STEP(k + q, W[q % NWB], W[(q + 1) % NWB], W[(q + 2) % NWB], W[(q + 2 + AW) % NWB], R[q % NRB], R[(q + AR) % NRB])
  }
#pragma unroll
  for (int q = 0; q < U - 1; q++) {
    if (k + q <= nz) RR_STEP(k + q, W[q % NWB], W[(q + 1) % NWB], W[(q + 2) % NWB], W[(q + 2 + AW) % NWB], R[q % NRB], R[(q + AR) % NRB])
  }
#undef RR_STEP
#undef RR_SLOTS
#undef RR_ZW_ROW
#undef RR_LOADS
  if (NORM) {  // wave sum, then the block's four waves: pairs throughout, so the grouping does not show in the norm (dd_add, mgx_device.h)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double oh = __shfl_xor(ss, off, 64), ol = __shfl_xor(sl, off, 64); dd_merge(ss, sl, oh, ol); }
    if ((threadIdx.x & 63) == 0) { red_ss[threadIdx.y] = ss; red_ss[4 + threadIdx.y] = sl; }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
      for (int w = 1; w < 4; w++) dd_merge(ss, sl, red_ss[w], red_ss[4 + w]);
      partial[blockIdx.x] = ss; partial[gridDim.x + blockIdx.x] = sl;
    }
  }
}

// The same operator without the walk.  A lane that climbs its column pays one memory round trip per row step (20 us for nz = 16 and 13 us
// for nz = 8 on 8-32 CUs, measured), but nothing in r = b - A p is sequential in k.  Here one wave owns S fine rows (S/2 coarse rows) of 32
// coarse columns (both fine planes, as above): the S + 2 window rows and the S rows' own values are all requested at once, the rows are
// computed and the 8-cell sums closed with the partner lane -- one round trip, nz/S times the waves.  The rows are RR_FIRST / RR_GENERAL /
// RR_LAST above: bit-identical.
template <bool REAL, int S, bool NORM = false>
__global__ __launch_bounds__(64) void k_residual_restrict_flat(LevView F, LevView C, double *__restrict__ dst, Sides ph, double *__restrict__ zero, int gx,
                                                              double *__restrict__ partial = nullptr, double *__restrict__ dup = nullptr) {
  constexpr bool ZW = false;  // the flat form streams its slots
  double ss = 0.0, sl = 0.0;
  // 1-D grid, k fastest: the nz/S waves of one (plane, j-chunk) share two of their window rows with the wave above and below, so they
  // are kept together in time and on ONE XCD (workgroups are dealt to the eight XCDs round-robin), where that re-use is an L2 hit
  const int nz = F.nz, nks = (nz + S - 1) / S, ng = gx * C.nx;
  int grp, ks;
  if ((ng & 7) == 0) { const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3; ks = local % nks; grp = xcd * (ng >> 3) + local / nks; }
  else { ks = blockIdx.x % nks; grp = blockIdx.x / nks; }
  const int i2 = 1 + grp / gx, bx = grp - (grp / gx) * gx;
  const int half = threadIdx.x >> 5;
  int j2 = 1 + bx * 32 + (threadIdx.x & 31);
  const bool live = j2 <= C.ny;
  if (!live) j2 = C.ny;
  const int k = ks * S + 1;  // fine rows k (odd) .. k + S - 1 (those <= nz; nz is even)
  const long long RS = F.RS;
  Geo g;
  g.o = (long long)(2 * i2 - 1 + half) * F.plane; g.om = g.o - F.plane; g.op = g.o + F.plane;
  g.c[1] = F.HO + (j2 - 1); g.c[2] = F.EO + j2; g.c[0] = F.EO + (j2 - 1); g.c[3] = F.HO + j2;
  const double qrt = 0.25;
  const double *__restrict__ a1 = F.cA[0], *__restrict__ a5 = F.cA[4], *__restrict__ a8 = F.cA[7];
  RowW W[S + 2];  // rows k-1 .. k+S, clamped to 1 .. nz (the clamped copies are never used: the first and the last row have their own expressions)
  RowR R[S];
#pragma unroll
  for (int r = 0; r < S + 2; r++) {
    const int kr = k - 1 + r < 1 ? 1 : (k - 1 + r > nz ? nz : k - 1 + r);
    load_w(W[r], F, g, (long long)(kr - 1) * RS);
  }
#pragma unroll
  for (int r = 0; r < S; r++) {
    const int kr = k + r > nz ? nz : k + r;
    load_r(R[r], F, g, (long long)(kr - 1) * RS);
  }
  double dedge[2] = {0.0, 0.0}, e[2][8];
  if (k == 1) {
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
      const int c = g.c[jj + 1], jm = g.c[jj], jp = g.c[jj + 2];
      dedge[jj] = a1[g.o + c];
      if (REAL) {
        e[jj][0] = a5[g.o + c]; e[jj][1] = F.p[g.om + jp]; e[jj][2] = a5[g.op + jm]; e[jj][3] = F.p[g.op + jm];
        e[jj][4] = a8[g.o + c]; e[jj][5] = F.p[g.om + jm]; e[jj][6] = a8[g.op + jp]; e[jj][7] = F.p[g.op + jp];
      }
    }
  }
  double dlast[2] = {0.0, 0.0};
  if (k + S > nz) {
#pragma unroll
    for (int jj = 0; jj < 2; jj++) dlast[jj] = a1[g.o + (long long)(nz - 1) * RS + g.c[jj + 1]];
  }
  double z = 0.0;
  const long long oc = (long long)i2 * C.plane + jpos(C, j2);
#pragma unroll
  for (int r = 0; r < S; r++) {
    const int kr = k + r;
    if (kr <= nz) {  // wave-uniform
      double rv[2];
#pragma unroll
      for (int jj = 0; jj < 2; jj++) {
        RR_CELL_IN(W[r], W[r + 1], W[r + 2], R[r], R[r].A4, R[r].A7, R[r].A7p)
        double rr;
        if (r == 0 && kr == 1) RR_FIRST(rr, R[r], dedge[jj], e[jj])
        else if (kr < nz) RR_GENERAL(rr, R[r])
        else RR_LAST(rr, R[r], dlast[jj])
        rv[jj] = rr;
      }
      RR_SUM(kr, rv)  /* odd row: z = its four values; even row: z += its four values, store coarse row kr/2 */
    }
  }
  if (NORM) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double oh = __shfl_xor(ss, off, 64), ol = __shfl_xor(sl, off, 64); dd_merge(ss, sl, oh, ol); }
    if (threadIdx.x == 0) { partial[blockIdx.x] = ss; partial[gridDim.x + blockIdx.x] = sl; }
  }
}
#undef RR_SUM
#undef RR_XOR
#undef RR_CELL_IN
#undef RR_GENERAL
#undef RR_LAST
#undef RR_FIRST

// ---- the launcher: an RrChoice (mgx_choice.h) to its template instance ----
// the flat form with S = 4, 2; the walking form with the look-aheads (AW, AR) = (1, 1), (1, 2), (2, 1), and with generated slots 4 and 7 the
// one instance that has the registers for them: (1, 1) without the norm
static void launch_resrest(hipStream_t st, const LevView *F, const LevView *C, const RrChoice &c, double *dst, Sides ph, double *zero, double *partial, double *dup) {
  with_bool(c.real, [&](auto R) {
    constexpr bool REAL = decltype(R)::value;
    if (c.family == KF_RR_FLAT) {
      with_int<4, 2>(c.s, [&](auto SV) {
        with_bool(c.norm, [&](auto N) {
          hipLaunchKernelGGL((k_residual_restrict_flat<REAL, decltype(SV)::value, decltype(N)::value>), dim3(c.grid), dim3(WAVE), 0, st, *F, *C, dst, ph, zero, c.gx, partial, dup);
        });
      });
      return;
    }
    const dim3 grd(c.grid), blk(WAVE, c.by);
    if (c.zw) { hipLaunchKernelGGL((k_residual_restrict<REAL, 1, 1, false, true>), grd, blk, 0, st, *F, *C, dst, ph, zero, c.gx, c.gy, partial, dup); return; }
    with_bool(c.norm, [&](auto N) {
      constexpr bool NORM = decltype(N)::value;
      if (c.aw == 2) hipLaunchKernelGGL((k_residual_restrict<REAL, 2, 1, NORM, false>), grd, blk, 0, st, *F, *C, dst, ph, zero, c.gx, c.gy, partial, dup);
      else if (c.ar == 2) hipLaunchKernelGGL((k_residual_restrict<REAL, 1, 2, NORM, false>), grd, blk, 0, st, *F, *C, dst, ph, zero, c.gx, c.gy, partial, dup);
      else hipLaunchKernelGGL((k_residual_restrict<REAL, 1, 1, NORM, false>), grd, blk, 0, st, *F, *C, dst, ph, zero, c.gx, c.gy, partial, dup);
    });
  });
}

extern "C" {

// workgroups (= pairs of norm partials) of the launch below, for a caller that sums r^2
int mgxk_residual_restrict_grid(const LevView *F, const LevView *C) { return (int)choose_resrest(lev_shape(F), lev_shape(C), 1, true, mgx_switches()).grid; }
// returns 1 when launched (choose_resrest, mgx_choice.h), 0 = use mgxk_residual + mgxk_fine2coarse
// partial != nullptr: also sum r^2 (partials, one pair per workgroup: room for twice mgxk_residual_restrict_grid()); dup: second destination of the coarse sums
int mgxk_residual_restrict_ex(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero, double *partial, double *dup) {
  mgx_before_launch();
  const RrChoice c = choose_resrest(lev_shape(F), lev_shape(C), real, partial != nullptr, mgx_switches());
  if (c.family == KF_NONE) return 0;
  launch_resrest(st, F, C, c, dst, ph, zero, partial, dup);
  return mgx_launched();
}
int mgxk_residual_restrict(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero) {
  return mgxk_residual_restrict_ex(st, F, C, dst, real, ph, zero, nullptr, nullptr);
}

}  // extern "C"
