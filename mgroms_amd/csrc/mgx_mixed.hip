// fp32 kernels of the mixed-precision solve_p (option "cycle_precision" = 32, include/mgx.h).  The fp64 outer loop of
// mgx_cycle.cpp (solve_p_mixed) keeps the iterate, the residual, its norm and the stopping test; each iteration runs the
// reference's F-cycle in correction form, A e = s r with e = 0 on entry, on fp32 shadows of every level (LevView32,
// mgx_internal.h), and adds e / s to p.  Hand-written, fp32, single rank (every side of every level physical).
//
// These kernels have no bit-parity duty: they are compiled with -ffp-contract=fast (Makefile) and sum in whatever order is
// convenient.  They keep the operator of the fp64 kernels term for term (mgx_residual.hip k_residual, mgx_relax.hip
// relax_col_any), so each one can be checked against its fp64 counterpart through mgx_mixed_op.
//
// Thread mapping as in the fp64 kernels: one lane = one (j,i) column, lanes along the unit-stride half-row of the JS layout.
#include "mgx_relax_common.h"   // XCD_BLOCK_MAP (and through it mgx_device.h)

// physical-boundary images of an interior value (homogeneous Neumann mirror incl. corners, as mirror_store; all four sides)
__device__ __forceinline__ void mirror32(const LevView32 &L, float *__restrict__ a, const long long ro, const int j, const int i, const int c, const float v) {
  const bool mS = j == 1, mN = j == L.ny, mW = i == 1, mE = i == L.nx;
  if (!(mS | mN | mW | mE)) return;
  const int cS = L.EO, cN = jpos32(L, L.ny + 1);
  const long long o = (long long)i * L.plane + ro, oW = ro, oE = (long long)(L.nx + 1) * L.plane + ro;
  if (mS) a[o + cS] = v;
  if (mN) a[o + cN] = v;
  if (mW) { a[oW + c] = v; if (mS) a[oW + cS] = v; if (mN) a[oW + cN] = v; }
  if (mE) { a[oE + c] = v; if (mS) a[oE + cS] = v; if (mN) a[oE + cN] = v; }
}

// positions of column j (= 2 jh + 1 odd, 2 jh + 2 even) and of its j-1, j+1 neighbours inside a row
__device__ __forceinline__ void col_pos(const LevView32 &L, const int jh, const int jodd, int &c, int &jm, int &jp) {
  if (jodd) { c = L.HO + jh; jm = L.EO + jh; }
  else      { c = L.EO + jh + 1; jm = L.HO + jh; }
  jp = jm + 1;
}

// Sum of the off-column couplings of row k of column (c, plane offset o), i.e. (A e)(k) without the own-column terms a1, a2
// (mg_relax.f90:262-301, the same terms as k_residual / relax_col_any).  SNAP: the k = 1 diagonal neighbours (same colour in
// red-black) come from the snapshot p1 taken before the colour; s = the column's snapshot row offset i * RS.
template <bool REAL, bool SNAP>
__device__ __forceinline__ float off32(const LevView32 &L, const float *__restrict__ e, const long long o, const long long s, const int c,
                                       const int jm, const int jp, const int k) {
  const long long RS = L.RS, om = o - L.plane, op = o + L.plane;
  const long long r0 = (long long)(k - 1) * RS, rm = r0 - RS, rp = r0 + RS;
  const float *__restrict__ a3 = L.cA[2], *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4],
              *__restrict__ a6 = L.cA[5], *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7];
  float t = a4[o + r0 + c] * e[o + r0 + jm] + a4[o + r0 + jp] * e[o + r0 + jp] + a7[o + r0 + c] * e[om + r0 + c] + a7[op + r0 + c] * e[op + r0 + c];
  if (k > 1)
    t += a3[o + rm + jp] * e[o + rm + jp] + a5[o + r0 + c] * e[o + rm + jm] + a6[op + rm + c] * e[op + rm + c] + a8[o + r0 + c] * e[om + rm + c];
  if (k < L.nz)
    t += a3[o + r0 + c] * e[o + rp + jm] + a5[o + rp + jp] * e[o + rp + jp] + a6[o + r0 + c] * e[om + rp + c] + a8[op + rp + c] * e[op + rp + c];
  if (REAL && k == 1) {
    const float *__restrict__ q1 = SNAP ? L.p1 : e;
    const long long sm = SNAP ? s - RS : om, sp = SNAP ? s + RS : op;
    t += a5[o + c] * q1[sm + jp] + a5[op + jm] * q1[sp + jm] + a8[o + c] * q1[sm + jm] + a8[op + jp] * q1[sp + jp];
  }
  return t;
}

// residual f - A e of row k
template <bool REAL>
__device__ __forceinline__ float res32(const LevView32 &L, const long long o, const int c, const int jm, const int jp, const int k) {
  const long long RS = L.RS, r0 = (long long)(k - 1) * RS;
  const float *__restrict__ e = L.e, *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1];
  float t = a1[o + r0 + c] * e[o + r0 + c] + off32<REAL, false>(L, e, o, 0, c, jm, jp, k);
  if (k > 1) t += a2[o + r0 + c] * e[o + r0 - RS + c];
  if (k < L.nz) t += a2[o + r0 + RS + c] * e[o + r0 + RS + c];
  return L.f[o + r0 + c] - t;
}

// ------------------------------------------------------------------------------------------------
// z-line smoother, one colour pass (mg_relax.f90:237-334): rhs = f - off-column couplings, then the column's tridiagonal solve
// with the stored pivots bet (gam(k) = a2(k) * bet(k-1), mg_relax.f90:325, formed on the fly).  NZ > 0: the rows of the solve
// live in registers and e is written once; NZ = 0: any nz >= 2, the forward sweep goes through e.  Either way the lane stores the
// physical-boundary images of its column (no halo launch behind the pass).
// ------------------------------------------------------------------------------------------------
template <int NZ, bool REAL, bool SNAP>
__device__ __forceinline__ void relax32_col(const LevView32 &L, const int i, const int jh, const int jodd) {
  int c, jm, jp;
  col_pos(L, jh, jodd, c, jm, jp);
  const long long RS = L.RS, o = (long long)i * L.plane, s = (long long)i * RS;
  const int nz = NZ > 0 ? NZ : L.nz;
  float *__restrict__ e = L.e;
  const float *__restrict__ f = L.f, *__restrict__ a2 = L.cA[1], *__restrict__ bet = L.bet;
  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
  if (NZ > 0) {
    float x[NZ > 0 ? NZ : 1], g[NZ > 0 ? NZ : 1];
    float xv = 0.f, betp = 0.f;
#pragma unroll
    for (int k = 1; k <= NZ; k++) {
      const long long ko = o + (long long)(k - 1) * RS + c;
      const float rhs = f[ko] - off32<REAL, SNAP>(L, e, o, s, c, jm, jp, k);
      const float bk = bet[ko];
      if (k == 1) xv = rhs * bk;
      else { const float a = a2[ko]; g[k - 1] = a * betp; xv = (rhs - a * xv) * bk; }
      betp = bk;
      x[k - 1] = xv;
    }
#pragma unroll
    for (int k = NZ - 1; k >= 1; k--) x[k - 1] = x[k - 1] - g[k] * x[k];
#pragma unroll
    for (int k = 1; k <= NZ; k++) {
      const long long ro = (long long)(k - 1) * RS;
      e[o + ro + c] = x[k - 1];
      mirror32(L, e, ro, j, i, c, x[k - 1]);
    }
  } else {
    float xv = 0.f;
    for (int k = 1; k <= nz; k++) {
      const long long ko = o + (long long)(k - 1) * RS + c;
      const float rhs = f[ko] - off32<REAL, SNAP>(L, e, o, s, c, jm, jp, k);
      xv = k == 1 ? rhs * bet[ko] : (rhs - a2[ko] * xv) * bet[ko];
      e[ko] = xv;
    }
    mirror32(L, e, (long long)(nz - 1) * RS, j, i, c, xv);
    for (int k = nz - 1; k >= 1; k--) {
      const long long ro = (long long)(k - 1) * RS, ko = o + ro + c;
      xv = e[ko] - a2[ko + RS] * bet[ko] * xv;
      e[ko] = xv;
      mirror32(L, e, ro, j, i, c, xv);
    }
  }
}

template <int NZ, bool REAL, bool SNAP>
__global__ __launch_bounds__(256) void k_relax32(LevView32 L, int i0, int istep, int nplanes, int jodd_fixed, int rb) {
  const int jh = blockIdx.x * WAVE + threadIdx.x;
  const int ipl = blockIdx.y * blockDim.y + threadIdx.y;
  if (jh >= (L.ny >> 1) || ipl >= nplanes) return;
  const int i = i0 + istep * ipl;
  // RB: j = 1+mod(i+rb,2),ny,2 (mg_relax.f90:174) ; FC: fixed parity (:216-217)
  const int jodd = jodd_fixed >= 0 ? jodd_fixed : (((i + rb) & 1) == 0);
  relax32_col<NZ, REAL, SNAP>(L, i, jh, jodd);
}

// ------------------------------------------------------------------------------------------------
// The same colour pass, software-pipelined (option "mixed_ring"; the levels choose_relax32 gives it: mgx_choice.h).  relax32_col asks for
// every coupling and neighbour value of a row where it uses it -- nothing is in flight while a row waits, and each neighbour row is read for
// the rows k-1, k and k+1.  Here, as in the fp64 stored-coefficient pass (SC_PROLOGUE / SC_ROW, mgx_relax_common.h): the k loop is fully
// unrolled; the raw rows of the own column (f, a2 .. a8, bet: 9 loads) and of the neighbours (e at j-1, i-1, j+1, i+1; a3 .. a5 at j+1,
// a6 .. a8 at i+1: 10 loads) are requested D rows ahead into register rings of D + 1 rows; a neighbour row is loaded once, its six
// products formed once and kept in a three-row window; x(k) and gam(k) stay in registers (2 NZ of them: no LDS), the back substitution
// issues no load, and e is stored once, the physical-boundary images with it.  The operator of relax32_col term for term, summed in
// another order: not its bits (-ffp-contract=fast), the same bound against the fp64 pass.  NT: the level does not fit the Infinity Cache
// between passes -- what the pass reads exactly once (the own rows) and what it writes carry the non-temporal hint.
// ------------------------------------------------------------------------------------------------
template <bool NT> __device__ __forceinline__ float ld32(const float *p) { return NT ? __builtin_nontemporal_load(p) : *p; }

template <int NZ, int D, bool REAL, bool SNAP, bool NT>
__device__ __forceinline__ void relax32r_col(const LevView32 &L, const int i, const int jh, const int jodd) {
  int c, jm, jp;
  col_pos(L, jh, jodd, c, jm, jp);
  const long long RS = L.RS, o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;
  float *__restrict__ e = L.e;
  const float *__restrict__ f = L.f, *__restrict__ a2 = L.cA[1], *__restrict__ a3 = L.cA[2], *__restrict__ a4 = L.cA[3],
              *__restrict__ a5 = L.cA[4], *__restrict__ a6 = L.cA[5], *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7],
              *__restrict__ bet = L.bet;
  constexpr int R = D + 1;   // rows of a ring: row q waits in slot q % R, which row q - R left when it was used
  float n_jm[R], n_im[R], n_jp[R], n_ip[R], n_a3[R], n_a4[R], n_a5[R], n_a6[R], n_a7[R], n_a8[R];
  float w_f[R], w_a2[R], w_a3[R], w_a4[R], w_a5[R], w_a6[R], w_a7[R], w_a8[R], w_bet[R];
  float x[NZ], g[NZ];
#define R32_NB_LOAD(q)                                                                                                     \
  if ((q) <= NZ) {                                                                                                         \
    const long long ro_ = (long long)((q)-1) * RS; const int s_ = (q) % R;                                                 \
    n_jm[s_] = e[o + ro_ + jm]; n_im[s_] = e[om + ro_ + c]; n_jp[s_] = e[o + ro_ + jp]; n_ip[s_] = e[op + ro_ + c];        \
    n_a3[s_] = a3[o + ro_ + jp]; n_a4[s_] = a4[o + ro_ + jp]; n_a5[s_] = a5[o + ro_ + jp];                                 \
    n_a6[s_] = a6[op + ro_ + c]; n_a7[s_] = a7[op + ro_ + c]; n_a8[s_] = a8[op + ro_ + c];                                 \
  }
#define R32_OW_LOAD(q)                                                                                                     \
  if ((q) <= NZ) {                                                                                                         \
    const long long ko_ = o + (long long)((q)-1) * RS + c; const int s_ = (q) % R;                                         \
    w_f[s_] = ld32<NT>(f + ko_); w_a2[s_] = ld32<NT>(a2 + ko_); w_a3[s_] = ld32<NT>(a3 + ko_); w_a4[s_] = ld32<NT>(a4 + ko_); \
    w_a5[s_] = ld32<NT>(a5 + ko_); w_a6[s_] = ld32<NT>(a6 + ko_); w_a7[s_] = ld32<NT>(a7 + ko_); w_a8[s_] = ld32<NT>(a8 + ko_); \
    w_bet[s_] = ld32<NT>(bet + ko_);                                                                                       \
  }
// the products of a raw neighbour row, formed when the row enters the window
#define R32_NB_USE(q, EJM, EIM, M3, M4, M5, N6, N7, N8)                                                                    \
  { const int s_ = (q) % R; EJM = n_jm[s_]; EIM = n_im[s_];                                                                \
    M3 = n_a3[s_] * n_jp[s_]; M4 = n_a4[s_] * n_jp[s_]; M5 = n_a5[s_] * n_jp[s_];                                          \
    N6 = n_a6[s_] * n_ip[s_]; N7 = n_a7[s_] * n_ip[s_]; N8 = n_a8[s_] * n_ip[s_]; }
  // the k = 1 diagonals (requested first: they depend on nothing); red-black reads the values from the snapshot
  float d1 = 0.f, d2 = 0.f, d3 = 0.f, d4 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f;
  if (REAL) {
    const float *__restrict__ q1 = SNAP ? L.p1 : e;
    const long long s = (long long)i * RS, sm = SNAP ? s - RS : om, sp = SNAP ? s + RS : op;
    d1 = q1[sm + jp]; d2 = q1[sp + jm]; d3 = q1[sm + jm]; d4 = q1[sp + jp];
    c1 = a5[o + c]; c2 = a5[op + jm]; c3 = a8[o + c]; c4 = a8[op + jp];
  }
  // neighbour rows 1 .. 1 + D and own rows 1 .. D
#pragma unroll
  for (int q = 1; q <= 1 + D; q++) { R32_NB_LOAD(q) }
#pragma unroll
  for (int q = 1; q <= D; q++) { R32_OW_LOAD(q) }
  // the window: e at j-1 and i-1 of the rows k-1, k, k+1 (_m, _0, _p) and the products a3 e .. a8 e of the j+1 and i+1 neighbours
  float ejm_m = 0.f, ejm_0, ejm_p = 0.f, eim_m = 0.f, eim_0, eim_p = 0.f;
  float m3_m = 0.f, m3_0, m3_p = 0.f, m4_0, m4_p = 0.f, m5_p = 0.f, n6_m = 0.f, n6_0, n6_p = 0.f, n7_0, n7_p = 0.f, n8_p = 0.f;
  R32_NB_USE(1, ejm_0, eim_0, m3_0, m4_0, m5_p, n6_0, n7_0, n8_p)
  float xv = 0.f, betp = 0.f;
#pragma unroll
  for (int k = 1; k <= NZ; k++) {
    R32_NB_LOAD(k + 1 + D)
    R32_OW_LOAD(k + D)
    if (k < NZ) { R32_NB_USE(k + 1, ejm_p, eim_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p) }
    const int s = k % R;
    // the twelve off-column products of off32, the neighbours' from the window
    float t = w_a4[s] * ejm_0 + m4_0 + w_a7[s] * eim_0 + n7_0;
    if (k > 1) t += m3_m + w_a5[s] * ejm_m + n6_m + w_a8[s] * eim_m;
    if (k < NZ) t += w_a3[s] * ejm_p + m5_p + w_a6[s] * eim_p + n8_p;
    if (REAL && k == 1) t += c1 * d1 + c2 * d2 + c3 * d3 + c4 * d4;
    const float rhs = w_f[s] - t, bk = w_bet[s];
    if (k == 1) xv = rhs * bk;
    else { const float a = w_a2[s]; g[k - 1] = a * betp; xv = (rhs - a * xv) * bk; }
    betp = bk;
    x[k - 1] = xv;
    ejm_m = ejm_0; ejm_0 = ejm_p; eim_m = eim_0; eim_0 = eim_p;
    m3_m = m3_0; m3_0 = m3_p; m4_0 = m4_p; n6_m = n6_0; n6_0 = n6_p; n7_0 = n7_p;
  }
#undef R32_NB_LOAD
#undef R32_OW_LOAD
#undef R32_NB_USE
#pragma unroll
  for (int k = NZ - 1; k >= 1; k--) x[k - 1] = x[k - 1] - g[k] * x[k];
  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
#pragma unroll
  for (int k = 1; k <= NZ; k++) {
    const long long ro = (long long)(k - 1) * RS;
    if (NT) __builtin_nontemporal_store(x[k - 1], e + o + ro + c); else e[o + ro + c] = x[k - 1];
    mirror32(L, e, ro, j, i, c, x[k - 1]);
  }
}

// one wave per 64 columns of a plane, blockDim.y planes per workgroup, blocks dealt to the XCDs in runs of planes (XCD_BLOCK_MAP)
template <int NZ, int D, bool REAL, bool SNAP, bool NT>
__global__ __launch_bounds__(128, 1) void k_relax32r(LevView32 L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int gx) {
  const int npair = (nplanes + blockDim.y - 1) / blockDim.y;
  int bx, ipr;
  XCD_BLOCK_MAP(npair, gx, bx, ipr)
  const int ipl = ipr * blockDim.y + threadIdx.y;
  const int jh = bx * WAVE + threadIdx.x;
  if (jh >= (L.ny >> 1) || ipl >= nplanes) return;
  const int i = i0 + istep * ipl;
  const int jodd = jodd_fixed >= 0 ? jodd_fixed : (((i + rb) & 1) == 0);
  relax32r_col<NZ, D, REAL, SNAP, NT>(L, i, jh, jodd);
}

// snapshot of e(k=1,:,:), halo included, for the red-black pass
__global__ void k_snapshot32(LevView32 L) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (t < L.RS) L.p1[(long long)i * L.RS + t] = L.e[(long long)i * L.plane + t];
}

// r = f - A e with the physical images of r (mgx_mixed_op "residual"; the cycle never writes r).  blockIdx.z = j parity.
template <bool REAL>
__global__ __launch_bounds__(256) void k_residual32(LevView32 L) {
  const int jh = blockIdx.x * WAVE + threadIdx.x;
  const int i = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (jh >= (L.ny >> 1) || i > L.nx) return;
  const int jodd = blockIdx.z == 0;
  int c, jm, jp;
  col_pos(L, jh, jodd, c, jm, jp);
  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
  const long long o = (long long)i * L.plane;
  for (int k = 1; k <= L.nz; k++) {
    const long long ro = (long long)(k - 1) * L.RS;
    const float v = res32<REAL>(L, o, c, jm, jp, k);
    L.r[o + ro + c] = v;
    mirror32(L, L.r, ro, j, i, c, v);
  }
}

// ------------------------------------------------------------------------------------------------
// Down leg of a V-cycle: compute_residual(lev) + fine2coarse(lev) in one pass, f_c = sum of the 8 fine residuals
// (mg_intergrids.f90:139-162), e_c = 0; no r written, no norm.  One lane = one coarse column = 2 x 2 fine columns.
// ------------------------------------------------------------------------------------------------
template <bool REAL>
__device__ __forceinline__ void resrest32_col(const LevView32 &F, const LevView32 &C, const int j2, const int i2) {
  const int i = 2 * i2 - 1, jh = j2 - 1;
  int co, jmo, jpo, ce, jme, jpe;
  col_pos(F, jh, 1, co, jmo, jpo);   // fine j = 2 j2 - 1
  col_pos(F, jh, 0, ce, jme, jpe);   // fine j = 2 j2
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  const int cc = jpos32(C, j2);
  const long long oc = (long long)i2 * C.plane + cc;
  for (int k2 = 1; k2 <= C.nz; k2++) {
    float z = 0.f;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = 2 * k2 - 1 + h;
      z += res32<REAL>(F, o0, co, jmo, jpo, k) + res32<REAL>(F, o1, co, jmo, jpo, k) + res32<REAL>(F, o0, ce, jme, jpe, k) + res32<REAL>(F, o1, ce, jme, jpe, k);
    }
    const long long ro = (long long)(k2 - 1) * C.RS;
    C.f[oc + ro] = z; mirror32(C, C.f, ro, j2, i2, cc, z);
    C.e[oc + ro] = 0.f; mirror32(C, C.e, ro, j2, i2, cc, 0.f);
  }
}
template <bool REAL>
__global__ __launch_bounds__(256) void k_resrest32(LevView32 F, LevView32 C) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int i2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (j2 > C.ny || i2 > C.nx) return;
  resrest32_col<REAL>(F, C, j2, i2);
}

// First leg of the F-cycle (mg_solvers.f90:110-115): f_c = sum of the 8 fine values of `src` (the fine f, which is the fine residual
// there because the fine e is 0), e_c = 0.  mg_intergrids.f90:139-162.
__device__ __forceinline__ void restrict32_col(const LevView32 &F, const LevView32 &C, const float *x, const int j2, const int i2) {
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j = 2*j2-1 (odd) and 2*j2 (even)
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  const int cc = jpos32(C, j2);
  const long long oc = (long long)i2 * C.plane + cc;
  for (int k2 = 1; k2 <= C.nz; k2++) {
    const long long r0 = (long long)(2 * k2 - 2) * F.RS, r1 = r0 + F.RS;
    const float z = x[o0 + r0 + po] + x[o1 + r0 + po] + x[o0 + r0 + pe] + x[o1 + r0 + pe] + x[o0 + r1 + po] + x[o1 + r1 + po] + x[o0 + r1 + pe] + x[o1 + r1 + pe];
    const long long ro = (long long)(k2 - 1) * C.RS;
    C.f[oc + ro] = z; mirror32(C, C.f, ro, j2, i2, cc, z);
    C.e[oc + ro] = 0.f; mirror32(C, C.e, ro, j2, i2, cc, 0.f);
  }
}
__global__ __launch_bounds__(256) void k_restrict32(LevView32 F, LevView32 C, const float *__restrict__ x) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int i2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (j2 > C.ny || i2 > C.nx) return;
  restrict32_col(F, C, x, j2, i2);
}

// ------------------------------------------------------------------------------------------------
// coarse2fine: fine e += interp(coarse e), mg_intergrids.f90:366-450 (tri-linear, top level x 1/2), :336-363 (nearest), :226.
// The expressions of k_coarse2fine_run and k_coarse2fine_nearest (mgx_transfer.hip); the interpolated correction is not stored in r.
// ------------------------------------------------------------------------------------------------
template <bool LINEAR>
__device__ __forceinline__ void coarse2fine32_cell(const LevView32 &F, const LevView32 &C, const int j2, const int k2, const int i2) {
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;
  const int c0 = jpos32(C, j2), cm = jpos32(C, j2 - 1), cp = jpos32(C, j2 + 1);
  const long long q0 = (long long)i2 * C.plane, qm = q0 - C.plane, qp = q0 + C.plane;
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  const float *__restrict__ xc = C.e;
  float *__restrict__ pf = F.e;
  const int nz = C.nz;
#define XC(kk, JJ, QQ) xc[QQ + (long long)((kk)-1) * C.RS + JJ]
#define PUT(k, OO, PP, val) { const long long ro_ = (long long)((k)-1) * F.RS, t_ = OO + ro_ + PP; const float w_ = pf[t_] + (val); pf[t_] = w_; \
    mirror32(F, pf, ro_, (PP == po) ? 2 * j2 - 1 : 2 * j2, (OO == o0) ? i : i + 1, PP, w_); }
  if (!LINEAR) {
    const float v = XC(k2, c0, q0);
    const int k = 2 * k2 - 1;
    PUT(k, o0, po, v); PUT(k + 1, o0, po, v); PUT(k, o0, pe, v); PUT(k + 1, o0, pe, v);
    PUT(k, o1, po, v); PUT(k + 1, o1, po, v); PUT(k, o1, pe, v); PUT(k + 1, o1, pe, v);
    return;
  }
  const float a = 9.f / 16.f, b = 3.f / 16.f, c = 1.f / 16.f, d = 27.f / 64.f, e = 9.f / 64.f, f = 3.f / 64.f, g = 1.f / 64.f;
  const float x00 = XC(k2, c0, q0), xmm = XC(k2, cm, qm), xm0 = XC(k2, cm, q0), x0m = XC(k2, c0, qm),
              xpm = XC(k2, cp, qm), xp0 = XC(k2, cp, q0), xmp = XC(k2, cm, qp), x0p = XC(k2, c0, qp), xpp = XC(k2, cp, qp);
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const int k = 2 * k2 - 1 + half;
    if (k == 1) {
      PUT(1, o0, po, a * x00 + c * xmm + b * xm0 + b * x0m);
      PUT(1, o0, pe, a * x00 + c * xpm + b * xp0 + b * x0m);
      PUT(1, o1, po, a * x00 + c * xmp + b * xm0 + b * x0p);
      PUT(1, o1, pe, a * x00 + c * xpp + b * xp0 + b * x0p);
    } else if (k == 2 * nz) {
      PUT(k, o0, po, 0.5f * (a * x00 + c * xmm + b * xm0 + b * x0m));
      PUT(k, o0, pe, 0.5f * (a * x00 + c * xpm + b * xp0 + b * x0m));
      PUT(k, o1, po, 0.5f * (a * x00 + c * xmp + b * xm0 + b * x0p));
      PUT(k, o1, pe, 0.5f * (a * x00 + c * xpp + b * xp0 + b * x0p));
    } else {
      const int kp = k2 - ((k % 2) * 2 - 1);
      const float y00 = XC(kp, c0, q0), ymm = XC(kp, cm, qm), ym0 = XC(kp, cm, q0), y0m = XC(kp, c0, qm),
                  ypm = XC(kp, cp, qm), yp0 = XC(kp, cp, q0), ymp = XC(kp, cm, qp), y0p = XC(kp, c0, qp), ypp = XC(kp, cp, qp);
      PUT(k, o0, po, d * x00 + f * xmm + e * xm0 + e * x0m + e * y00 + g * ymm + f * ym0 + f * y0m);
      PUT(k, o0, pe, d * x00 + f * xpm + e * xp0 + e * x0m + e * y00 + g * ypm + f * yp0 + f * y0m);
      PUT(k, o1, po, d * x00 + f * xmp + e * xm0 + e * x0p + e * y00 + g * ymp + f * ym0 + f * y0p);
      PUT(k, o1, pe, d * x00 + f * xpp + e * xp0 + e * x0p + e * y00 + g * ypp + f * yp0 + f * y0p);
    }
  }
#undef XC
#undef PUT
}
template <bool LINEAR>
__global__ __launch_bounds__(256) void k_coarse2fine32(LevView32 F, LevView32 C) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int k2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  const int i2 = 1 + blockIdx.z;
  if (j2 > C.ny || k2 > C.nz) return;
  coarse2fine32_cell<LINEAR>(F, C, j2, k2, i2);
}

// ------------------------------------------------------------------------------------------------
// The coarsest solve of a cycle as ONE matrix-vector product (option "mixed_direct"): the level is entered with e = 0 and left after
// ns_coarsest sweeps, a fixed linear map e = B f of its right-hand side (mgx_relax_coarse.hip has the fp64 form and the builder).  M is
// that operator rounded once to fp32, column by column: M[c * n + r], the cells numbered r = (k - 1) + nz * ((j - 1) + ny * (i - 1)).
// direct32_rows is the whole product on the tiles t0 .. t1 - 1 of 64 rows, by the waves of one workgroup: f is staged in LDS; an item is
// one tile of rows times one slab of columns (ch_direct32_slabs, mgx_choice.h), lanes along r (coalesced), the columns of the slab walked
// in ascending order by one chain of fmaf; the S partial sums of a row meet in LDS and are added in ascending order of the slab.  So the
// order in which the terms of a row are added is a function of n alone -- not of the lane count, the launch or which wave ran an item:
// the stand-alone launch and the phase of the tail kernel give the same bits (explicit fmaf / __fadd_rn: nothing for -ffp-contract to
// decide).  Whole rows belong to one workgroup: no atomics, no tickets.  Lanes past n neither load nor store.  Two barriers inside;
// the caller's follows the stores of e and of its physical-boundary images.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long cell_js32(const LevView32 &L, const int r, int &k0, int &j, int &i) {
  k0 = r % L.nz; const int q = r / L.nz; j = 1 + q % L.ny; i = 1 + q / L.ny;
  return (long long)i * L.plane + (long long)k0 * L.RS + jpos32(L, j);
}
__device__ __forceinline__ void direct32_rows(const LevView32 &L, const float *__restrict__ M, const int n, float *fs, float *part, const int t0, const int t1) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nwaves = nt / WAVE;
  const int S = ch_direct32_slabs(n), cps = (n + S - 1) / S, npad = ch_direct32_tiles(n) * WAVE;
  for (int c = tid; c < n; c += nt) { int k0, j, i; fs[c] = L.f[cell_js32(L, c, k0, j, i)]; }
  __syncthreads();
  for (int q = wave; q < (t1 - t0) * S; q += nwaves) {
    const int t = t0 + q / S, s = q - (q / S) * S, r = t * WAVE + lane;
    const int c0 = s * cps, c1 = c0 + cps < n ? c0 + cps : n;
    if (r < n) {
      const float *__restrict__ m = M + (long long)c0 * n + r;
      float acc = 0.f;
#pragma unroll 8
      for (int c = c0; c < c1; c++, m += n) acc = __fmaf_rn(*m, fs[c], acc);
      part[s * npad + r] = acc;
    }
  }
  __syncthreads();
  const int r1 = t1 * WAVE < n ? t1 * WAVE : n;
  for (int r = t0 * WAVE + tid; r < r1; r += nt) {
    float v = part[r];
    for (int s = 1; s < S; s++) v = __fadd_rn(v, part[s * npad + r]);
    int k0, j, i;
    const long long o = cell_js32(L, r, k0, j, i);
    L.e[o] = v;
    mirror32(L, L.e, (long long)k0 * L.RS, j, i, jpos32(L, j), v);
  }
}
// one workgroup per tile of 64 rows, one wave per slab (choose_coarse_direct32)
__global__ __launch_bounds__(WAVE * DIRECT32_MAX_SLABS) void k_coarse_direct32(LevView32 L, const float *__restrict__ M, int n) {
  __shared__ float fs[DIRECT32_MAX_N], part[DIRECT32_PART];
  direct32_rows(L, M, n, fs, part, blockIdx.x, blockIdx.x + 1);
}
// B32 = the fp64 operator rounded once, same storage
__global__ void k_direct32_round(const double *__restrict__ M64, float *__restrict__ M, long long nn) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nn) M[t] = (float)M64[t];
}

// ------------------------------------------------------------------------------------------------
// The tail of a cycle in ONE workgroup (option "mixed_tail"): the coarsest levels that are all small (mixed_tail_small, mgx_internal.h)
// cost a per-launch cycle its launch latency and nothing else (16x16x2: 960 launches per F-cycle), so here the schedule of relax32 /
// vcycle32 / fcycle32 (mgx_cycle.cpp) on those levels runs inside one launch of up to 768 lanes.  Lane 0 writes the schedule as a list of
// phases into LDS (tail_program); every phase is a workgroup-strided loop over the work items the per-launch kernel of the same name gives a
// lane, calls that kernel's device function, and ends with __syncthreads() -- the only synchronisation there is: one workgroup, no flags, no
// atomics, nothing to wait for.  No lane leaves a phase early, so every lane reaches every barrier.  e, f and p1 change from phase to phase
// and are read through the plain pointers of the by-value LevView32 (nothing marks them invariant); a column's mirror images are stored by
// the lane that owns the column, before the barrier.
// ------------------------------------------------------------------------------------------------
// levels one launch takes.  A tail has no more: its coarsest level has at least 4 x 4 x 2 cells and every finer one 8 times as many (more where
// an odd nz was halved), so the fifth from the bottom is past MIXED_TAIL_MAX_CELLS = 32768.
#define MIXED_TAIL_MAX_LEVELS 4
// Two register classes, both without scratch: a tail whose levels take the instances relax32_col<2>, <4>, <8> or the generic pass needs 164
// registers (the residual + restriction's loads in flight) and runs with up to 768 lanes (3 waves per SIMD, 170 registers each); one with an
// nz = 16 or 32 level needs 251-256 (relax32_col<32>: 239 in its own kernel), and runs with up to 256 lanes (1 wave per SIMD, 512 registers).
#define MIXED_TAIL_LANES_A 768
#define MIXED_TAIL_LANES_B 256
// a phase: kind | level (index into Tail32::L) << 2 | which sweep count << 5
enum { TP_RELAX = 0, TP_RESREST = 1, TP_RESTRICT = 2, TP_C2F = 3 };
enum { TN_CALL = 0, TN_PRE = 1, TN_POST = 2, TN_COARSEST = 3, TN_DIRECT = 4 };   // TN_DIRECT: not sweeps, the product of option "mixed_direct"
#define TAIL_OP(kind, lev, nsel) (unsigned char)((kind) | (lev) << 2 | (nsel) << 5)
// the F-cycle of nl levels: nl restrictions and coarsest relax, then V-cycles of 2 + 4 d phases from d = 1 .. nl - 1 levels above the coarsest
#define MIXED_TAIL_MAX_OPS (MIXED_TAIL_MAX_LEVELS + 2 * (MIXED_TAIL_MAX_LEVELS - 1) * (MIXED_TAIL_MAX_LEVELS + 1))
struct Tail32 {
  LevView32 L[MIXED_TAIL_MAX_LEVELS];   // the tail's levels, finest first
  int nl, mode, lead;                   // mode: TAIL_* of mgx_wrappers.h; lead: the V-cycle starts with coarse2fine onto L[0]
  int n, ns_pre, ns_post, ns_coarsest, linear;
  // the NZ instance of each level's colour pass, as mgxx_relax_pass picks it (0 = the generic pass).  Apart from L[].nz on purpose: inside
  // `case 8:` of a switch over L.nz the compiler knows L.nz, folds the `k < L.nz` of off32 / res32 that the per-launch kernels test at run
  // time, and -ffp-contract=fast then fuses across what were block boundaries: other roundings than theirs.
  int inst[MIXED_TAIL_MAX_LEVELS];
  // option "mixed_direct": the coarsest solve of a cycle is the product with dM (dn rows) instead of ns_coarsest sweeps; nullptr = the sweeps
  const float *dM; int dn;
};

// vcycle32(a, lead) on levels a .. nl-1 (indices into Tail32::L)
__device__ __forceinline__ int tail_vcycle(unsigned char *p, int q, const int a, const int nl, const bool lead, const int coarsest) {
  for (int l = a; l < nl - 1; l++) {
    if (lead && l == a) p[q++] = TAIL_OP(TP_C2F, l, 0);
    p[q++] = TAIL_OP(TP_RELAX, l, TN_PRE);
    p[q++] = TAIL_OP(TP_RESREST, l, 0);
  }
  p[q++] = TAIL_OP(TP_RELAX, nl - 1, coarsest);
  for (int l = nl - 2; l >= a; l--) {
    p[q++] = TAIL_OP(TP_C2F, l, 0);
    p[q++] = TAIL_OP(TP_RELAX, l, TN_POST);
  }
  return q;
}
// coarsest: TN_COARSEST, or TN_DIRECT in the instances that have the phase (the host hands them a cycle whose coarsest level was just restricted onto)
__device__ __forceinline__ int tail_program(const Tail32 &T, unsigned char *p, const int coarsest) {
  if (T.mode == TAIL_RELAX) { p[0] = TAIL_OP(TP_RELAX, 0, TN_CALL); return 1; }
  if (T.mode == TAIL_VCYCLE) return tail_vcycle(p, 0, 0, T.nl, T.lead != 0, coarsest);
  int q = 0;   // TAIL_FCYCLE: fcycle32 with L[0] as its finest level
  for (int l = 0; l < T.nl - 1; l++) p[q++] = TAIL_OP(TP_RESTRICT, l, 0);
  p[q++] = TAIL_OP(TP_RELAX, T.nl - 1, coarsest);
  for (int l = T.nl - 2; l >= 0; l--) q = tail_vcycle(p, q, l, T.nl, true, coarsest);
  return q;
}

// relax32(lev, nsweeps): the colour passes of k_relax32 (and k_snapshot32 before each red-black colour of cmatrix='real')
template <int NZ, bool REAL, bool RB>
__device__ __forceinline__ void tail_relax(const LevView32 &L, const int nsweeps) {
  const int nh = L.ny >> 1, nt = blockDim.x, tid = threadIdx.x;
  for (int it = 0; it < nsweeps; it++) {
    if (RB) {
#pragma nounroll
      for (int rb = 1; rb <= 2; rb++) {
        if (REAL) {
          const int RS = L.RS, n = (L.nx + 2) * RS;
          for (int t = tid; t < n; t += nt) { const int i = t / RS; L.p1[t] = L.e[(long long)i * L.plane + (t - i * RS)]; }
          __syncthreads();
        }
        const int n = nh * L.nx;
        for (int t = tid; t < n; t += nt) {
          const int ipl = t / nh, jh = t - ipl * nh, i = 1 + ipl;
          relax32_col<NZ, REAL, REAL>(L, i, jh, ((i + rb) & 1) == 0);
        }
        __syncthreads();
      }
    } else {
#pragma nounroll
      for (int fc = 0; fc < 4; fc++) {   // (fc1, fc2) = (1,1), (1,2), (2,1), (2,2)
        const int i0 = 1 + (fc >> 1), jodd = (fc & 1) == 0, n = nh * (L.nx >> 1);
        for (int t = tid; t < n; t += nt) {
          const int ipl = t / nh, jh = t - ipl * nh;
          relax32_col<NZ, REAL, false>(L, i0 + 2 * ipl, jh, jodd);
        }
        __syncthreads();
      }
    }
  }
}

// The row count of the direct phase reaches it through LDS, read inside the phase: taken from the kernel's argument, everything the phase
// derives from it (slabs, columns per slab, the lanes' tiles) is loop-invariant, hoisted out of the phase loop and kept alive across the colour
// passes -- 3 registers too many for the 768-lane class (16 bytes of scratch in its red-black instances).
__device__ __forceinline__ int *tail_direct_n() { __shared__ int n; return &n; }
// NZMAX: the largest register instance of the colour pass compiled in (a level with a larger one goes to the other class: launch_tail)
// DIRECT: the instance has the phase of option "mixed_direct" (direct32_rows on every tile of the coarsest level) and emits it for the coarsest
// solve of its cycles; without it the kernel is the text it was before the option existed
template <bool REAL, bool RB, int NZMAX, int LANES, bool DIRECT>
__global__ __launch_bounds__(LANES) void k_tail32(const Tail32 T) {
  __shared__ unsigned char prog[MIXED_TAIL_MAX_OPS];
  __shared__ int nprog;
  if (threadIdx.x == 0) nprog = tail_program(T, prog, DIRECT ? TN_DIRECT : TN_COARSEST);
  if constexpr (DIRECT) { if (threadIdx.x == 0) *tail_direct_n() = T.dn; }
  __syncthreads();
  const int np = __builtin_amdgcn_readfirstlane(nprog), nt = blockDim.x, tid = threadIdx.x;
  for (int pc = 0; pc < np; pc++) {
    const int op = __builtin_amdgcn_readfirstlane((int)prog[pc]), kind = op & 3, l = (op >> 2) & 7, nsel = op >> 5;
    const LevView32 &L = T.L[l];
    if (kind == TP_RELAX) {
      if constexpr (DIRECT) {
        if (nsel == TN_DIRECT) {
          __shared__ float dfs[DIRECT32_MAX_N], dpart[DIRECT32_PART];
          const int dn = __builtin_amdgcn_readfirstlane(*tail_direct_n());
          direct32_rows(L, T.dM, dn, dfs, dpart, 0, ch_direct32_tiles(dn));
          __syncthreads();
          continue;
        }
      }
      const int ns = nsel == TN_CALL ? T.n : (nsel == TN_PRE ? T.ns_pre : (nsel == TN_POST ? T.ns_post : T.ns_coarsest));
      switch (T.inst[l]) {   // the instance mgxx_relax_pass picks
        case 2: tail_relax<2, REAL, RB>(L, ns); break;
        case 4: tail_relax<4, REAL, RB>(L, ns); break;
        case 8: tail_relax<8, REAL, RB>(L, ns); break;
        case 16: if constexpr (NZMAX >= 16) { tail_relax<16, REAL, RB>(L, ns); } break;
        case 32: if constexpr (NZMAX >= 32) { tail_relax<32, REAL, RB>(L, ns); } break;
        default: tail_relax<0, REAL, RB>(L, ns); break;
      }
      continue;   // (every colour pass has ended with its barrier)
    }
    const LevView32 &C = T.L[l + 1];
    if (kind == TP_C2F) {
      const int n = C.ny * C.nz * C.nx;
      for (int t = tid; t < n; t += nt) {
        const int q = t / C.ny, j2 = 1 + (t - q * C.ny), i2 = 1 + q / C.nz, k2 = 1 + (q - (i2 - 1) * C.nz);
        if (T.linear) coarse2fine32_cell<true>(L, C, j2, k2, i2); else coarse2fine32_cell<false>(L, C, j2, k2, i2);
      }
    } else {
      const int n = C.ny * C.nx;
      for (int t = tid; t < n; t += nt) {
        const int q = t / C.ny, j2 = 1 + (t - q * C.ny), i2 = 1 + q;
        if (kind == TP_RESREST) resrest32_col<REAL>(L, C, j2, i2); else restrict32_col(L, C, L.f, j2, i2);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// fp64 <-> fp32 over a whole JS array, halo included (the two layouts differ in EO / HO / RS).  One lane = one half-row position
// h = 0..ny/2 of parity blockIdx.z (j = 2h+1 odd, 2h even) in plane i, walking up k.
//   to32: dst = (float)(scale * src)                    (coefficients, pivots, the demoted residual, mgx_mixed_op inputs)
//   to64: dst = (add ? dst : 0) + (double)src * scale    (p += e / s after the cycle, mgx_mixed_op results)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_to32(LevView D, LevView32 S, const double *__restrict__ src, float *__restrict__ dst, double scale) {
  const int h = blockIdx.x * WAVE + threadIdx.x;
  const int i = blockIdx.y * blockDim.y + threadIdx.y;
  if (h > (D.ny >> 1) || i > D.nx + 1) return;
  const int j = blockIdx.z ? 2 * h : 2 * h + 1;
  const long long od = (long long)i * D.plane + jpos(D, j), os = (long long)i * S.plane + jpos32(S, j);
  for (int k = 0; k < D.nz; k++) dst[os + (long long)k * S.RS] = (float)(scale * src[od + (long long)k * D.RS]);
}
__global__ __launch_bounds__(256) void k_to64(LevView D, LevView32 S, const float *__restrict__ src, double *__restrict__ dst, double scale, int add) {
  const int h = blockIdx.x * WAVE + threadIdx.x;
  const int i = blockIdx.y * blockDim.y + threadIdx.y;
  if (h > (D.ny >> 1) || i > D.nx + 1) return;
  const int j = blockIdx.z ? 2 * h : 2 * h + 1;
  const long long od = (long long)i * D.plane + jpos(D, j), os = (long long)i * S.plane + jpos32(S, j);
  for (int k = 0; k < D.nz; k++) {
    const double v = (double)src[os + (long long)k * S.RS] * scale;
    dst[od + (long long)k * D.RS] = add ? dst[od + (long long)k * D.RS] + v : v;
  }
}

// the instance a Choice of choose_relax32 names (mgx_choice.h), launched
static void launch_relax32(hipStream_t st, const LevView32 *L, const Choice &c, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap) {
  const dim3 blk(c.bx, c.by), grd(c.grid, c.gy);
  if (c.family == KF_RELAX32R) {
    with_nz<RING_NZ_LIST>(c.nz, [&](auto nz) {
      with_real_and(real, snap, [&](auto re, auto sn) {
        with_bool(c.stream, [&](auto nt) {
          constexpr int NZ = decltype(nz)::value;
          hipLaunchKernelGGL((k_relax32r<NZ, ch_ring_depth(NZ), decltype(re)::value, decltype(sn)::value, decltype(nt)::value>), grd, blk, 0, st, *L, i0,
                             istep, nplanes, jodd_fixed, rb, c.gx);
        });
      });
    });
    return;
  }
  with_real_and(real, snap, [&](auto re, auto sn) {
    constexpr bool RE = decltype(re)::value, SN = decltype(sn)::value;
    if (!with_nz<RELAX32_NZ_LIST>(c.nz, [&](auto nz) { hipLaunchKernelGGL((k_relax32<decltype(nz)::value, RE, SN>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb); }))
      hipLaunchKernelGGL((k_relax32<0, RE, SN>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb);
  });
}

template <int NZMAX, int LANES, bool DIRECT>
static void launch_tail(hipStream_t st, const Tail32 &T, int cols, int real, int rb) {
  const dim3 blk(cols >= LANES ? LANES : (cols + WAVE - 1) / WAVE * WAVE);
  if (real && rb) hipLaunchKernelGGL((k_tail32<true, true, NZMAX, LANES, DIRECT>), dim3(1), blk, 0, st, T);
  else if (real) hipLaunchKernelGGL((k_tail32<true, false, NZMAX, LANES, DIRECT>), dim3(1), blk, 0, st, T);
  else if (rb) hipLaunchKernelGGL((k_tail32<false, true, NZMAX, LANES, DIRECT>), dim3(1), blk, 0, st, T);
  else hipLaunchKernelGGL((k_tail32<false, false, NZMAX, LANES, DIRECT>), dim3(1), blk, 0, st, T);
}
static dim3 whole_grid(int ny, int nx) { return dim3((ny / 2 + 1 + WAVE - 1) / WAVE, (nx + 2 + 3) / 4, 2); }

extern "C" {
// one colour pass: planes i0, i0+istep, ... (nplanes of them), j parity jodd_fixed (-1: red-black colour rb); snap: read the k=1
// diagonals from L->p1; ring: option "mixed_ring".  Returns 1 where k_relax32r served the pass, 0 where k_relax32 did.
int mgxx_relax_pass(hipStream_t st, const LevView32 *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, int ring) {
  const Choice c = choose_relax32(lev_shape32(L), nplanes, real, snap, ring, mgx_switches());
  launch_relax32(st, L, c, i0, istep, nplanes, jodd_fixed, rb, real, snap);
  return c.ret;
}
// what choose_relax32 answers for a colour pass of nplanes planes on a level of nx x ny x nz with option "mixed_ring" on, no launch: out[0..5] =
// served by k_relax32r, look-ahead D, planes per workgroup, non-temporal instance, workgroups, instance NZ (mgx_mixed_ring_levels, mgx_mixed_ring_choice)
void mgxx_ring_choice(int nx, int ny, int nz, int nplanes, int *out) {
  const LevShape s = {nx, ny, nz, false, false, false, false, 0};
  const Choice c = choose_relax32(s, nplanes, 0, 0, 1, mgx_switches());
  out[0] = c.family == KF_RELAX32R; out[1] = c.d; out[2] = (int)c.by; out[3] = c.stream; out[4] = (int)(c.grid * c.gy); out[5] = c.nz;
}
void mgxx_snapshot(hipStream_t st, const LevView32 *L) {
  hipLaunchKernelGGL(k_snapshot32, dim3((L->RS + 255) / 256, L->nx + 2), dim3(256), 0, st, *L);
}
void mgxx_residual(hipStream_t st, const LevView32 *L, int real) {
  const dim3 grd = col_grid(L->ny / 2, L->nx, 2), blk(WAVE, 4);
  if (real) hipLaunchKernelGGL(k_residual32<true>, grd, blk, 0, st, *L);
  else hipLaunchKernelGGL(k_residual32<false>, grd, blk, 0, st, *L);
}
void mgxx_resrest(hipStream_t st, const LevView32 *F, const LevView32 *C, int real) {
  const dim3 grd = col_grid(C->ny, C->nx), blk(WAVE, 4);
  if (real) hipLaunchKernelGGL(k_resrest32<true>, grd, blk, 0, st, *F, *C);
  else hipLaunchKernelGGL(k_resrest32<false>, grd, blk, 0, st, *F, *C);
}
void mgxx_restrict(hipStream_t st, const LevView32 *F, const LevView32 *C, const float *src) {
  hipLaunchKernelGGL(k_restrict32, col_grid(C->ny, C->nx), dim3(WAVE, 4), 0, st, *F, *C, src);
}
void mgxx_coarse2fine(hipStream_t st, const LevView32 *F, const LevView32 *C, int linear) {
  const int by = C->nz >= 4 ? 4 : C->nz;
  const dim3 blk(WAVE, by), grd((C->ny + WAVE - 1) / WAVE, (C->nz + by - 1) / by, C->nx);
  if (linear) hipLaunchKernelGGL(k_coarse2fine32<true>, grd, blk, 0, st, *F, *C);
  else hipLaunchKernelGGL(k_coarse2fine32<false>, grd, blk, 0, st, *F, *C);
}
// The tail kernel on levels levs[0 .. nl-1] (consecutive, finest first, all small): mode TAIL_RELAX = n sweeps of levs[0] (nl = 1),
// TAIL_VCYCLE = vcycle32(levs[0], lead) down to levs[nl-1] and back, TAIL_FCYCLE = fcycle32 with levs[0] as its finest level.  Returns 0,
// nothing launched, where the kernel does not serve the call (more levels than it takes, a level that is not small, levels that are not
// consecutive): tail_hand (mgx_cycle.cpp) keeps a cycle of more levels on its launches, anything else is the caller's error to report.
// dM (option "mixed_direct"): the operator of the coarsest level levs[nl-1], dn rows -- the coarsest solve of the cycle is then the product
// (a TAIL_VCYCLE of one level relaxes the e it finds: never with dM); nullptr = the sweeps, by the instances without the phase.
int mgxx_tail(hipStream_t st, const LevView32 *const *levs, int nl, int mode, int lead, int n, int ns_pre, int ns_post, int ns_coarsest, int rb,
              int real, int linear, const float *dM, int dn) {
  if (nl < 1 || nl > MIXED_TAIL_MAX_LEVELS || (mode == TAIL_RELAX && nl != 1)) return 0;
  if (dM && (mode == TAIL_RELAX || nl < 2 || dn != levs[nl - 1]->nx * levs[nl - 1]->ny * levs[nl - 1]->nz || dn > DIRECT32_MAX_N)) return 0;
  Tail32 T = {};
  for (int l = 0; l < nl; l++) {
    const LevView32 &v = *levs[l];
    if (!mixed_tail_small(v.nx, v.ny, v.nz) || (rb && real && !v.p1)) return 0;
    // (nz halves by integer division: 20, 10, 5, 2 is a hierarchy, and the transfers walk the coarse rows only)
    if (l > 0 && (2 * v.nx != levs[l - 1]->nx || 2 * v.ny != levs[l - 1]->ny || v.nz != levs[l - 1]->nz / 2)) return 0;
    T.L[l] = v;
    T.inst[l] = (v.nz == 2 || v.nz == 4 || v.nz == 8 || v.nz == 16 || v.nz == 32) ? v.nz : 0;
  }
  T.nl = nl; T.mode = mode; T.lead = lead; T.n = n; T.ns_pre = ns_pre; T.ns_post = ns_post; T.ns_coarsest = ns_coarsest; T.linear = linear;
  T.dM = dM; T.dn = dn;
  // one lane per column of the largest colour pass, whole waves, the instance's lanes at the most (the strided loops take the rest)
  const int cols = T.L[0].nx * (T.L[0].ny / 2);
  bool big = false;
  for (int l = 0; l < nl; l++) big = big || T.L[l].nz == 16 || T.L[l].nz == 32;
  if (big) { if (dM) launch_tail<32, MIXED_TAIL_LANES_B, true>(st, T, cols, real, rb); else launch_tail<32, MIXED_TAIL_LANES_B, false>(st, T, cols, real, rb); }
  else { if (dM) launch_tail<8, MIXED_TAIL_LANES_A, true>(st, T, cols, real, rb); else launch_tail<8, MIXED_TAIL_LANES_A, false>(st, T, cols, real, rb); }
  return 1;
}
int mgxx_tail_max_levels(void) { return MIXED_TAIL_MAX_LEVELS; }
// cells of the coarsest level nx x ny x nz of a hierarchy of nlevs levels that the product of option "mixed_direct" serves, 0 = the sweeps
// (any: option "small_any_nz"): mgx_mixed_direct_cells, and the launch below is made by the same function
int mgxx_direct32_cells(int nx, int ny, int nz, int nlevs, int any) {
  const LevShape s = {nx, ny, nz, false, false, false, false, 0};
  return choose_mixed_direct_cells(s, nlevs, any);
}
// M (n * n floats) = M64 rounded
void mgxx_direct32_round(hipStream_t st, const double *M64, float *M, int n) {
  const long long nn = (long long)n * n;
  hipLaunchKernelGGL(k_direct32_round, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, M64, M, nn);
}
// e = M f on the coarsest level L of a hierarchy of nlevs levels, with the images of e; returns 0, nothing launched, where the level is not served
int mgxx_coarse_direct32(hipStream_t st, const LevView32 *L, const float *M, int nlevs, int any) {
  const Choice c = choose_coarse_direct32(lev_shape32(L), nlevs, any);
  if (c.family != KF_DIRECT32) return 0;
  hipLaunchKernelGGL(k_coarse_direct32, dim3(c.grid), dim3(c.bx), 0, st, *L, M, c.nt);
  return c.ret;
}
void mgxx_to32(hipStream_t st, const LevView *D, const LevView32 *S, const double *src, float *dst, double scale) {
  hipLaunchKernelGGL(k_to32, whole_grid(D->ny, D->nx), dim3(WAVE, 4), 0, st, *D, *S, src, dst, scale);
}
void mgxx_to64(hipStream_t st, const LevView *D, const LevView32 *S, const float *src, double *dst, double scale, int add) {
  hipLaunchKernelGGL(k_to64, whole_grid(D->ny, D->nx), dim3(WAVE, 4), 0, st, *D, *S, src, dst, scale, add);
}
}  // extern "C"
