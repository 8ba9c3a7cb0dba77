// The z-line smoother of the multigrid cycle (mg_relax.f90:16-334) as HIP kernels for gfx950 (MI355X): one colour pass per
// launch on the bandwidth-bound levels, whole relax calls in one workgroup on the launch-bound ones.  Hand-written, fp64.
//
// All arithmetic keeps the reference's operation order and is compiled with -ffp-contract=off, so a colour pass of the
// four-colour smoother is bit-identical to the reference's CPU loop.
//
// Thread mapping everywhere: one lane = one (j,i) column, lanes run along the unit-stride half-row of
// the JS layout (mgx_internal.h), so every global access of a wave is one contiguous 512-byte run.
#include "mgx_switches.h"
#include "mgx_relax_common.h"
#include "mgx_choice.h"

// ------------------------------------------------------------------------------------------------
// z-line smoother, one colour pass.  mg_relax.f90:237-305 (relax_3D_8_heart) + :308-334 (tridiag).
// Columns of one colour never read each other (four-colour), or only through the k=1 horizontal
// diagonals (red-black): those are then read from the snapshot L.p1 taken before the pass (SNAP).
// The tridiagonal pivots (bet, gam) depend on the matrix only and are precomputed at set-up.
// ------------------------------------------------------------------------------------------------
// One column (any nz >= 2, a runtime value): forward sweep through p, back substitution re-reading it.  No mirrors.
template <bool REAL, bool SNAP>
__device__ __forceinline__ void relax_col_any(const LevView &L, const int i, const int jh, const int jodd) {
  int c, jm, jp;  // positions of columns j, j-1, j+1 inside a row
  COL_POS(L, jh, jodd, c, jm, jp)
  const long long RS = L.RS;
  const int nz = L.nz;
  double *__restrict__ p = L.p;
  const double *__restrict__ b = L.b;
  const double *__restrict__ a2 = L.cA[1], *__restrict__ a3 = L.cA[2], *__restrict__ a4 = L.cA[3],
               *__restrict__ a5 = L.cA[4], *__restrict__ a6 = L.cA[5], *__restrict__ a7 = L.cA[6],
               *__restrict__ a8 = L.cA[7], *__restrict__ bet = L.bet, *__restrict__ gam = L.gam;
  const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;

  // neighbour rows: p of (j-1,i) and (j,i-1); products coef*p of (j+1,i) [slots 3,4,5] and (j,i+1) [6,7,8]
  double pjm_m, pjm_0, pjm_p, pim_m, pim_0, pim_p;
  double m3_m, m3_0, m4_0, m5_p, n6_m, n6_0, n7_0, n8_p;
  double m3_p, m4_p, n6_p, n7_p;
#define LOAD_ROW(q, PJM, PIM, M3, M4, M5, N6, N7, N8)                         \
  {                                                                            \
    const long long ro = (long long)((q)-1) * RS;                              \
    PJM = p[o + ro + jm];                                                      \
    PIM = p[om + ro + c];                                                      \
    const double pj_ = p[o + ro + jp], pi_ = p[op + ro + c];                   \
    M3 = a3[o + ro + jp] * pj_; M4 = a4[o + ro + jp] * pj_; M5 = a5[o + ro + jp] * pj_; \
    N6 = a6[op + ro + c] * pi_; N7 = a7[op + ro + c] * pi_; N8 = a8[op + ro + c] * pi_; \
  }
  double dum5, dum8;
  LOAD_ROW(1, pjm_0, pim_0, m3_0, m4_0, dum5, n6_0, n7_0, dum8);
  LOAD_ROW(2, pjm_p, pim_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);
  (void)dum5; (void)dum8;

  // ---- k = 1 (mg_relax.f90:262-279)
  double rhs = ROW_RHS_FIRST(b[o + c], ST_TERMS(o + c));
  if (REAL) {  // the loads stay in the products: through K1_DIAG, all eight first, the three REAL kernels of this text compile differently
    K1_SNAP_ADDR(SNAP)
    rhs = rhs - a5[o + c] * q1[sm + jp] - a5[op + jm] * q1[sp + jm] - a8[o + c] * q1[sm + jm] - a8[op + jp] * q1[sp + jp];
  }
  double x = rhs * bet[o + c];
  p[o + c] = x;

  // ---- k = 2 .. nz-1 (:281-291)
  for (int k = 2; k <= nz - 1; k++) {
    pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p;
    m3_m = m3_0; m3_0 = m3_p; m4_0 = m4_p; n6_m = n6_0; n6_0 = n6_p; n7_0 = n7_p;
    LOAD_ROW(k + 1, pjm_p, pim_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);
    const long long ko = o + (long long)(k - 1) * RS + c;
    rhs = ROW_RHS_MID(b[ko], ST_TERMS(ko));
    x = (rhs - a2[ko] * x) * bet[ko];
    p[ko] = x;
  }
  // ---- k = nz (:293-301)
  {
    pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p;
    m3_m = m3_0; m4_0 = m4_p; n6_m = n6_0; n7_0 = n7_p;
    const long long ko = o + (long long)(nz - 1) * RS + c;
    rhs = ROW_RHS_LAST(b[ko], ST_TERMS(ko));
    x = (rhs - a2[ko] * x) * bet[ko];
    p[ko] = x;
  }
  // ---- back substitution (:330-332): xc(k) = xc(k) - gam(k+1)*xc(k+1)
  for (int k = nz - 1; k >= 1; k--) {
    const long long ko = o + (long long)(k - 1) * RS + c;
    x = p[ko] - gam[ko + RS] * x;
    p[ko] = x;
  }
#undef LOAD_ROW
}

template <bool REAL, bool SNAP>
__global__ __launch_bounds__(256) void k_relax_colour(LevView L, int i0, int istep, int nplanes, int jodd_fixed, int rb, Sides ph) {
  const int jh = blockIdx.x * WAVE + threadIdx.x;
  const int ipl = blockIdx.y * blockDim.y + threadIdx.y;
  if (jh >= (L.ny >> 1) || ipl >= nplanes) return;
  const int i = i0 + istep * ipl;
  // RB: j = 1+mod(i+rb,2),ny,2 (mg_relax.f90:174) ; FC: fixed parity (:216-217)
  const int jodd = jodd_fixed >= 0 ? jodd_fixed : (((i + rb) & 1) == 0);
  if (sides_part_skip(ph, i, L.nx, jodd, blockIdx.x, gridDim.x)) return;
  relax_col_any<REAL, SNAP>(L, i, jh, jodd);
}


// ------------------------------------------------------------------------------------------------
// Register-resident variant of the colour pass for nz in {2,...,64} (level 1 of the 512x512x64 problem
// is NZ=64).  One wave = 64 columns; a colour of a 512^2 level is only 1024 waves (1 per SIMD), so the
// kernel is written for ONE wave per SIMD and spends its 512-VGPR budget on memory-level parallelism:
//   * the k loop is fully unrolled and software-pipelined: raw neighbour/own rows are loaded D rows ahead
//     into register rings, so ~D*19 independent 512-byte loads are in flight per wave;
//   * the forward solution x(k) and the back-substitution factors gam(k) stay in registers: p is written
//     once (no forward store + backward re-read), and the backward sweep does no dependent loads;
//   * physical-boundary mirrors of the updated columns (mg_mpi_exchange.f90:509-537,552-597) are stored by
//     the lane that owns the column, which removes the separate halo kernel after every colour.
// The forward rows are the stored-coefficient text of mgx_relax_common.h (SC_ROW), shared with the tall-column pass of
// mgx_relax_tall.hip; it expands ROW_RHS_* (mgx_device.h) as relax_col_any of k_relax_colour does: bit-identical results.
// ------------------------------------------------------------------------------------------------
template <int NZ, bool REAL, bool SNAP, int D>
__device__ __forceinline__ void relax_col_nz(const LevView &L, const int i, const int jh, const int jodd, const Sides ph) {
  int c, jm, jp;
  COL_POS(L, jh, jodd, c, jm, jp)
  constexpr bool ST = false;  // stored-slot path: coarser levels / user matrices, which live in the caches
#define SC_G_PUT(kk, v) g[(kk)-1] = (v);
#define SC_X_PUT(kk, v) x[(kk)-1] = (v);
  SC_PROLOGUE(NZ, NZ)
#pragma unroll
  for (int k = 1; k <= NZ; k++) SC_ROW(k)
#undef SC_G_PUT
#undef SC_X_PUT
  // back substitution in registers, then one store per cell (+ mirrors on physical boundaries)
#pragma unroll
  for (int k = NZ - 1; k >= 1; k--) x[k - 1] = x[k - 1] - g[k] * x[k];

  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
  COL_IMAGES(L, i, j, ph)
#pragma unroll
  for (int k = 1; k <= NZ; k++) {
    const long long ro = (long long)(k - 1) * RS;
    const double v = x[k - 1];
    COL_STORE(false, p, o, ro, c, v)
  }
  if (SNAP && L.d0w != nullptr) L.d0w[(long long)i * RS + c] = x[0] - L.p1[(long long)i * RS + c];  // mgx_rbseq.hip (b): d0, what k_rbseq_d0 would compute from the stored y
  if (SNAP && L.p1w != nullptr) COL_SNAPSHOT(L, RS, i, c, x[0])
}

// ------------------------------------------------------------------------------------------------
// Matrix-free cross terms, generated slots 4 / 7 (ZW), own slopes (ZG) and pivots: the column pass of mgx_relax_common.h with x(k)
// in registers.  ZW and ZG are parameters because the NZ < 32 instances use the stored slots (k_relax_nz decides).
// GL: gam(k) waits in LDS (gl: NZ rows x 64 lanes per wave) instead of registers.  At NZ = 64 x and gam together take half of
// the 512 registers; with the in-kernel pivots on top the kernel spilled (268 B/lane of scratch) -- 32 KB of LDS per wave
// (one wave per SIMD: 128 KB of the CU's 160 KB) frees 128 registers, and the backward sweep's reads are independent of its
// dependency chain.
// ------------------------------------------------------------------------------------------------
template <int NZ, bool REAL, bool SNAP, int D, bool ST, bool GL = false, bool ZW = false, bool ZG = false>
__device__ __forceinline__ void relax_col_mf(const LevView &L, const int i, const int jh, const int jodd, const Sides ph, double *__restrict__ gl = nullptr) {
  int c, jm, jp;
  COL_POS(L, jh, jodd, c, jm, jp)
  constexpr bool PAIR = true;
#define MF_G_PUT(kk, v) { if (GL) gl[((kk)-1) * WAVE + lane] = (v); else g[GL ? 0 : (kk)-1] = (v); }
#define MF_X_PUT(kk, v, a2k, betk) x[(kk)-1] = (v);
  MF_PROLOGUE(NZ, GL ? 1 : NZ)
#pragma unroll
  for (int k = 1; k <= NZ; k++) MF_ROW(k)
#undef MF_G_PUT
#undef MF_X_PUT
#pragma unroll
  for (int k = NZ - 1; k >= 1; k--) x[k - 1] = x[k - 1] - (GL ? gl[k * WAVE + lane] : g[GL ? 0 : k]) * x[k];

  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
  COL_IMAGES(L, i, j, ph)
#pragma unroll
  for (int k = 1; k <= NZ; k++) {
    const long long ro = (long long)(k - 1) * RS;
    const double v = x[k - 1];
    COL_STORE(ST, p, o, ro, c, v)
  }
  if (SNAP && L.d0w != nullptr) L.d0w[(long long)i * RS + c] = x[0] - L.p1[(long long)i * RS + c];  // mgx_rbseq.hip (b): d0, what k_rbseq_d0 would compute from the stored y
  if (SNAP && L.p1w != nullptr) COL_SNAPSHOT(L, RS, i, c, x[0])
}

template <int NZ, bool REAL, bool SNAP, int D, bool MF, bool ST>
__global__ __launch_bounds__(128, 1) void k_relax_nz(LevView L, int i0, int istep, int nplanes, int jodd_fixed, int rb, Sides ph, int gx) {
  const int npair = (nplanes + blockDim.y - 1) / blockDim.y;
  int bx, ipr;  // j-chunk, plane pair
  XCD_BLOCK_MAP(npair, gx, bx, ipr)
  const int ipl = ipr * blockDim.y + threadIdx.y;
  const int jh = bx * WAVE + threadIdx.x;
  if (jh >= (L.ny >> 1) || ipl >= nplanes) return;
  const int i = i0 + istep * ipl;
  // RB: j = 1+mod(i+rb,2),ny,2 (mg_relax.f90:174) ; FC: fixed parity (:216-217)
  const int jodd = jodd_fixed >= 0 ? jodd_fixed : (((i + rb) & 1) == 0);
  if (sides_part_skip(ph, i, L.nx, jodd, bx, gx)) return;  // wave-uniform
  constexpr bool GL = gam_in_lds<NZ, MF>;
  constexpr bool ZW = MF && NZ >= 32;  // generated slots 4 / 7 and own slopes: the levels whose streams come from HBM
  if (GL) {
    extern __shared__ double g_lds[];  // blockDim.y waves x NZ rows x 64 lanes
    relax_col_mf<NZ, REAL, SNAP, D, ST, GL, ZW, ZW>(L, i, jh, jodd, ph, g_lds + (size_t)threadIdx.y * NZ * WAVE);
  } else if (MF) relax_col_mf<NZ, REAL, SNAP, D, ST, false, ZW, ZW>(L, i, jh, jodd, ph);
  else relax_col_nz<NZ, REAL, SNAP, D>(L, i, jh, jodd, ph);
}

// Lexicographic Gauss-Seidel (mg_relax.f90:116-148) on the device, EXACTLY: column (j,i) of the reference's
// `do i; do j` sweep reads new values of (j-1,i), (j,i-1), (j+1,i-1), (j-1,i-1) and old values of the rest, so all
// columns with equal t = j + 2 i are independent and hyperplanes t = 3 .. ny+2nx are processed in order (one
// launch each).  Slow (launch-bound, ~ny+2nx launches per sweep) but bit-identical to the sequential loop.
template <int NZ, bool REAL>
__global__ __launch_bounds__(64, 1) void k_relax_gs_front(LevView L, int t) {
  int ilo = (t - L.ny + 1) / 2; if (ilo < 1) ilo = 1;        // j = t - 2i <= ny
  const int i = ilo + blockIdx.x * WAVE + threadIdx.x;
  const int j = t - 2 * i;
  if (i > L.nx || j < 1 || j > L.ny) return;
  const Sides none = {0, 0, 0, 0};  // halo is refreshed once per sweep, after the loop (mg_relax.f90:141)
  relax_col_nz<NZ, REAL, false, 1>(L, i, (j - 1) >> 1, j & 1, none);
}
// the same hyperplane for a level with no register-resident instance (runtime nz: 128, and the sizes that are not powers of two)
template <bool REAL>
__global__ __launch_bounds__(64, 1) void k_relax_gs_front_any(LevView L, int t) {
  int ilo = (t - L.ny + 1) / 2; if (ilo < 1) ilo = 1;
  const int i = ilo + blockIdx.x * WAVE + threadIdx.x;
  const int j = t - 2 * i;
  if (i > L.nx || j < 1 || j > L.ny) return;
  relax_col_any<REAL, false>(L, i, (j - 1) >> 1, j & 1);
}

// Whole relax(lev, nsweeps) of a SMALL level (<= 1024 columns per colour, no neighbours) in ONE launch of ONE
// workgroup: colours are separated by __syncthreads() instead of kernel boundaries.  The coarsest-level solve of
// the reference (40 sweeps, mg_solvers.f90:117,144) is 160 colour passes of a 16x16x2 grid: launch-bound as
// separate kernels, ~1 us per pass here.  method: 1 = RB, 2 = FC.
template <int NZ, bool REAL, int MAXT>
__global__ __launch_bounds__(MAXT) void k_relax_small(LevView L, int nsweeps, int method, Sides ph, int exact) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int nyh = L.ny >> 1;
  for (int it = 0; it < nsweeps; it++) {
    const int ncolour = method == 2 ? 4 : 2;
    for (int cidx = 0; cidx < ncolour; cidx++) {
      if (method == 1 && REAL && exact) {
        // the reference's sequential red-black order (mg_relax.f90:173-176): planes i = 1..nx one after the other, so that a
        // column reads the already updated same-colour k=1 diagonals of plane i-1 and the old ones of plane i+1 (:271-276)
        for (int i = 1; i <= L.nx; i++) {
          const int jodd = ((i + cidx + 1) & 1) == 0;
          for (int t = tid; t < nyh; t += nth) relax_col_nz<NZ, REAL, false, 1>(L, i, t, jodd, ph);
          __syncthreads();
        }
        continue;
      }
      if (method == 1 && REAL) {  // snapshot of p(k=1) for the same-colour diagonals of red-black
        for (int t = tid; t < (L.nx + 2) * L.RS; t += nth) L.p1[t] = L.p[(long long)(t / L.RS) * L.plane + (t % L.RS)];
        __syncthreads();
      }
      const int ncol = method == 2 ? (L.nx >> 1) * nyh : L.nx * nyh;
      for (int t = tid; t < ncol; t += nth) {
        const int ipl = t / nyh, jh = t - ipl * nyh;
        int i, jodd;
        if (method == 2) { i = 1 + (cidx >> 1) + 2 * ipl; jodd = (cidx & 1) == 0; }
        else { i = 1 + ipl; jodd = ((i + cidx + 1) & 1) == 0; }
        if (method == 1) relax_col_nz<NZ, REAL, REAL, 1>(L, i, jh, jodd, ph);
        else relax_col_nz<NZ, REAL, false, 1>(L, i, jh, jodd, ph);
      }
      __syncthreads();
    }
  }
}

// snapshot of p(k=1,:,:) for the parallel red-black pass
__global__ void k_snapshot_k1(LevView L) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (t < L.RS) L.p1[(long long)i * L.RS + t] = L.p[(long long)i * L.plane + t];
}


// Register-resident relax of a level with <= 1024 columns (the coarsest levels: 16x16x2, and 16x16x4 / 32x32x2 class
// grids): ONE workgroup, one thread per column for the whole call.  Everything that does not change between colour
// passes -- b, the 7 own off-diagonal slots and pivots, the 6 neighbour slots the symmetric storage makes a column
// read, the k=1 diagonal slots, gam -- is loaded into registers once; only p lives in LDS (with its mirrored halo) and
// is exchanged there.  A colour pass is then ~4 NZ LDS reads, ~30 NZ flops and one barrier (0.1-0.2 us instead of
// 0.8 us with every operand re-read from LDS, and ~5 us as a separate launch): relax(nlevs, ns_coarsest=40) is 160
// dependent passes.  The rows expand ROW_RHS_* (mgx_device.h), as relax_col_nz's do: bit-identical.
template <int NZ, bool REAL, int MAXT>
__global__ __launch_bounds__(MAXT) void k_relax_reg(LevView G, int nsweeps, int method, Sides ph, int exact_in) {
  extern __shared__ double ldsr[];
  double *lds = ldsr;
  const int nx = G.nx, ny = G.ny, W = ny + 2, PL = (nx + 2) * W;  // P[k][i][j]
  double *__restrict__ P = lds, *__restrict__ P1 = lds + NZ * PL;  // P1: k=1 snapshot of the parallel red-black pass
  const int tid = threadIdx.x, nth = blockDim.x;
#define GI(k0, jj, ii) ((long long)(ii) * G.plane + (long long)(k0) * G.RS + jpos(G, jj))
  for (int t = tid; t < NZ * PL; t += nth) {
    const int k0 = t / PL, r = t - k0 * PL, i = r / W, j = r - i * W;
    P[t] = G.p[GI(k0, j, i)];
  }
  const int j = 1 + tid % ny, i = 1 + tid / ny;
  const bool mine = tid < nx * ny;
  double ob[NZ], a2[NZ], a3[NZ], a4[NZ], a5[NZ], a6[NZ], a7[NZ], a8[NZ], bet[NZ], g[NZ];
  double r3[NZ], r4[NZ], r5[NZ], r6[NZ], r7[NZ], r8[NZ], e2 = 0, e4 = 0;
  if (mine) {
#pragma unroll
    for (int k = 0; k < NZ; k++) {
      const long long c = GI(k, j, i), cj = GI(k, j + 1, i), ci = GI(k, j, i + 1);
      ob[k] = G.b[c]; a2[k] = G.cA[1][c]; a3[k] = G.cA[2][c]; a4[k] = G.cA[3][c]; a5[k] = G.cA[4][c];
      a6[k] = G.cA[5][c]; a7[k] = G.cA[6][c]; a8[k] = G.cA[7][c]; bet[k] = G.bet[c];
      r3[k] = G.cA[2][cj]; r4[k] = G.cA[3][cj]; r5[k] = G.cA[4][cj];
      r6[k] = G.cA[5][ci]; r7[k] = G.cA[6][ci]; r8[k] = G.cA[7][ci];
    }
    if (REAL) { e2 = G.cA[4][GI(0, j - 1, i + 1)]; e4 = G.cA[7][GI(0, j + 1, i + 1)]; }
    g[0] = 0.0;
#pragma unroll
    for (int k = 1; k < NZ; k++) g[k] = a2[k] * bet[k - 1];  // gam(k) = dd(k-1)*bet(k-1) (mg_relax.f90:325)
  }
  __syncthreads();
  const bool mS = ph.S && j == 1, mN = ph.N && j == ny, mW = ph.W && i == 1, mE = ph.E && i == nx;
  const int ncolour = method == 2 ? 4 : 2;
  // exact: the reference's sequential red-black order (mg_relax.f90:173-176) -- the planes of a colour one after the other,
  // k=1 diagonals read from p itself (new in plane i-1, old in plane i+1) instead of the snapshot
  const bool exact = exact_in && method == 1 && REAL;
  for (int it = 0; it < nsweeps; it++) {
    for (int cidx = 0; cidx < ncolour; cidx++) {
      if (method == 1 && REAL && !exact) {
        for (int t = tid; t < PL; t += nth) P1[t] = P[t];
        __syncthreads();
      }
      bool colour;
      if (method == 2) colour = ((i & 1) == ((cidx >> 1) ? 0 : 1)) && ((j & 1) == ((cidx & 1) ? 0 : 1));  // mg_relax.f90:214-217
      else colour = (j & 1) == ((((i + cidx + 1) & 1) == 0) ? 1 : 0);                                        // :174
      const int nstep = exact ? nx : 1;
      for (int ip = 1; ip <= nstep; ip++) {
      const bool active = colour && (!exact || i == ip);
      if (mine && active) {
        double x[NZ];
        const double *__restrict__ Q1 = (method == 1 && REAL && !exact) ? P1 : P;
        double d1 = 0, d2 = 0, d3 = 0, d4 = 0;
        if (REAL) { d1 = Q1[(i - 1) * W + j + 1]; d2 = Q1[(i + 1) * W + j - 1]; d3 = Q1[(i - 1) * W + j - 1]; d4 = Q1[(i + 1) * W + j + 1]; }
        double pjm[NZ], pjp[NZ], pim[NZ], pip[NZ];
#pragma unroll
        for (int k = 0; k < NZ; k++) {
          const int o = k * PL + i * W + j;
          pjm[k] = P[o - 1]; pjp[k] = P[o + 1]; pim[k] = P[o - W]; pip[k] = P[o + W];
        }
        double xv = 0.0;
#pragma unroll
        for (int k = 0; k < NZ; k++) {
          double rhs;
          // row k + 1 as the arguments of ROW_RHS_* (mgx_device.h); the rows a form leaves out are never indexed
#define REG_TERMS ob[k], a3[k] * pjm[k + 1], r3[k - 1] * pjp[k - 1], a4[k] * pjm[k], r4[k] * pjp[k], a5[k] * pjm[k - 1], r5[k + 1] * pjp[k + 1], \
                  a6[k] * pim[k + 1], r6[k - 1] * pip[k - 1], a7[k] * pim[k], r7[k] * pip[k], a8[k] * pim[k - 1], r8[k + 1] * pip[k + 1]
          if (k == 0) {
            rhs = ROW_RHS_FIRST(REG_TERMS);
            if (REAL) rhs = rhs - a5[0] * d1 - e2 * d2 - a8[0] * d3 - e4 * d4;
            xv = rhs * bet[k];
          } else if (k < NZ - 1) {
            rhs = ROW_RHS_MID(REG_TERMS);
            xv = (rhs - a2[k] * xv) * bet[k];
          } else {
            rhs = ROW_RHS_LAST(REG_TERMS);
            xv = (rhs - a2[k] * xv) * bet[k];
          }
#undef REG_TERMS
          x[k] = xv;
        }
#pragma unroll
        for (int k = NZ - 2; k >= 0; k--) x[k] = x[k] - g[k + 1] * x[k + 1];
#pragma unroll
        for (int k = 0; k < NZ; k++) {
          const int o = k * PL;
          const double v = x[k];
          P[o + i * W + j] = v;
          if (mS) P[o + i * W] = v;
          if (mN) P[o + i * W + ny + 1] = v;
          if (mW) { P[o + j] = v; if (mS) P[o] = v; if (mN) P[o + ny + 1] = v; }
          if (mE) { P[o + (nx + 1) * W + j] = v; if (mS) P[o + (nx + 1) * W] = v; if (mN) P[o + (nx + 1) * W + ny + 1] = v; }
        }
      }
      __syncthreads();
      }
    }
  }
  for (int t = tid; t < NZ * PL; t += nth) {
    const int k0 = t / PL, r = t - k0 * PL, ii = r / W, jj = r - ii * W;
    G.p[GI(k0, jj, ii)] = P[t];
  }
#undef GI
}

// Coarsest-level solve entirely out of LDS: when p, b, slots 2..8 and the pivots of a level fit in 64 KB (16x16x2:
// 57 KB), ONE workgroup copies them in (compact JS layout), runs all nsweeps x colours with the same column routine
// (its pointers now address LDS), and writes p back.  relax(nlevs, ns_coarsest=40) = 160 dependent colour passes:
// ~0.3 us each from LDS instead of ~1.1 us through L2 (and ~5 us as separate launches).
template <int NZ, bool REAL>
__global__ __launch_bounds__(256) void k_relax_tiny(LevView G, int nsweeps, int method, Sides ph) {
  extern __shared__ double lds[];
  LevView L = G;
  L.EO = 0; L.HO = (G.ny >> 1) + 1; L.RS = G.ny + 2; L.plane = (long long)NZ * L.RS;
  const int n3 = (G.nx + 2) * (int)L.plane;
  double *base = lds;
  L.p = base; base += n3; L.b = base; base += n3;
  for (int q = 1; q < 8; q++) { L.cA[q] = base; base += n3; }
  L.cA[0] = nullptr; L.bet = base; base += n3; L.gam = nullptr; L.zy = L.zx = nullptr;
  L.p1 = base;
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int t = tid; t < n3; t += nth) {  // copy in: compact index t -> (i,k,j) -> padded global index
    const int i = t / (int)L.plane, rem = t - i * (int)L.plane, k = rem / L.RS, pos = rem - k * L.RS;
    const int j = pos < L.HO ? 2 * pos : 2 * (pos - L.HO) + 1;
    const long long gidx = (long long)i * G.plane + (long long)k * G.RS + jpos(G, j);
    L.p[t] = G.p[gidx]; L.b[t] = G.b[gidx]; L.bet[t] = G.bet[gidx];
    for (int q = 1; q < 8; q++) L.cA[q][t] = G.cA[q][gidx];
  }
  __syncthreads();
  const int nyh = L.ny >> 1;
  for (int it = 0; it < nsweeps; it++) {
    const int ncolour = method == 2 ? 4 : 2;
    for (int cidx = 0; cidx < ncolour; cidx++) {
      if (method == 1 && REAL) {
        for (int t = tid; t < (L.nx + 2) * L.RS; t += nth) L.p1[t] = L.p[(t / L.RS) * (int)L.plane + (t % L.RS)];
        __syncthreads();
      }
      const int ncol = method == 2 ? (L.nx >> 1) * nyh : L.nx * nyh;
      for (int t = tid; t < ncol; t += nth) {
        const int ipl = t / nyh, jh = t - ipl * nyh;
        int i, jodd;
        if (method == 2) { i = 1 + (cidx >> 1) + 2 * ipl; jodd = (cidx & 1) == 0; }
        else { i = 1 + ipl; jodd = ((i + cidx + 1) & 1) == 0; }
        if (method == 1) relax_col_nz<NZ, REAL, REAL, 1>(L, i, jh, jodd, ph);
        else relax_col_nz<NZ, REAL, false, 1>(L, i, jh, jodd, ph);
      }
      __syncthreads();
    }
  }
  for (int t = tid; t < n3; t += nth) {  // copy p back (halo included: the column routine kept it mirrored)
    const int i = t / (int)L.plane, rem = t - i * (int)L.plane, k = rem / L.RS, pos = rem - k * L.RS;
    const int j = pos < L.HO ? 2 * pos : 2 * (pos - L.HO) + 1;
    G.p[(long long)i * G.plane + (long long)k * G.RS + jpos(G, j)] = L.p[t];
  }
}

// ---- the launchers: a Choice (mgx_choice.h) to its template instance ----
static void launch_small(hipStream_t st, const LevView *L, const Choice &c, int nsweeps, int method, int real, Sides ph, int exact) {
  const dim3 grd(c.grid), blk(c.bx);
  with_bool(real, [&](auto R) {
    constexpr bool REAL = decltype(R)::value;
    if (c.family == KF_TINY) with_nz<2, 4>(c.nz, [&](auto N) { hipLaunchKernelGGL((k_relax_tiny<decltype(N)::value, REAL>), grd, blk, c.lds, st, *L, nsweeps, method, ph); });
    else if (c.family == KF_REG && c.nt == 1024) hipLaunchKernelGGL((k_relax_reg<2, REAL, 1024>), grd, blk, c.lds, st, *L, nsweeps, method, ph, exact);
    else if (c.family == KF_REG) with_nz<3, 4, 5, 6, 7>(c.nz, [&](auto N) { hipLaunchKernelGGL((k_relax_reg<decltype(N)::value, REAL, 256>), grd, blk, c.lds, st, *L, nsweeps, method, ph, exact); });
    else if (c.nt == 1024) hipLaunchKernelGGL((k_relax_small<2, REAL, 1024>), grd, blk, c.lds, st, *L, nsweeps, method, ph, exact);
    else with_nz<2, 3, 4, 5, 6, 7, 8>(c.nz, [&](auto N) { hipLaunchKernelGGL((k_relax_small<decltype(N)::value, REAL, 256>), grd, blk, c.lds, st, *L, nsweeps, method, ph, exact); });
  });
}
// a colour pass of k_relax_nz or of the generic column
static void launch_colour(hipStream_t st, const LevView *L, const Choice &c, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  const dim3 grd(c.grid, c.gy), blk(c.bx, c.by);
  with_real_and(real, snap, [&](auto R, auto S) {
    constexpr bool REAL = decltype(R)::value, SNAP = decltype(S)::value;
    if (c.family == KF_COLOUR) { hipLaunchKernelGGL((k_relax_colour<REAL, SNAP>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph); return; }
    with_nz<REG_NZ_LIST>(c.nz, [&](auto N) {
      constexpr int NZ = decltype(N)::value, D = ch_colour_depth(NZ);
      with_mf_stream(c.mf, c.stream, [&](auto M, auto T) {
        hipLaunchKernelGGL((k_relax_nz<NZ, REAL, SNAP, D, decltype(M)::value, decltype(T)::value>), grd, blk, c.lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, c.gx);
      });
    });
  });
}

extern "C" {

// one Gauss-Seidel sweep as ny+2nx-2 hyperplane launches
int mgxk_relax_gs_sweep(hipStream_t st, const LevView *L, int real) {
  const LevShape s = lev_shape(L);
  for (int t = 3; t <= L->ny + 2 * L->nx; t++) {
    const Choice c = choose_gs_front(s, t);
    if (!c.grid) continue;
    const dim3 grd(c.grid), blk(c.bx);
    with_bool(real, [&](auto R) {
      constexpr bool REAL = decltype(R)::value;
      if (c.family == KF_GS) with_nz<2, 4, 8, 16, 32, 64>(c.nz, [&](auto N) { hipLaunchKernelGGL((k_relax_gs_front<decltype(N)::value, REAL>), grd, blk, 0, st, *L, t); });
      else hipLaunchKernelGGL((k_relax_gs_front_any<REAL>), grd, blk, 0, st, *L, t);
    });
  }
  return 1;
}

// one-launch relax of a small level; returns 0 if the level does not qualify, else what choose_small (mgx_choice.h) says
int mgxk_relax_small(hipStream_t st, const LevView *L, int nsweeps, int method, int real, Sides ph, int mode, int any) {
  mgx_before_launch();
  const Choice c = choose_small(lev_shape(L), method, real, ph, mode, any, mgx_switches());
  if (c.ask_wave >= 0 && mgxk_relax_wave(st, L, nsweeps, method, real, ph, mode, c.ask_wave)) return c.wave_ret;
  if (c.family == KF_NONE) return 0;
  launch_small(st, L, c, nsweeps, method, real, ph, mode != 0);
  return mgx_launched() ? c.ret : 0;
}

// returns what the pass did (mgx_wrappers.h): PASS_MIRRORS the kernel stored the physical mirrors of p itself (no k_halo_phys needed); PASS_D0 it
// wrote L->d0w; PASS_TALL_STORED it was the stored-coefficient tall-column pass (mgx_relax_tall.hip; relax() counts those)
int mgxk_relax_colour(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  if (const int ks = mgxk_relax_ks(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph)) return ks;  // mid levels: rows split over the waves of a workgroup
  const LevShape s = lev_shape(L);
  Choice c = choose_colour(s, nplanes, real, snap, mgx_switches());
  if (c.family == KF_TALL || c.family == KF_TALL_ST) {
    if (const int tall = mgxk_relax_tall(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph)) return tall;
    c = choose_colour_generic(s, nplanes);  // the launch was refused
  }
  launch_colour(st, L, c, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph);
  return c.ret;
}
// does mgxk_relax_colour run a register-resident kernel (which writes mirrors and chained snapshots) on this level?
int mgxk_has_reg_kernel(const LevView *L) { return choose_has_reg_kernel(lev_shape(L), mgx_switches()); }
void mgxk_snapshot_k1(hipStream_t st, const LevView *L) {
  hipLaunchKernelGGL(k_snapshot_k1, dim3((L->RS + 255) / 256, L->nx + 2), dim3(256), 0, st, *L);
}

}  // extern "C"
