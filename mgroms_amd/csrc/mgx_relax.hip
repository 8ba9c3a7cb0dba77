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
template <int NZ, bool MF> constexpr bool gam_in_lds = MF && NZ == 64;  // read by k_relax_nz and by the launch that sizes its LDS
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

template <int NZ, int D>
static void launch_relax_nz_d(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  const int gx0 = (L->ny / 2 + WAVE - 1) / WAVE, gx = mgx_switches().no_xcd ? -gx0 : gx0;
  // two planes per workgroup only when there are plenty of workgroups (it halves the number of CUs a small level uses)
  const int by = gx0 * nplanes >= 2048 ? 2 : 1;
  dim3 blk(WAVE, by), grd(gx0 * ((nplanes + by - 1) / by));
  const bool mf = L->zy != nullptr && NZ >= 16;  // matrix-free cross terms on the bandwidth-bound levels
  // streaming (nontemporal) hints only when the level cannot live in the 256 MB Infinity Cache between passes:
  // measured +14 % on the 1.2 GB level 1, -20 % on the 150 MB level 2 which is otherwise re-read from cache
  const bool stream = mf && (double)L->nx * L->ny * NZ * 72.0 > 256e6;
#define LAUNCH_NZ(MFV, STV)                                                                                              \
  {                                                                                                                       \
    const size_t lds = gam_in_lds<NZ, MFV> ? (size_t)by * NZ * WAVE * sizeof(double) : 0;  /* 32 KB per wave (GL, relax_col_mf) */ \
    if (real && snap) hipLaunchKernelGGL((k_relax_nz<NZ, true, true, D, MFV, STV>), grd, blk, lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, gx); \
    else if (real) hipLaunchKernelGGL((k_relax_nz<NZ, true, false, D, MFV, STV>), grd, blk, lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, gx);   \
    else hipLaunchKernelGGL((k_relax_nz<NZ, false, false, D, MFV, STV>), grd, blk, lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, gx);            \
  }
  if (mf && stream) LAUNCH_NZ(true, true)
  else if (mf) LAUNCH_NZ(true, false)
  else LAUNCH_NZ(false, false)
#undef LAUNCH_NZ
}
template <int NZ>
static void launch_relax_nz(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  // look-ahead depth D (rows of loads in flight)
  // measured: NZ=16 6.3 us/pass at D=2 vs 9.3 at D=3; NZ>=32 flat for D=2..5
  constexpr int D = NZ >= 32 ? 3 : (NZ >= 8 ? 2 : 1);
  launch_relax_nz_d<NZ, D>(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph);
}

extern "C" {

// one Gauss-Seidel sweep as ny+2nx-2 hyperplane launches (register-resident columns for nz a power of two <= 64, any nz otherwise)
int mgxk_relax_gs_sweep(hipStream_t st, const LevView *L, int real) {
  for (int t = 3; t <= L->ny + 2 * L->nx; t++) {
    int ilo = (t - L->ny + 1) / 2; if (ilo < 1) ilo = 1;
    int ihi = (t - 1) / 2; if (ihi > L->nx) ihi = L->nx;
    if (ihi < ilo) continue;
    dim3 grd((ihi - ilo + 1 + WAVE - 1) / WAVE), blk(WAVE);
#define GS_CASE(NZV) case NZV: if (real) hipLaunchKernelGGL((k_relax_gs_front<NZV, true>), grd, blk, 0, st, *L, t); \
                               else hipLaunchKernelGGL((k_relax_gs_front<NZV, false>), grd, blk, 0, st, *L, t); break;
    switch (L->nz) {
      GS_CASE(2) GS_CASE(4) GS_CASE(8) GS_CASE(16) GS_CASE(32) GS_CASE(64)
      default: if (real) hipLaunchKernelGGL((k_relax_gs_front_any<true>), grd, blk, 0, st, *L, t);
               else hipLaunchKernelGGL((k_relax_gs_front_any<false>), grd, blk, 0, st, *L, t);
    }
#undef GS_CASE
  }
  return 1;
}

// one-launch relax of a small level; returns 0 if the level does not qualify
// mode (red-black with cmatrix='real'): 0 = parallel colour passes (snapshot), 1 = the reference's plane loop bit for bit (rb_exact), 2 = the
// same order by the walk of mgx_rbseq.hip where a kernel has it (k_relax_wave), else the plane loop
// any (option "small_any_nz"): a closed level of at most 1024 columns with nz = 3, 5, 6 or 7 and even nx, ny is served too, and the call then
// returns 2 -- nz = 3 by k_relax_wave where it takes the mode, every other case by k_relax_reg up to 256 columns and by k_relax_small above
// (a 512- or 1024-thread k_relax_reg would have 128 or 64 registers per thread for 16 nz coefficients: the operands are re-read through L2)
int mgxk_relax_small(hipStream_t st, const LevView *L, int nsweeps, int method, int real, Sides ph, int mode, int any) {
  mgx_before_launch();
  const int exact = mode != 0;
  if (any && (L->nz == 3 || (L->nz >= 5 && L->nz <= 7))) {
    const int ncols = L->nx * L->ny;
    if (!(ph.S && ph.E && ph.N && ph.W) || method == 0 || (L->nx & 1) || (L->ny & 1) || ncols > 1024) return 0;
    if (L->nz == 3 && mgxk_relax_wave(st, L, nsweeps, method, real, ph, mode, 1)) return 2;  // not the plane loop of rb_exact, nor the walk of a half-row wider than a wave
    // Declined by measurement (profiles/small_any_nz_time.json): the sequential order at speed where only the plane loop could
    // serve it -- 2 nx barrier steps per sweep with one plane's columns at work lose against the colour pass and its walk, or only draw with
    // them -- except nz = 5 in one wave (8 x 8 x 5: 57-63 us against 98-99 for 3 sweeps); and 'simple' red-black at nz = 6, 7 above 256
    // columns (k_relax_small at 32 x 32 x 7: 961-977 us against 877-901 for 40 sweeps; at nz = 6 a draw)
    if (method == 1 && real && mode == 2 && !(L->nz == 5 && ncols <= 64)) return 0;
    if (method == 1 && !real && L->nz >= 6 && ncols > 256) return 0;
    const size_t bytes = ((size_t)L->nz + 1) * (L->nx + 2) * (L->ny + 2) * sizeof(double);
    const int nth = (ncols + 63) / 64 * 64;
#define ANY_CASE(NZV) case NZV:                                                                                                                \
      if (ncols <= 256) { if (real) hipLaunchKernelGGL((k_relax_reg<NZV, true, 256>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact);   \
                          else hipLaunchKernelGGL((k_relax_reg<NZV, false, 256>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact); }     \
      else { if (real) hipLaunchKernelGGL((k_relax_small<NZV, true, 256>), dim3(1), dim3(256), 0, st, *L, nsweeps, method, ph, exact);                  \
             else hipLaunchKernelGGL((k_relax_small<NZV, false, 256>), dim3(1), dim3(256), 0, st, *L, nsweeps, method, ph, exact); }                    \
      return mgx_launched() ? 2 : 0;
    switch (L->nz) { ANY_CASE(3) ANY_CASE(5) ANY_CASE(6) ANY_CASE(7) default: return 0; }
#undef ANY_CASE
  }
  if (mgxk_relax_wave(st, L, nsweeps, method, real, ph, mode, 0)) return 1;  // <= 256 columns, nz = 2: the whole level in one wave
  {  // one thread per column, coefficients in registers, p in LDS
    const int ncols = L->nx * L->ny;
    const bool closed = ph.S && ph.E && ph.N && ph.W;
    if (!mgx_switches().no_reg && closed && method != 0 && ((L->nz == 2 && ncols <= 1024) || (L->nz == 4 && ncols <= 256))) {
      const size_t bytes = ((size_t)L->nz + 1) * (L->nx + 2) * (L->ny + 2) * sizeof(double);
      const int nth = (ncols + 63) / 64 * 64;
      if (L->nz == 2) { if (real) hipLaunchKernelGGL((k_relax_reg<2, true, 1024>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact);
                        else hipLaunchKernelGGL((k_relax_reg<2, false, 1024>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact); }
      else { if (real) hipLaunchKernelGGL((k_relax_reg<4, true, 256>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact);
             else hipLaunchKernelGGL((k_relax_reg<4, false, 256>), dim3(1), dim3(nth), bytes, st, *L, nsweeps, method, ph, exact); }
      return mgx_launched();
    }
  }
  {  // everything in LDS? (11 arrays of the compact level + the k=1 snapshot)
    const size_t n3 = (size_t)(L->nx + 2) * (L->ny + 2) * L->nz, bytes = (11 * n3 + (size_t)(L->nx + 2) * (L->ny + 2)) * sizeof(double);
    if (!mgx_switches().no_tiny && !(exact && method == 1 && real) && bytes <= 64 * 1024 && (ph.S && ph.E && ph.N && ph.W) && (L->nz == 2 || L->nz == 4)) {
      const int ncolt = method == 2 ? (L->nx / 2) * (L->ny / 2) : L->nx * (L->ny / 2);
      const int ntht = ncolt <= 64 ? 64 : 256;
      if (L->nz == 2) { if (real) hipLaunchKernelGGL((k_relax_tiny<2, true>), dim3(1), dim3(ntht), bytes, st, *L, nsweeps, method, ph);
                        else hipLaunchKernelGGL((k_relax_tiny<2, false>), dim3(1), dim3(ntht), bytes, st, *L, nsweeps, method, ph); }
      else { if (real) hipLaunchKernelGGL((k_relax_tiny<4, true>), dim3(1), dim3(ntht), bytes, st, *L, nsweeps, method, ph);
             else hipLaunchKernelGGL((k_relax_tiny<4, false>), dim3(1), dim3(ntht), bytes, st, *L, nsweeps, method, ph); }
      return mgx_launched();
    }
  }
  const int ncol = method == 2 ? (L->nx / 2) * (L->ny / 2) : L->nx * (L->ny / 2);
  // (Measured and dropped: one cooperative launch per relax call with a grid-wide barrier between colour passes on the
  // 1024-16384-column levels -- cg grid.sync and a hand-written atomic barrier both cost more than the kernel boundary
  // they replace: V-cycle 2.81 -> 3.03 ms.)
  // one CU streams ~25-50 GB/s: worth it only while the level is launch-bound, not bandwidth-bound (measured:
  // 16x16x2 and 32x32x4 win, 64x64x8 loses 2x against separate launches over 256 CUs).  A 2-level-deep coarsest grid
  // is still launch-bound at 1024 columns per colour (the gathered 64x32x2 grid of an 8-GPU run): 1024 threads.
  if (!(ph.S && ph.E && ph.N && ph.W)) return 0;
  if (L->nz == 2 && ncol > 256 && ncol <= 1024) {
    if (real) hipLaunchKernelGGL((k_relax_small<2, true, 1024>), dim3(1), dim3(1024), 0, st, *L, nsweeps, method, ph, exact);
    else hipLaunchKernelGGL((k_relax_small<2, false, 1024>), dim3(1), dim3(1024), 0, st, *L, nsweeps, method, ph, exact);
    return mgx_launched();
  }
  if (ncol > 256 || L->nz > 8) return 0;
  // 32x32x8 (fifth level of an nz = 128 hierarchy), four colours: two colour-pair launches per sweep (k_relax_ks2, 5.9 us each) beat this
  // kernel's 22-32 us per sweep, which re-reads every operand through L2
  if (L->nz == 8 && method == 2 && L->zy != nullptr && ncol > 64 && L->ny / 2 <= WAVE) return 0;
  const int nth = ncol <= 64 ? 64 : 256;
#define SMALL_CASE(NZV) case NZV: if (real) hipLaunchKernelGGL((k_relax_small<NZV, true, 256>), dim3(1), dim3(nth), 0, st, *L, nsweeps, method, ph, exact); \
                                  else hipLaunchKernelGGL((k_relax_small<NZV, false, 256>), dim3(1), dim3(nth), 0, st, *L, nsweeps, method, ph, exact); return mgx_launched();
  switch (L->nz) { SMALL_CASE(2) SMALL_CASE(4) SMALL_CASE(8) default: return 0; }
#undef SMALL_CASE
}

// the nz of the register-resident instances of the colour pass (k_relax_nz): the powers of two, and the vertical sizes that are not (ROMS /
// CROCO users choose nz for their physics) with their coarser levels.  X(nz) once per instance; nz = 80, 96, 128 are mgxk_relax_tall's.
#ifdef MGX_QUICK  // -DMGX_QUICK: only the nz=64 instantiations (resource-usage checks of the level-1 kernel in seconds)
#define REG_NZ_LIST(X) X(64)
#else
#define REG_NZ_LIST(X) X(2) X(4) X(8) X(16) X(32) X(64) X(12) X(20) X(24) X(40) X(48)
#endif

// returns what the pass did (mgx_wrappers.h): PASS_MIRRORS the kernel stored the physical mirrors of p itself (no k_halo_phys needed); PASS_D0 it
// wrote L->d0w; PASS_TALL_STORED it was the stored-coefficient tall-column pass (mgx_relax_tall.hip; relax() counts those)
int mgxk_relax_colour(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  if (const int ks = mgxk_relax_ks(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph)) return ks;  // mid levels: rows split over the waves of a workgroup
  switch (L->nz) {
#define REG_CASE(NZV) case NZV: launch_relax_nz<NZV>(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph); break;
    REG_NZ_LIST(REG_CASE)
#undef REG_CASE
#ifndef MGX_QUICK
    case 80: case 96: case 128: if (const int tall = mgxk_relax_tall(st, L, i0, istep, nplanes, jodd_fixed, rb, real, snap, ph)) return tall;
#endif
    // fall through
    default: {
      dim3 blk(WAVE, 4), grd = col_grid(L->ny / 2, nplanes);
      if (real && snap) hipLaunchKernelGGL((k_relax_colour<true, true>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph);
      else if (real) hipLaunchKernelGGL((k_relax_colour<true, false>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph);
      else hipLaunchKernelGGL((k_relax_colour<false, false>), grd, blk, 0, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph);
      return 0;
    }
  }
  return (real && snap && L->d0w != nullptr) ? PASS_MIRRORS | PASS_D0 : PASS_MIRRORS;
}
// does mgxk_relax_colour run a register-resident kernel (which writes mirrors and chained snapshots) on this level?
int mgxk_has_reg_kernel(const LevView *L) {
  switch (L->nz) {
#define REG_CASE(NZV) case NZV:
    REG_NZ_LIST(REG_CASE) return 1;
#undef REG_CASE
#ifndef MGX_QUICK
    case 80: case 96: case 128: return !mgx_switches().no_tall;  // matrix-free or stored: mgxk_relax_tall has both
#endif
    default: return 0;
  }
}
#undef REG_NZ_LIST
void mgxk_snapshot_k1(hipStream_t st, const LevView *L) {
  hipLaunchKernelGGL(k_snapshot_k1, dim3((L->RS + 255) / 256, L->nx + 2), dim3(256), 0, st, *L);
}

}  // extern "C"
