// z-line smoother for tall columns (nz = 128, BASELINE config 5; 96 and 80 alike): one colour pass, matrix-free cross terms, the lower 64 rows'
// forward values in LDS.  mg_relax.f90:237-305 + :308-334.  Its own translation unit: x and gam of 64 rows stay in registers here
// (500 of 512), it needs a larger `#pragma unroll` budget than the others (Makefile), and the 16-byte pair loads of relax_col_mf
// do not fit next to them (0.8 KB/lane of scratch: PAIR = false); slots 4 / 7 from regenerated zw and the own slopes from regenerated zr do.
#include <cstdlib>

#include "mgx_relax_common.h"

// Tall columns (nz = 128, BASELINE config 5): x and gam of 128 rows do not fit the register file next to the load rings.
// The forward pass is the one of mgx_relax_common.h; only where its values go differs from relax_col_mf.  The forward-eliminated
// values of the lower LOW rows wait in LDS (xf: LOW rows x 64 lanes x 8 B = 32 KB per wave, one wave per SIMD = 128 KB of the
// CU's 160 KB) instead of going out to p and coming back; their gam is rebuilt on the way down from a2(k+1) and bet(k), re-read
// ahead of use (addresses are known: no dependent loads).  x and gam of the upper NZ-LOW rows stay in registers.
// Same expressions, same order: bit-identical to the reference.
template <int NZ, int LOW, bool REAL, bool SNAP, int D, bool ST>
__device__ __forceinline__ void relax_col_mf_tall(const LevView &L, const int i, const int jh, const int jodd, const Sides ph, double *__restrict__ xf) {
  int c, jm, jp;
  COL_POS(L, jh, jodd, c, jm, jp)
  constexpr bool PAIR = false, ZW = true, ZG = true;
  constexpr int UP = NZ - LOW;
  double g0 = 0.0, bet_low_in = 0.0;  // g0 = gam(LOW+1) = a2(LOW+1)*bet(LOW): links the register half to the LDS half
#define MF_G_PUT(kk, v) { if ((kk) > LOW + 1) g[(kk) - LOW - 1] = (v); }
#define MF_X_PUT(kk, v, a2k, betk)                                                   \
  {                                                                                  \
    if ((kk) > LOW) x[(kk) - LOW - 1] = (v); else xf[((kk) - 1) * WAVE + lane] = (v); \
    if ((kk) == LOW + 1) g0 = (a2k) * bet_low_in;                                    \
    if ((kk) == LOW) bet_low_in = (betk);                                            \
  }
  MF_PROLOGUE(UP, UP)
#pragma unroll
  for (int k = 1; k <= LOW; k++) MF_ROW(k)
#pragma unroll
  for (int k = LOW + 1; k <= NZ; k++) MF_ROW(k)
#undef MF_G_PUT
#undef MF_X_PUT
#pragma unroll
  for (int k = UP - 1; k >= 1; k--) x[k - 1] = x[k - 1] - g[k] * x[k];

  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;
  COL_IMAGES(L, i, j, ph)
#define STORE_ROW(k, v) { const long long ro = (long long)((k)-1) * RS; COL_STORE(ST, p, o, ro, c, v) }
  // lower rows, top down: x(k) = xf(k) - gam(k+1)*x(k+1), gam(k+1) = a2(k+1)*bet(k) (mg_relax.f90:325,330).  With the pivots
  // computed in the kernel the downward pass needs bet(k) again: the recurrence only runs upward, so bet(k), k < LOW, is
  // re-read from the array define_matrices left in memory (same bits), together with a2(k+1), DB rows ahead of use.
  constexpr int DB = 8;
  double r_a2[DB], r_bt[DB];
#define LOW_LOAD(q)                                                                                       \
  if ((q) >= 1 && (q) < LOW) {                                                                            \
    const long long ko_ = o + (long long)(LOW - (q)-1) * RS + c;                                          \
    r_a2[(q) % DB] = ld_stream<ST>(a2 + ko_ + RS); r_bt[(q) % DB] = ld_stream<ST>(bet + ko_);           \
  }
#pragma unroll
  for (int q = 1; q < DB; q++) { LOW_LOAD(q) }
#pragma unroll
  for (int k = LOW + 1; k <= NZ; k++) STORE_ROW(k, x[k - LOW - 1])
  double xn = x[0];
#pragma unroll
  for (int q = 0; q < LOW; q++) {  // row LOW - q
    const double gg = q == 0 ? g0 : r_a2[q % DB] * r_bt[q % DB];
    const double xk = xf[(LOW - q - 1) * WAVE + lane] - gg * xn;
    LOW_LOAD(q + DB)
    STORE_ROW(LOW - q, xk)
    xn = xk;
  }
  if (SNAP && L.p1w != nullptr) COL_SNAPSHOT(L, RS, i, c, xn)
#undef LOW_LOAD
#undef STORE_ROW
}

// same launch geometry for the tall-column routine (nz = 128)
template <int NZ, int LOW, bool REAL, bool SNAP, int D, bool ST>
__global__ __launch_bounds__(128, 1) void k_relax_tall(LevView L, int i0, int istep, int nplanes, int jodd_fixed, int rb, Sides ph, int gx) {
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
  extern __shared__ double xf_lds[];  // blockDim.y waves x LOW rows x 64 lanes
  relax_col_mf_tall<NZ, LOW, REAL, SNAP, D, ST>(L, i, jh, jodd, ph, xf_lds + (size_t)threadIdx.y * LOW * WAVE);
}


// nz = 128 (BASELINE config 5), 96 and 80: matrix-free form only, lower 64 rows through memory (relax_col_mf_tall)
extern "C" int mgxk_relax_tall(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  if (L->zy == nullptr || (L->nz != 128 && L->nz != 96 && L->nz != 80)) return 0;
  mgx_before_launch();
  static const bool noxcd = getenv("MGX_NO_XCD") != nullptr, notall = getenv("MGX_NO_TALL") != nullptr;
  if (notall) return 0;
  const int gx0 = (L->ny / 2 + WAVE - 1) / WAVE, gx = noxcd ? -gx0 : gx0;
  const int by = gx0 * nplanes >= 2048 ? 2 : 1;
  dim3 blk(WAVE, by), grd(gx0 * ((nplanes + by - 1) / by));
  const bool stream = (double)L->nx * L->ny * L->nz * 72.0 > 256e6;
  const size_t lds = (size_t)by * 64 * WAVE * sizeof(double);  // the lower 64 rows' forward values: 32 KB per wave
#define LAUNCH_TALL_ONE(NZV, RV, SV, STV)                                                                                \
  {                                                                                                                     \
    static bool attr = false;                                                                                           \
    if (!attr) {                                                                                                        \
      if (hipFuncSetAttribute((const void *)k_relax_tall<NZV, 64, RV, SV, 3, STV>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * WAVE * (int)sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return 0; } \
      attr = true;                                                                                                      \
    }                                                                                                                   \
    hipLaunchKernelGGL((k_relax_tall<NZV, 64, RV, SV, 3, STV>), grd, blk, lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, gx); \
  }
#define LAUNCH_TALL(NZV, STV)                                                                                           \
  {                                                                                                                     \
    if (real && snap) LAUNCH_TALL_ONE(NZV, true, true, STV)                                                             \
    else if (real) LAUNCH_TALL_ONE(NZV, true, false, STV)                                                               \
    else LAUNCH_TALL_ONE(NZV, false, false, STV)                                                                        \
  }
#define LAUNCH_TALL_NZ(NZV) { if (stream) LAUNCH_TALL(NZV, true) else LAUNCH_TALL(NZV, false) }
  if (L->nz == 128) LAUNCH_TALL_NZ(128)
  else if (L->nz == 96) LAUNCH_TALL_NZ(96)
  else LAUNCH_TALL_NZ(80)
#undef LAUNCH_TALL_NZ
#undef LAUNCH_TALL
#undef LAUNCH_TALL_ONE
  return mgx_launched();
}
