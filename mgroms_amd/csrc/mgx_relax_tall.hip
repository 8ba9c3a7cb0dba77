// z-line smoother for tall columns (nz = 128, BASELINE config 5; 96 and 80 alike): one colour pass, the lower 64 rows' forward values in
// LDS.  mg_relax.f90:237-305 + :308-334.  Two forms of one frame: matrix-free cross terms (relax_col_mf_tall: the matrix came from
// define_matrices without a mask) and stored coefficients (relax_col_st_tall: bmask, a user matrix, MGX_NO_MF).  Its own translation
// unit: x and gam of 64 rows stay in registers here (matrix-free: 500 of 512), it needs a larger `#pragma unroll` budget than the others
// (Makefile), and the 16-byte pair loads of relax_col_mf do not fit next to them (0.8 KB/lane of scratch: PAIR = false); slots 4 / 7 from
// regenerated zw and the own slopes from regenerated zr do.
// The forward rows of both forms are the shared texts of mgx_relax_common.h (MF_ROW with relax_col_mf, SC_ROW with relax_col_nz: the
// instances of mgx_relax.hip compile to the instructions they had before the stored text was shared); the way down is TALL_DOWN below.
#include "mgx_switches.h"
#include "mgx_relax_common.h"
#include "mgx_choice.h"

// Tall columns (nz = 128, BASELINE config 5): x and gam of 128 rows do not fit the register file next to the load rings.
// The forward pass is the one of mgx_relax_common.h; only where its values go differs from relax_col_mf / relax_col_nz.  The
// forward-eliminated values of the lower LOW rows wait in LDS (xf: LOW rows x 64 lanes x 8 B = 32 KB per wave, one wave per SIMD = 128 KB
// of the CU's 160 KB) instead of going out to p and coming back; their gam is rebuilt on the way down from a2(k+1) and bet(k), re-read
// ahead of use (addresses are known: no dependent loads).  x and gam of the upper NZ-LOW rows stay in registers.
// The rows expand ROW_RHS_* (mgx_device.h) through MF_ROW / SC_ROW: bit-identical to the reference.
//
// TALL_DOWN: the way down of both forms.  In scope: NZ, LOW, UP, SNAP, ST; L, i, jh, jodd, ph, c, o, RS, p, a2, bet, lane, xf; x[UP], g[UP]
// of the upper rows after the forward pass and g0 = gam(LOW+1).
// Lower rows, top down: x(k) = xf(k) - gam(k+1)*x(k+1), gam(k+1) = a2(k+1)*bet(k) (mg_relax.f90:325,330).  The pivot recurrence only
// runs upward, so bet(k), k < LOW, is re-read from the array the set-up left in memory (the matrix-free pass computed the same bits),
// together with a2(k+1), DB rows ahead of use.
#define TALL_STORE_ROW(OD, k, v) { const long long ro = (long long)((k)-1) * RS; COL_STORE(ST, p, OD, ro, c, v) }
#define TALL_LOW_LOAD(OD, q)                                                                                \
  if ((q) >= 1 && (q) < LOW) {                                                                            \
    const long long ko_ = OD + (long long)(LOW - (q)-1) * RS + c;                                         \
    r_a2[(q) % DB] = ld_stream<ST>(a2 + ko_ + RS); r_bt[(q) % DB] = ld_stream<ST>(bet + ko_);             \
  }
#define TALL_DOWN(OD)                                                                                     \
  _Pragma("unroll") for (int k = UP - 1; k >= 1; k--) x[k - 1] = x[k - 1] - g[k] * x[k];                  \
  const int j = jodd ? 2 * jh + 1 : 2 * jh + 2;                                                           \
  COL_IMAGES(L, i, j, ph)                                                                                 \
  constexpr int DB = 8;                                                                                   \
  double r_a2[DB], r_bt[DB];                                                                              \
  _Pragma("unroll") for (int q = 1; q < DB; q++) { TALL_LOW_LOAD(OD, q) }                                 \
  _Pragma("unroll") for (int k = LOW + 1; k <= NZ; k++) TALL_STORE_ROW(OD, k, x[k - LOW - 1])             \
  double xn = x[0];                                                                                       \
  _Pragma("unroll") for (int q = 0; q < LOW; q++) {  /* row LOW - q */                                    \
    const double gg = q == 0 ? g0 : r_a2[q % DB] * r_bt[q % DB];                                          \
    const double xk = xf[(LOW - q - 1) * WAVE + lane] - gg * xn;                                          \
    TALL_LOW_LOAD(OD, q + DB)                                                                             \
    TALL_STORE_ROW(OD, LOW - q, xk)                                                                       \
    xn = xk;                                                                                              \
  }                                                                                                       \
  if (SNAP && L.p1w != nullptr) COL_SNAPSHOT(L, RS, i, c, xn)

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
  TALL_DOWN(o)
}

// Stored coefficients: slots 2-8 and the pivots bet as they lie in memory (SC_ROW, mgx_relax_common.h), nothing regenerated -- 19 load
// streams per row instead of the matrix-free pass's 12, no generator state, hence the same look-ahead in fewer registers.
template <int NZ, int LOW, bool REAL, bool SNAP, int D, bool ST>
__device__ __forceinline__ void relax_col_st_tall(const LevView &L, const int i, const int jh, const int jodd, const Sides ph, double *__restrict__ xf) {
  int c, jm, jp;
  COL_POS(L, jh, jodd, c, jm, jp)
  constexpr int UP = NZ - LOW;
  const int lane = threadIdx.x;
  double g0 = 0.0;  // gam(LOW+1) = a2(LOW+1)*bet(LOW): links the register half to the LDS half
#define SC_G_PUT(kk, v) { if ((kk) > LOW + 1) g[(kk) - LOW - 1] = (v); else if ((kk) == LOW + 1) g0 = (v); }
#define SC_X_PUT(kk, v) { if ((kk) > LOW) x[(kk) - LOW - 1] = (v); else xf[((kk) - 1) * WAVE + lane] = (v); }
  SC_PROLOGUE(UP, UP)
#pragma unroll
  for (int k = 1; k <= LOW; k++) SC_ROW(k)
#pragma unroll
  for (int k = LOW + 1; k <= NZ; k++) SC_ROW(k)
#undef SC_G_PUT
#undef SC_X_PUT
  // The way down addresses the rows the forward pass loaded (a2, bet): left to itself the compiler keeps those 128 addresses alive
  // across the upper rows (0.8 KB/lane of scratch at NZ = 128).  An opaque copy of the plane offset makes it form them again.
  long long od = o;
  asm volatile("" : "+v"(od));
  TALL_DOWN(od)
}

// the launch geometry of k_relax_nz for the two tall-column routines: one text, two kernels (the matrix-free one keeps its name)
#define TALL_KERNEL(NAME, COLUMN)                                                                                        \
  template <int NZ, int LOW, bool REAL, bool SNAP, int D, bool ST>                                                      \
  __global__ __launch_bounds__(128, 1) void NAME(LevView L, int i0, int istep, int nplanes, int jodd_fixed, int rb, Sides ph, int gx) { \
    const int npair = (nplanes + blockDim.y - 1) / blockDim.y;                                                          \
    int bx, ipr;  /* j-chunk, plane pair */                                                                             \
    XCD_BLOCK_MAP(npair, gx, bx, ipr)                                                                                   \
    const int ipl = ipr * blockDim.y + threadIdx.y;                                                                     \
    const int jh = bx * WAVE + threadIdx.x;                                                                             \
    if (jh >= (L.ny >> 1) || ipl >= nplanes) return;                                                                    \
    const int i = i0 + istep * ipl;                                                                                     \
    /* RB: j = 1+mod(i+rb,2),ny,2 (mg_relax.f90:174) ; FC: fixed parity (:216-217) */                                   \
    const int jodd = jodd_fixed >= 0 ? jodd_fixed : (((i + rb) & 1) == 0);                                              \
    if (sides_part_skip(ph, i, L.nx, jodd, bx, gx)) return;  /* wave-uniform */                                         \
    extern __shared__ double xf_lds[];  /* blockDim.y waves x LOW rows x 64 lanes */                                    \
    COLUMN<NZ, LOW, REAL, SNAP, D, ST>(L, i, jh, jodd, ph, xf_lds + (size_t)threadIdx.y * LOW * WAVE);                  \
  }
TALL_KERNEL(k_relax_tall, relax_col_mf_tall)
TALL_KERNEL(k_relax_tall_st, relax_col_st_tall)
#undef TALL_KERNEL

// one instance of either kernel: its LDS (two waves' worth, above the 64 KB a kernel gets without asking) is granted once; false = refused
template <auto KERNEL>
static bool launch_tall_one(hipStream_t st, const LevView *L, const Choice &c, int i0, int istep, int nplanes, int jodd_fixed, int rb, Sides ph) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * WAVE * (int)sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return false; }
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(c.grid), dim3(c.bx, c.by), c.lds, st, *L, i0, istep, nplanes, jodd_fixed, rb, ph, c.gx);
  return true;
}

// The tall-column pass of choose_tall (mgx_choice.h).  Returns 0 = nothing ran (the caller's generic column takes the pass), PASS_MIRRORS = the
// matrix-free pass ran (the physical mirrors are written), with PASS_TALL_STORED the stored one.
extern "C" int mgxk_relax_tall(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph) {
  mgx_before_launch();
  const Choice c = choose_tall(lev_shape(L), nplanes, mgx_switches());
  if (c.family == KF_NONE) return 0;
  bool ok = false;
  with_nz<128, 96, 80>(c.nz, [&](auto N) {
    with_bool(c.stream, [&](auto T) {
      with_real_and(real, snap, [&](auto R, auto S) {
        constexpr int NZ = decltype(N)::value, TALL_D = 3;  // choose_tall's d
        constexpr bool REAL = decltype(R)::value, SNAP = decltype(S)::value, ST = decltype(T)::value;
        if (c.mf) ok = launch_tall_one<k_relax_tall<NZ, 64, REAL, SNAP, TALL_D, ST>>(st, L, c, i0, istep, nplanes, jodd_fixed, rb, ph);
        else ok = launch_tall_one<k_relax_tall_st<NZ, 64, REAL, SNAP, TALL_D, ST>>(st, L, c, i0, istep, nplanes, jodd_fixed, rb, ph);
      });
    });
  });
  return ok && mgx_launched() ? c.ret : 0;
}
