// Down leg of a held pair in one kernel (options "hold_z_levels", "hold_odd_nz": the coarse level has the fine level's nz and half its nx, ny):
// the residual r = b - A p of the fine level (mg_relax.f90:421-515) and its 2-D restriction row by row (fine2coarse_2D, mg_intergrids.f90:121),
// without r ever being written.  Separately the two operators are mgxk_residual and k_fine2coarse_held (mgx_hold.hip), which write the
// fine r and read it back; under "hold_z_levels" the pair of levels 1 and 2 is held, and that r is the largest array of the cycle.
//
// The operator is the ONE text of mgx_operator.h, the columns k_residual and k_residual_mf expand: OP_COLUMN_MF where the level has its
// slopes, OP_COLUMN on the stored slots otherwise (bmask, a user matrix, MGX_NO_MF) -- every row's r has the bits of compute_residual.
// What differs is the sink and the lane map.  The four fine columns of coarse column (j2, i2) are entry j2 - 1 of the odd and of the even
// half-row of planes iA = 2 i2 - 1 and iB = 2 i2: a wave holds them for 16 coarse columns, lanes 0-15 (iA, odd j), 16-31 (iB, odd j), 32-47
// (iA, even j), 48-63 (iB, even j) -- four 128-byte runs per request -- so a row's sum is closed inside the wave by three shuffles, in the
// order of k_fine2coarse_held, r(j,i) + r(j,i+1) + r(j+1,i) + r(j+1,i+1) left to right: b_c has the bits of the two launches.  A workgroup
// is four waves = four coarse planes.  Rows are independent in a held pair, so an odd nz would be served as well; the choice declines it
// (choose_resrest_held, mgx_choice_transfer.h).
// NORM: also the sum of r^2 over the workgroup's fine cells, as a pair -> partial[block], partial[nblocks + block]: the closing
// compute_residual of a solve_p iteration on a held pair of levels 1 and 2 (residual_closing, mgx_cycle.cpp).  The pair is rounded once
// (dd_add, mgx_device.h), summed in another order than k_residual's.
// dup / zero: a second destination of the sums and the array to clear, with their physical images, as in k_fine2coarse_held.
#include "mgx_switches.h"
#include "mgx_operator.h"

#define HELD_RHS(ko) b[ko]
#define HELD_RHS_MF(ko) ld_rt(b + ko, stream)
// a row of the column: into the norm, then the four columns' values meet in the lane of (iA, odd j), which stores the coarse row
#define HELD_SINK(ro, ko, rr)                                                                                                \
  {                                                                                                                          \
    if (NORM && live) dd_add(acc, acl, rr * rr);                                                                             \
    const double s1_ = __shfl_down(rr, 16, 64), s2_ = __shfl_down(rr, 32, 64), s3_ = __shfl_down(rr, 48, 64);                \
    if (q == 0 && live) {                                                                                                    \
      const double z = rr + s1_ + s2_ + s3_;                                                                                 \
      dst[oc + rc] = z;                                                                                                      \
      mirror_store(C, dst, rc, j2, i2, cc, z, ph);                                                                           \
      if (dup) { dup[oc + rc] = z; mirror_store(C, dup, rc, j2, i2, cc, z, ph); }                                            \
      if (zero) { zero[oc + rc] = 0.0; mirror_store(C, zero, rc, j2, i2, cc, 0.0, ph); }                                     \
    }                                                                                                                        \
    rc += C.RS;                                                                                                              \
  }

// grid: (coarse columns / 16, coarse planes / 4); block: (64, 4).  L is the fine level (the operator texts call it so), C the coarse one
// or the pre-gather block; `dst` its b.
template <bool MF, bool REAL, bool NORM>
__global__ __launch_bounds__(256) void k_residual_restrict_held(LevView L, LevView C, double *__restrict__ dst, Sides ph, double *__restrict__ zero,
                                                                double *__restrict__ partial, double *__restrict__ dup, int stream) {
  const int q = threadIdx.x >> 4;                       // 0: (iA, odd j), 1: (iB, odd j), 2: (iA, even j), 3: (iB, even j)
  int j2 = 1 + blockIdx.x * CH_HELD_COLS + (threadIdx.x & 15);
  const int i2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  const bool live = j2 <= C.ny;
  if (!live) j2 = C.ny;                                  // ragged chunk: dead lanes shadow a live column (they take part in the shuffles), store and sum nothing
  double acc = 0.0, acl = 0.0;                           // the sum of r^2 as a pair (dd_add, mgx_device.h)
  if (i2 <= C.nx) {                                      // wave-uniform
    const int i = 2 * i2 - 1 + (q & 1), jh = j2 - 1, jodd = q < 2;
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const double *__restrict__ b = L.b;
    const int cc = jpos(C, j2);
    const long long oc = (long long)i2 * C.plane + cc;
    long long rc = 0;                                    // the coarse row's offset: the sink is called for k = 1 .. nz in order
    if constexpr (MF) OP_COLUMN_MF(OP_P, OP_P2, HELD_RHS_MF, HELD_SINK)
    else OP_COLUMN(OP_P, HELD_RHS, HELD_SINK)
  }
  if (!NORM) return;
  OP_BLOCK_SUM_DD(acc, acl, partial, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y)
}

extern "C" {

// workgroups (= pairs of norm partials) of the launch below, for a caller that sums r^2
int mgxk_residual_restrict_held_grid(const LevView *F, const LevView *C) { return (int)choose_resrest_held(lev_shape(F), lev_shape(C), 1, true, mgx_switches()).grid; }
// returns 1 when launched (choose_resrest_held, mgx_choice_transfer.h), 0 = use mgxk_residual + mgxk_fine2coarse_held
// partial != nullptr: also sum r^2 (room for twice mgxk_residual_restrict_held_grid()); dup: second destination of the coarse sums
int mgxk_residual_restrict_held(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero, double *partial, double *dup) {
  mgx_before_launch();
  const HeldRrChoice c = choose_resrest_held(lev_shape(F), lev_shape(C), real, partial != nullptr, mgx_switches());
  if (!c.served) return 0;
  with_bool(c.mf, [&](auto MF) {
    with_bool(c.real, [&](auto REAL) {
      with_bool(c.norm, [&](auto NORM) {
        hipLaunchKernelGGL((k_residual_restrict_held<MF(), REAL(), NORM()>), dim3(c.gx, c.gy), dim3(WAVE, 4), 0, st, *F, *C, dst, ph, zero, partial, dup, c.stream);
      });
    });
  });
  return mgx_launched();
}

}  // extern "C"
