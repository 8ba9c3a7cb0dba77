// Transfers of a held pair (option "hold_odd_nz"): the fine and the coarse level have the same nz and the pair coarsens in x and y only.  They
// are the reference's 2-D operators (mg_intergrids.f90: fine2coarse_2D with a 2-D x, coarse2fine_2D_linear, coarse2fine_2D_nearest) applied
// to every row k, in the reference's order of operations: with -ffp-contract=off comparable bit for bit with the same loops on the CPU.
// Rows are independent; lanes run along j.  In the JS layout the fine columns j = 2 j2 - 1 and j + 1 of coarse column j2 are entry j2 - 1 of the
// odd and of the even half-row, so both are unit-stride across a wave.  Physical sides get their mirrors from the lane that owns the cell
// (mirror_store); open sides (rank seams, periodic sides) are the caller's halo fill.  Held pairs are small levels (the first one of
// 512 x 512 x 40 is 64 x 64 x 5 -> 32 x 32 x 5): one lane per coarse cell, no cache hints, no look-ahead.
#include "mgx_device.h"

// restriction: b_c(k,j2,i2) = r(k,j,i) + r(k,j,i+1) + r(k,j+1,i) + r(k,j+1,i+1), left to right (mg_intergrids.f90:121).
// `dst` is the coarse b, or the pre-gather block when the coarse level is gathered; dup / zero as in k_fine2coarse (closed levels only).
__global__ __launch_bounds__(256) void k_fine2coarse_held(LevView F, LevView C, double *__restrict__ dst, Sides ph, double *__restrict__ dup, double *__restrict__ zero) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int i2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  const int k = 1 + blockIdx.z;
  if (j2 > C.ny || i2 > C.nx || k > C.nz) return;
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j = 2*j2-1 (odd) and 2*j2 (even)
  const double *__restrict__ x = F.r;
  const long long o0 = (long long)i * F.plane + (long long)(k - 1) * F.RS, o1 = o0 + F.plane;
  const long long rc = (long long)(k - 1) * C.RS, oc = (long long)i2 * C.plane + rc + jpos(C, j2);
  const double z = x[o0 + po] + x[o1 + po] + x[o0 + pe] + x[o1 + pe];
  dst[oc] = z;
  mirror_store(C, dst, rc, j2, i2, jpos(C, j2), z, ph);
  if (dup) { dup[oc] = z; mirror_store(C, dup, rc, j2, i2, jpos(C, j2), z, ph); }
  if (zero) { zero[oc] = 0.0; mirror_store(C, zero, rc, j2, i2, jpos(C, j2), 0.0, ph); }
}

// prolongation + correction: fine r = interp(coarse p) row by row; fine p += fine r (interior and physical images).
// LIN: the four bilinear expressions of coarse2fine_2D_linear (mg_intergrids.f90:317-328), reading the coarse halo; else the four copies of
// coarse2fine_2D_nearest (:268-271).  WR, SK: as in k_coarse2fine_run (keep_r, skip1).  `xc` is the coarse p (or the split block).
template <bool WR, bool SK, bool LIN>
__global__ __launch_bounds__(256) void k_coarse2fine_held(LevView F, LevView C, const double *__restrict__ xc, Sides ph) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int k = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  const int i2 = 1 + blockIdx.z;
  if (j2 > C.ny || k > C.nz || i2 > C.nx) return;
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j (odd) and j+1 (even)
  const long long rf_ = (long long)(k - 1) * F.RS, rc = (long long)(k - 1) * C.RS;
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  const long long q0 = (long long)i2 * C.plane + rc, qm = q0 - C.plane, qp = q0 + C.plane;
  const int c0 = jpos(C, j2), cm = jpos(C, j2 - 1), cp = jpos(C, j2 + 1);
  double *__restrict__ rf = F.r;
  double *__restrict__ pf = F.p;
  const bool edge0 = (ph.S && j2 == 1) || (ph.W && i2 == 1);  // SK: the (i odd, j odd) column of this lane is read through a mirror
  // fine cell Q of the 2x2 block: bit 1 = plane i+1, bit 0 = column j+1 (Q = 0 is the first colour's column)
#define PUT(Q, val) if (!(SK && (Q) == 0) || edge0) { const long long OO_ = ((Q) & 2) ? o1 : o0; const int PP_ = ((Q) & 1) ? pe : po;    \
    const long long t_ = OO_ + rf_ + PP_; const double v_ = (val), w_ = pf[t_] + v_;                                                    \
    if (WR) rf[t_] = v_; pf[t_] = w_;                                                                                                   \
    const int jf_ = ((Q) & 1) ? 2 * j2 : 2 * j2 - 1, if_ = ((Q) & 2) ? i + 1 : i;                                                        \
    if (WR) mirror_store(F, rf, rf_, jf_, if_, PP_, v_, ph); mirror_store(F, pf, rf_, jf_, if_, PP_, w_, ph); }
  const double x00 = xc[q0 + c0];
  if (LIN) {
    // first letter: the column (j2-1, j2, j2+1), second: the plane (i2-1, i2, i2+1)
    const double xmm = xc[qm + cm], x0m = xc[qm + c0], xpm = xc[qm + cp], xm0 = xc[q0 + cm], xp0 = xc[q0 + cp], xmp = xc[qp + cm], x0p = xc[qp + c0], xpp = xc[qp + cp];
    const double a = 9. / 16., b = 3. / 16., c = 1. / 16.;
    PUT(0, +a * x00 + c * xmm + b * xm0 + b * x0m);
    PUT(1, +a * x00 + c * xpm + b * xp0 + b * x0m);
    PUT(2, +a * x00 + c * xmp + b * xm0 + b * x0p);
    PUT(3, +a * x00 + c * xpp + b * xp0 + b * x0p);
  } else {
    PUT(0, x00); PUT(1, x00); PUT(2, x00); PUT(3, x00);
  }
#undef PUT
}

extern "C" {

void mgxk_fine2coarse_held(hipStream_t st, const LevView *F, const LevView *C, double *dst, Sides ph, double *dup, double *zero) {
  hipLaunchKernelGGL(k_fine2coarse_held, col_grid(C->ny, C->nx, C->nz), dim3(WAVE, 4), 0, st, *F, *C, dst, ph, dup, zero);
}

// skip1: the caller guarantees that a four-colour relax of the fine level follows (cycles only; see k_coarse2fine_run, SK)
void mgxk_coarse2fine_held(hipStream_t st, const LevView *F, const LevView *C, const double *src, int linear, Sides ph, int keep_r, int skip1) {
  const C2fChoice c = choose_coarse2fine_held(lev_shape(F), lev_shape(C), linear, keep_r, skip1);
  with_bool(c.run, [&](auto LIN) {
    with_wr_sk(c.wr, c.sk, [&](auto WR, auto SK) {
      hipLaunchKernelGGL((k_coarse2fine_held<WR(), SK(), LIN()>), dim3(c.gx, c.gy, c.gz), dim3(WAVE, c.by), 0, st, *F, *C, src, ph);
    });
  });
}

}  // extern "C"
