// The operator's kernels of the multigrid cycle for gfx950 (MI355X): residual, norms and inner products.  Hand-written, fp64, bandwidth-bound stencils.
//
// All arithmetic keeps the reference's operation order and is compiled with -ffp-contract=off, so a
// colour pass of the four-colour smoother, the residual and the transfers are bit-identical to the
// reference's CPU loops (only reductions differ in summation order).
//
// Thread mapping everywhere: one lane = one (j,i) column, lanes run along the unit-stride half-row of
// the JS layout (mgx_internal.h), so every global access of a wave is one contiguous 512-byte run.
#include "mgx_operator.h"

// ------------------------------------------------------------------------------------------------
// residual r = b - A p on the interior and per-block partial sums of r^2.  mg_relax.f90:421-515: the column of mgx_operator.h with
// the right-hand side b; a row goes to r with its physical images and into the norm.
// 1-D grid of gx * gy * 2 blocks (op_block_map): bz = 0 handles the odd-j half-rows, bz = 1 the even-j ones.
// ------------------------------------------------------------------------------------------------
#define RES_RHS(ko) b[ko]
#define RES_SINK(ro, ko, rr) { r[ko] = rr; mirror_store(L, r, ro, jcol, i, c, rr, ph); dd_add(acc, acl, rr * rr); }
template <bool REAL>
__global__ __launch_bounds__(256) void k_residual(LevView L, double *__restrict__ partial, int want_norm, int gx, int gy, Sides ph, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc = 0.0, acl = 0.0;  // the sum of r^2 as a pair (dd_add, mgx_device.h)
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const double *__restrict__ b = L.b;
    double *__restrict__ r = L.r;
    OP_COLUMN(OP_P, RES_RHS, RES_SINK)
  }
  if (!want_norm) return;
  OP_BLOCK_SUM_DD(acc, acl, partial, blockIdx.x, gridDim.x)
}

// residual with matrix-free cross terms (OP_COLUMN_MF, mgx_operator.h): b and r of a level that does not fit the caches are streamed past them
#define RES_RHS_MF(ko) ld_rt(b + ko, stream)
#define RES_SINK_MF(ro, ko, rr) { st_rt(r + ko, rr, stream); mirror_store(L, r, ro, jodd ? 2 * jh + 1 : 2 * jh + 2, i, c, rr, ph); dd_add(acc, acl, rr * rr); }
template <bool REAL>
__global__ __launch_bounds__(256) void k_residual_mf(LevView L, double *__restrict__ partial, int want_norm, int gx, int gy, Sides ph, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc = 0.0, acl = 0.0;  // the sum of r^2 as a pair (dd_add, mgx_device.h)
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const double *__restrict__ b = L.b;
    double *__restrict__ r = L.r;
    OP_COLUMN_MF(OP_P, OP_P2, RES_RHS_MF, RES_SINK_MF)
  }
  if (!want_norm) return;
  OP_BLOCK_SUM_DD(acc, acl, partial, blockIdx.x, gridDim.x)
}

// sum of squares of the interior of a JS field (bnorm of solve_p, mg_solvers.f90:50)
__global__ __launch_bounds__(256) void k_sumsq(LevView L, const double *__restrict__ a, double *__restrict__ partial) {
  const int jh = blockIdx.x * WAVE + threadIdx.x;
  const int i = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  double acc = 0.0;
  if (jh < (L.ny >> 1) && i <= L.nx) {
    const int c = blockIdx.z == 0 ? L.HO + jh : L.EO + jh + 1;
    const long long o = (long long)i * L.plane + c;
    for (int k = 0; k < L.nz; k++) { const double v = a[o + (long long)k * L.RS]; acc += v * v; }
  }
  OP_BLOCK_SUM(acc, partial, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x)
}

// inner product of the interiors of two JS fields (norm(lev,x,y), mg_solvers.f90:180-200)
__global__ __launch_bounds__(256) void k_dot(LevView L, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ partial) {
  const int jh = blockIdx.x * WAVE + threadIdx.x;
  const int i = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  double acc = 0.0;
  if (jh < (L.ny >> 1) && i <= L.nx) {
    const int c = blockIdx.z == 0 ? L.HO + jh : L.EO + jh + 1;
    const long long o = (long long)i * L.plane + c;
    for (int k = 0; k < L.nz; k++) acc += a[o + (long long)k * L.RS] * b[o + (long long)k * L.RS];
  }
  OP_BLOCK_SUM(acc, partial, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x)
}

// second stage: one block sums the partials in index order -> out[0]
__global__ __launch_bounds__(256) void k_reduce_partials(const double *__restrict__ partial, int n, double *__restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int q = threadIdx.x; q < n; q += 256) s += partial[q];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// second stage of a sum whose n partials are pairs (dd_add, mgx_device.h: hi at partial[q], lo at partial[n + q]) -> out[0], rounded once
__global__ __launch_bounds__(256) void k_reduce_partials_dd(const double *__restrict__ partial, int n, double *__restrict__ out) {
  __shared__ double red[512];
  double s = 0.0, sl = 0.0;
  for (int q = threadIdx.x; q < n; q += 256) dd_merge(s, sl, partial[q], partial[n + q]);
  red[threadIdx.x] = s; red[256 + threadIdx.x] = sl;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      dd_merge(s, sl, red[threadIdx.x + off], red[256 + threadIdx.x + off]);
      red[threadIdx.x] = s; red[256 + threadIdx.x] = sl;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s + sl;
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
extern "C" {

int mgxk_residual_nblocks(const LevView *L) { return (int)choose_operator(lev_shape(L)).grid; }
void mgxk_residual(hipStream_t st, const LevView *L, double *partial, double *out, int real, int want_norm, Sides ph) {
  const OpChoice c = choose_operator(lev_shape(L));
  op_launch(c, real, [&](auto MF, auto REAL) {
    if constexpr (MF()) hipLaunchKernelGGL((k_residual_mf<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, partial, want_norm, c.gx, c.gy, ph, c.stream);
    else hipLaunchKernelGGL((k_residual<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, partial, want_norm, c.gx, c.gy, ph, c.stream);
  });
  if (want_norm) hipLaunchKernelGGL(k_reduce_partials_dd, dim3(1), dim3(256), 0, st, partial, (int)c.grid, out);
}
// second stage of a norm whose partials another kernel wrote (one pair per workgroup: the fused residual + restriction, mgx_resrest.hip)
void mgxk_reduce(hipStream_t st, const double *partial, int n, double *out) { hipLaunchKernelGGL(k_reduce_partials_dd, dim3(1), dim3(256), 0, st, partial, n, out); }
void mgxk_sumsq(hipStream_t st, const LevView *L, const double *a, double *partial, double *out) {
  dim3 blk(WAVE, 4), grd = col_grid(L->ny / 2, L->nx, 2);
  hipLaunchKernelGGL(k_sumsq, grd, blk, 0, st, *L, a, partial);
  hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, partial, (int)(grd.x * grd.y * grd.z), out);
}
void mgxk_dot(hipStream_t st, const LevView *L, const double *a, const double *b, double *partial, double *out) {
  dim3 blk(WAVE, 4), grd = col_grid(L->ny / 2, L->nx, 2);
  hipLaunchKernelGGL(k_dot, grd, blk, 0, st, *L, a, b, partial);
  hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, partial, (int)(grd.x * grd.y * grd.z), out);
}

}  // extern "C"
