// The matrices from the caller's own vertical grid (mgx_matrices_depths*, mgx_update_depths_device of include/mgx.h): the kernels that stand
// where k_zr_zw and the coarsening of h and zeta stand when the library evaluates its own stretching.  The depths of level 1 come in from the
// caller's arrays (k_depths_in: the model's i-fastest padded arrays; k_depths_copy: the library's dense layout), every coarser level's depths
// are averages of the finer level's (k_depths_coarsen, the rule of DESIGN.md 6.4), and h, zeta of every level are read off its zw
// (k_depths_hz).  All work in the reference layout of mgx_setup.hip, zr(nz, -1:ny+2, -1:nx+2) and zw(nz+1, -1:ny+2, -1:nx+2), k fastest, and
// touch interior columns only: halos are the halo fills' (rl_fill_halo, nh = 2).  The launches are chosen in mgx_choice_depths.h.
#include "mgx_internal.h"
#include "mgx_choice_depths.h"

// column (j, i), 1-based interior numbering, of a reference-layout array with two halo cells per side: its offset in columns
__device__ __forceinline__ long long dcol(int j, int i, int ny) { return (long long)(i + 1) * (ny + 4) + (j + 1); }

// One level pair, both arrays, one launch.  Lanes run along the coarse k (as KCOL_THREAD of mgx_setup.hip): a wave reads whole k-runs of the
// four fine columns and writes whole k-runs of the coarse one.  The lane of coarse interface kc = 1..nzc+1 writes zw_C(kc) and, for kc <= nzc,
// zr_C(kc).  avg = 0.25 * (x(fj,fi) + x(fj+1,fi) + x(fj,fi+1) + x(fj+1,fi+1)) in that order, the order of k_coarsen2d.
//   halving (nzc = nzf / 2, nzf even): zw_C(kc) = avg zw_F(2kc-1), zr_C(kc) = avg zw_F(2kc) -- only zw_F is read, its entries 2kc-1 and 2kc a
//   pair of adjacent doubles per lane (8-byte loads: a column of nzf+1 doubles has no wider alignment)
//   HELD (nzc = nzf): zw_C(k) = avg zw_F(k), zr_C(k) = avg zr_F(k)
// The coarse column (J, I) lands at column (I + oj) * ow + (J + oj) of the outputs: oj = 1, ow = nyc + 4 is the level's own array, oj = -1,
// ow = nyc the packed interior block a gathered level sends (k fastest, then j, then i: the buffer order of k_rect's pack).
template <bool HELD>
__global__ __launch_bounds__(256) void k_depths_coarsen(const double *__restrict__ zrf, const double *__restrict__ zwf, double *__restrict__ zrc,
                                                        double *__restrict__ zwc, int nyf, int nzf, int nxc, int nyc, int nzc, int oj, int ow) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned nk = (unsigned)(nzc + 1), c = t / nk;
  const int kc = 1 + (int)(t - c * nk);
  const unsigned ci = c / (unsigned)nyc;
  const int J = 1 + (int)(c - ci * (unsigned)nyc), I = 1 + (int)ci;
  if (I > nxc) return;
  const int fj = 2 * J - 1, fi = 2 * I - 1;
  const long long c00 = dcol(fj, fi, nyf), c10 = c00 + 1, c01 = c00 + (nyf + 4), c11 = c01 + 1;
  const long long oc = (long long)(I + oj) * ow + (J + oj);
  const long long nw = nzf + 1;
  if (HELD) {
    const int k = kc - 1;
    zwc[oc * (nzc + 1) + k] = 0.25 * (zwf[c00 * nw + k] + zwf[c10 * nw + k] + zwf[c01 * nw + k] + zwf[c11 * nw + k]);
    if (kc <= nzc) zrc[oc * nzc + k] = 0.25 * (zrf[c00 * nzf + k] + zrf[c10 * nzf + k] + zrf[c01 * nzf + k] + zrf[c11 * nzf + k]);
  } else {
    const int a = 2 * kc - 2;   // zw_F(2kc-1), 0-based; a <= nzf, and a + 1 <= nzf while kc <= nzc
    zwc[oc * (nzc + 1) + (kc - 1)] = 0.25 * (zwf[c00 * nw + a] + zwf[c10 * nw + a] + zwf[c01 * nw + a] + zwf[c11 * nw + a]);
    if (kc <= nzc) zrc[oc * nzc + (kc - 1)] = 0.25 * (zwf[c00 * nw + a + 1] + zwf[c10 * nw + a + 1] + zwf[c01 * nw + a + 1] + zwf[c11 * nw + a + 1]);
  }
}

// The model's arrays into level 1: z(i,j,k) = src[(i-1) + (j-1) sj + dk sk], i fastest, to the interior of zr / zw, k fastest.  An LDS-tiled
// transpose of (i, k) tiles, row by row in j: lanes run along i for the loads and along k for the stores, 512-byte runs on both sides; tile
// rows of DEPTHS_TILE + 1 doubles against bank conflicts.  Both arrays in one launch: blockIdx.x counts the k tiles of zr, then those of zw,
// each ti times (the i tiles).  Only i = 1..nx, j = 1..ny, the nz (zr) or nz + 1 (zw) levels are read; only those elements are written.
__global__ __launch_bounds__(256) void k_depths_in(const double *__restrict__ zr, const double *__restrict__ zw, long long rsj, long long rsk,
                                                   long long wsj, long long wsk, double *__restrict__ dzr, double *__restrict__ dzw, int nx, int ny,
                                                   int nz, int ti, int ktr) {
  __shared__ double tile[DEPTHS_TILE][DEPTHS_TILE + 1];
  const int bt = blockIdx.x / ti, it = blockIdx.x - bt * ti;
  const bool w = bt >= ktr;
  const int k0 = (w ? bt - ktr : bt) * DEPTHS_TILE, i0 = it * DEPTHS_TILE;
  const int nzz = w ? nz + 1 : nz;
  const double *__restrict__ src = w ? zw : zr;
  double *__restrict__ dst = w ? dzw : dzr;
  const long long sj = w ? wsj : rsj, sk = w ? wsk : rsk;
  for (int j = 1 + (int)blockIdx.y; j <= ny; j += (int)gridDim.y) {   // (uniform per block: the barriers are reached by all)
    for (int r = threadIdx.y; r < DEPTHS_TILE; r += blockDim.y) {
      const int k = k0 + r, i = i0 + (int)threadIdx.x;   // both 0-based
      if (k < nzz && i < nx) tile[r][threadIdx.x] = src[(long long)i + (long long)(j - 1) * sj + (long long)k * sk];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < DEPTHS_TILE; r += blockDim.y) {
      const int i = i0 + r, k = k0 + (int)threadIdx.x;
      if (i < nx && k < nzz) dst[dcol(j, i + 1, ny) * nzz + k] = tile[threadIdx.x][r];
    }
    __syncthreads();
  }
}

// The library's dense layout into level 1 (what mgx_get_field(1, MGX_ZR / MGX_ZW) returns): the interior columns of both arrays, lanes along k
__global__ __launch_bounds__(256) void k_depths_copy(const double *__restrict__ zr, const double *__restrict__ zw, double *__restrict__ dzr,
                                                     double *__restrict__ dzw, int nx, int ny, int nz) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned nk = (unsigned)(2 * nz + 1), c = t / nk;
  const int kk = (int)(t - c * nk);
  const unsigned ci = c / (unsigned)ny;
  const int j = 1 + (int)(c - ci * (unsigned)ny), i = 1 + (int)ci;
  if (i > nx) return;
  const long long col = dcol(j, i, ny);
  if (kk < nz) dzr[col * nz + kk] = zr[col * nz + kk];
  else dzw[col * (nz + 1) + (kk - nz)] = zw[col * (nz + 1) + (kk - nz)];
}

// h = -zw(1) and zeta = zw(nz+1) on 0:ny+1 x 0:nx+1 of a level, after the halo fill of zw: grid(lev)%h and %zeta stay what they mean
__global__ void k_depths_hz(GeoView G) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (j > G.ny + 1 || i > G.nx + 1) return;
  const long long col = dcol(j, i, G.ny) * (G.nz + 1), o2 = (long long)i * (G.ny + 2) + j;
  G.h[o2] = -G.zw[col];
  G.zeta[o2] = G.zw[col + G.nz];
}

extern "C" {
// F: the fine level; the coarse level has nxc x nyc columns (its pre-gather block on a gathered level) of nzc rows.  block = 0: zrc, zwc are the
// coarse level's own arrays; block = 1: packed interior blocks of nzc and nzc + 1 rows
void mgxd_coarsen(hipStream_t st, const GeoView *F, int nxc, int nyc, int nzc, double *zrc, double *zwc, int block) {
  const DepthsRunChoice c = choose_depths_coarsen(nxc, nyc, nzc);
  const int oj = block ? -1 : 1, ow = block ? nyc : nyc + 4;
  if (nzc == F->nz) hipLaunchKernelGGL(k_depths_coarsen<true>, dim3(c.grid), dim3(c.block), 0, st, F->zr, F->zw, zrc, zwc, F->ny, F->nz, nxc, nyc, nzc, oj, ow);
  else hipLaunchKernelGGL(k_depths_coarsen<false>, dim3(c.grid), dim3(c.block), 0, st, F->zr, F->zw, zrc, zwc, F->ny, F->nz, nxc, nyc, nzc, oj, ow);
}
void mgxd_in(hipStream_t st, const double *zr, const double *zw, const mgx_depth_strides *s, const GeoView *G) {
  const DepthsInChoice c = choose_depths_in(G->nx, G->ny, G->nz);
  hipLaunchKernelGGL(k_depths_in, dim3(c.gx, c.gy), dim3(c.bx, c.by), 0, st, zr, zw, s->zr_sj, s->zr_sk, s->zw_sj, s->zw_sk, G->zr, G->zw, G->nx, G->ny,
                     G->nz, c.ti, c.ktr);
}
void mgxd_copy(hipStream_t st, const double *zr, const double *zw, const GeoView *G) {
  const DepthsRunChoice c = choose_depths_copy(G->nx, G->ny, G->nz);
  hipLaunchKernelGGL(k_depths_copy, dim3(c.grid), dim3(c.block), 0, st, zr, zw, G->zr, G->zw, G->nx, G->ny, G->nz);
}
void mgxd_hz(hipStream_t st, const GeoView *G) {
  const DepthsHzChoice c = choose_depths_hz(G->nx, G->ny);
  hipLaunchKernelGGL(k_depths_hz, dim3(c.gx, c.gy), dim3(c.bx, c.by), 0, st, *G);
}
// what the choices above say for a level 1 of nx x ny x nz: out[0..7] = k_depths_in (i tiles, k tiles of zr, of zw, grid.x, grid.y, block.x,
// block.y, LDS bytes), out[8..9] = k_depths_copy (grid, block), out[10..11] = k_depths_coarsen of its halving (or, nz odd, held) pair,
// out[12..15] = k_depths_hz (grid.x, grid.y, block.x, block.y), out[16] = the level's colour pass takes the stored coefficients
void mgxd_choice(int nx, int ny, int nz, int *out) {
  const DepthsInChoice a = choose_depths_in(nx, ny, nz);
  const DepthsRunChoice b = choose_depths_copy(nx, ny, nz), d = choose_depths_coarsen(nx / 2, ny / 2, (nz & 1) ? nz : nz / 2);
  const DepthsHzChoice e = choose_depths_hz(nx, ny);
  const int v[17] = {a.ti, a.ktr, a.ktw, (int)a.gx, (int)a.gy, (int)a.bx, (int)a.by, (int)a.lds, (int)b.grid, (int)b.block, (int)d.grid, (int)d.block,
                     (int)e.gx, (int)e.gy, (int)e.bx, (int)e.by, depths_pass_stored(nz) ? 1 : 0};
  for (int q = 0; q < 17; q++) out[q] = v[q];
}
}
