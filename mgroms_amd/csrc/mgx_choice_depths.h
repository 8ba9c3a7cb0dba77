// Which launch serves the kernels of mgx_depths.hip (the matrices from the caller's own z_r, z_w), and which levels keep what when the depths
// are the caller's: pure host functions in the style of mgx_choice_transfer.h -- no HIP call, no state, no environment, one small result
// struct per kernel.  mgx_depths.hip launches by them, mgx_depths_launch (include/mgx.h) reports them, tests/test_depths_host.py pins them.
#pragma once
#include <cstddef>

// ---- k_depths_in: (i, k) tiles of one row j through LDS, both arrays in one launch ----
// A tile is DEPTHS_TILE x DEPTHS_TILE doubles: 64 lanes x 8 B = one 512-byte run along i on the load side and along k on the store side.
// Rows of DEPTHS_TILE + 1 doubles keep the transposed reads off each other's banks.  grid.x = i tiles x (k tiles of zr + k tiles of zw),
// grid.y = rows j, capped at the grid limit (the kernel strides over the rest).
constexpr int DEPTHS_TILE = 64;
struct DepthsInChoice { int ti, ktr, ktw; unsigned gx, gy, bx, by; size_t lds; };
static inline DepthsInChoice choose_depths_in(int nx, int ny, int nz) {
  DepthsInChoice c;
  c.ti = (nx + DEPTHS_TILE - 1) / DEPTHS_TILE;
  c.ktr = (nz + DEPTHS_TILE - 1) / DEPTHS_TILE;
  c.ktw = (nz + 1 + DEPTHS_TILE - 1) / DEPTHS_TILE;
  c.gx = (unsigned)c.ti * (unsigned)(c.ktr + c.ktw);
  c.gy = ny > 65535 ? 65535u : (unsigned)ny;
  c.bx = DEPTHS_TILE; c.by = 4;
  c.lds = (size_t)DEPTHS_TILE * (DEPTHS_TILE + 1) * sizeof(double);
  return c;
}

// ---- the kernels with one lane per (k, column): 256 threads per block over n items ----
struct DepthsRunChoice { long long items; unsigned grid, block; };
static inline DepthsRunChoice ch_depths_run(long long n) { return {n, (unsigned)((n + 255) / 256), 256u}; }
// k_depths_coarsen: one lane per coarse interface, nzc + 1 of them per coarse column (the lane of interface kc <= nzc also writes zr_C(kc))
static inline DepthsRunChoice choose_depths_coarsen(int nxc, int nyc, int nzc) { return ch_depths_run((long long)(nzc + 1) * nyc * nxc); }
// k_depths_copy (the dense layout): one lane per element of the two interior columns, nz of zr and nz + 1 of zw
static inline DepthsRunChoice choose_depths_copy(int nx, int ny, int nz) { return ch_depths_run((long long)(2 * nz + 1) * ny * nx); }
// k_depths_hz: one lane per column of 0:ny+1 x 0:nx+1, lanes along j
struct DepthsHzChoice { unsigned gx, gy, bx, by; };
static inline DepthsHzChoice choose_depths_hz(int nx, int ny) { return {(unsigned)((ny + 2 + 63) / 64), (unsigned)((nx + 2 + 3) / 4), 64u, 4u}; }

// ---- what a pair of levels is to the coarsening rule of the depths ----
enum { DEPTHS_HALVE = 0, DEPTHS_HELD = 1, DEPTHS_REFUSED = 2 };
// halving needs an even nz_F: from an odd one the rule has no top interface
static inline int depths_pair(int nzf, int nzc) { return nzc == nzf ? DEPTHS_HELD : ((nzf & 1) ? DEPTHS_REFUSED : DEPTHS_HALVE); }

// ---- the colour pass of a level whose depths are the caller's ----
// The matrix-free instances of the register-resident colour pass from nz = 32 on (k_relax_nz: ZW = MF && NZ >= 32) and of the tall-column
// pass (nz = 80, 96, 128) generate slots 4 / 7, zw and the column's own slopes from the nine sigma fields at compile time: they have no
// instance that streams them.  A level without those fields hands such a pass the stored coefficients (the instances a masked domain runs);
// below nz = 32 the matrix-free instances stream slots 4 / 7 and take the slopes as they are.
static inline bool depths_pass_stored(int nz) { return nz >= 32; }
