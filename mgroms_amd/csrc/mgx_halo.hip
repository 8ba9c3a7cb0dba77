// Halo and gather transport of the multigrid cycle for gfx950 (MI355X): physical images, the wrap of a periodic side, pack / unpack of the
// exchange buffers, the peer-to-peer pushes over xGMI, and the gather / split of a coarse level.  Lanes run along the unit-stride half-row of
// the JS layout (mgx_internal.h) wherever an edge allows it.
#include "mgx_switches.h"
#include "mgx_device.h"

// ------------------------------------------------------------------------------------------------
// physical-boundary halo (homogeneous Neumann mirror), nh = 1.  mg_mpi_exchange.f90:509-537 (edges),
// :552,567,582,597 (corners where both sides are physical).  All sources are interior cells.
// grid: x = perimeter index, y = k.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_halo_phys(LevView L, double *__restrict__ a, Sides ph) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const long long ro = (long long)blockIdx.y * L.RS;
  const int nx = L.nx, ny = L.ny;
  if (q < nx) {  // south and north edges of plane i
    const long long o = (long long)(q + 1) * L.plane + ro;
    if (ph.S) a[o + jpos(L, 0)] = a[o + jpos(L, 1)];
    if (ph.N) a[o + jpos(L, ny + 1)] = a[o + jpos(L, ny)];
  } else if (q < nx + ny) {  // west and east planes, j = 1..ny
    const int j = q - nx + 1, c = jpos(L, j);
    if (ph.W) a[ro + c] = a[L.plane + ro + c];
    if (ph.E) a[(long long)(nx + 1) * L.plane + ro + c] = a[(long long)nx * L.plane + ro + c];
  } else if (q == nx + ny) {
    const long long oE = (long long)(nx + 1) * L.plane + ro, oI = (long long)nx * L.plane + ro;
    if (ph.S && ph.W) a[ro + jpos(L, 0)] = a[L.plane + ro + jpos(L, 1)];
    if (ph.S && ph.E) a[oE + jpos(L, 0)] = a[oI + jpos(L, 1)];
    if (ph.N && ph.E) a[oE + jpos(L, ny + 1)] = a[oI + jpos(L, ny)];
    if (ph.N && ph.W) a[ro + jpos(L, ny + 1)] = a[L.plane + ro + jpos(L, ny)];
  }
}

// Halo fill of a level whose neighbours are all the rank itself (option "periodic" on one rank): the wrap in ONE launch, plain loads and
// stores in stream order.  im, jm: what the halo planes i = 0, nx+1 and the halo entries j = 0, ny+1 of a row become -- 0 = left as they are (a
// closed side whose images the producing kernel stored), 1 = the interior one period away (planes nx, 1; entries ny, 1), 2 = the image of a
// closed side that is still due (planes 1, nx; entries 1, ny: k_halo_phys's rule).
//   blockIdx.y = 0, 1: plane 0 / nx+1 as a whole plane of nz * RS doubles, 16 bytes per lane: a streaming copy, contiguous and 128-byte aligned by
//     the layout.  The two j-halo entries of a row are NOT taken from the source plane's halo, which this same launch may be writing (y = 2): they
//     are formed from the source plane's interior by the rule jm, so both kinds of corner come out right whatever the order of the blocks
//     (wrap x wrap: the diagonal cell; wrap x closed: the closed side's image of the wrapped edge).  jm = 0: copied as found (stored earlier).
//   blockIdx.y = 2: the entries j = 0, ny+1 of every row of the planes 1..nx -- of 0..nx+1 when the halo planes are left (im = 0): their corners are
//     then the wrap of the images an earlier kernel stored there.  Two scattered doubles per row; lanes along k, the shorter stride (RS).
// NT: the level does not fit the Infinity Cache (level_streams): the plane copy carries the non-temporal hint like the colour pass.
typedef double v2d __attribute__((ext_vector_type(2)));
template <bool NT>
__global__ __launch_bounds__(256) void k_halo_wrap(LevView L, double *__restrict__ a, int im, int jm) {
  const int nx = L.nx, ny = L.ny;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = jpos(L, 0), cN = jpos(L, ny + 1);                                                    // the j-halo entries of a row ...
  const int s0 = jm == 1 ? jpos(L, ny) : jpos(L, 1), sN = jm == 1 ? jpos(L, 1) : jpos(L, ny);          // ... and their sources
  if (blockIdx.y < 2) {
    if (!im || 2 * t >= L.plane) return;
    const int east = blockIdx.y;
    const int src = im == 1 ? (east ? 1 : nx) : (east ? nx : 1), dst = east ? nx + 1 : 0;
    const double *__restrict__ s = a + (long long)src * L.plane;
    const long long e = 2 * t;   // (RS is a multiple of 16: a pair never straddles two rows)
    v2d v = NT ? __builtin_nontemporal_load((const v2d *)(s + e)) : *(const v2d *)(s + e);
    if (jm) {
      const int c = (int)(e % L.RS);
      const long long ro = e - c;
      if (c == c0) v.x = s[ro + s0]; else if (c + 1 == c0) v.y = s[ro + s0];
      if (c == cN) v.x = s[ro + sN]; else if (c + 1 == cN) v.y = s[ro + sN];
    }
    v2d *d = (v2d *)(a + (long long)dst * L.plane + e);
    if (NT) __builtin_nontemporal_store(v, d); else *d = v;
  } else {
    if (!jm) return;
    const int i0 = im ? 1 : 0, np = im ? nx : nx + 2;
    if (t >= (long long)np * L.nz) return;
    const long long o = (long long)(i0 + (int)(t / L.nz)) * L.plane + (t % L.nz) * L.RS;
    a[o + c0] = a[o + s0];
    a[o + cN] = a[o + sN];
  }
}

// mixed corners, after the edge halos have been received (mg_mpi_exchange.f90:720-743).
// mode per corner (SW,SE,NE,NW): 0 nothing, 1 copy along i from the received S/N halo row, 2 copy along j
// from the received W/E halo plane.
__global__ void k_halo_mixed_corners(LevView L, double *__restrict__ a, int mSW, int mSE, int mNE, int mNW) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= L.nz) return;
  const long long ro = (long long)k * L.RS;
  const int nx = L.nx, ny = L.ny;
  const long long W0 = ro, W1 = L.plane + ro, E0 = (long long)(nx + 1) * L.plane + ro, E1 = (long long)nx * L.plane + ro;
  const int j0 = jpos(L, 0), j1 = jpos(L, 1), jn = jpos(L, ny), jn1 = jpos(L, ny + 1);
  if (mSW == 1) a[W0 + j0] = a[W1 + j0]; else if (mSW == 2) a[W0 + j0] = a[W0 + j1];
  if (mSE == 1) a[E0 + j0] = a[E1 + j0]; else if (mSE == 2) a[E0 + j0] = a[E0 + j1];
  if (mNE == 1) a[E0 + jn1] = a[E1 + jn1]; else if (mNE == 2) a[E0 + jn1] = a[E0 + jn];
  if (mNW == 1) a[W0 + jn1] = a[W1 + jn1]; else if (mNW == 2) a[W0 + jn1] = a[W0 + jn];
}

// pack / unpack of the 8 exchange buffers (edges nz*nx, nz*ny; corners nz).  dir: 0 S,1 E,2 N,3 W,4 SW,5 SE,6 NE,7 NW.
// pack reads the interior edge that the neighbour in direction `dir` needs; unpack writes my halo on side `dir`.
// all present directions in one launch: blockIdx.z = direction (absent ones return), buffers passed by value.
// Buffer element (q,k) of an edge sits at k*n + q (q = position along the edge, lane-contiguous), so the writes of a
// push into a neighbour GPU's memory leave each wave as whole 512-byte runs.
struct HaloBufs { double *b[8]; int present[8]; };
__device__ __forceinline__ bool halo_elem(const LevView &L, int dir, int q, int k, int unpack, long long &e, long long &t) {
  const int nx = L.nx, ny = L.ny;
  int i, j, n;
  switch (dir) {
    case 0: n = nx; i = q + 1; j = unpack ? 0 : 1; break;
    case 1: n = ny; j = q + 1; i = unpack ? nx + 1 : nx; break;
    case 2: n = nx; i = q + 1; j = unpack ? ny + 1 : ny; break;
    case 3: n = ny; j = q + 1; i = unpack ? 0 : 1; break;
    case 4: n = 1; i = unpack ? 0 : 1; j = unpack ? 0 : 1; break;
    case 5: n = 1; i = unpack ? nx + 1 : nx; j = unpack ? 0 : 1; break;
    case 6: n = 1; i = unpack ? nx + 1 : nx; j = unpack ? ny + 1 : ny; break;
    default: n = 1; i = unpack ? 0 : 1; j = unpack ? ny + 1 : ny; break;
  }
  if (q >= n) return false;
  e = (long long)i * L.plane + (long long)k * L.RS + jpos(L, j);
  t = (long long)k * n + q;
  return true;
}
// present[dir] = HALO_SELF (option "periodic": the neighbour in this direction is the rank itself, on a level that has other ranks as neighbours too):
// nothing is packed; the unpack launch assigns halo element (dir, q, k) the interior element that halo_elem packs for the opposite direction.
__device__ __forceinline__ int halo_opp(int d) { return d < 4 ? (d ^ 2) : 4 + ((d - 4) ^ 2); }
// MIXED = false (no self direction: every level of a closed grid) is the kernel as it was before the option existed.
template <bool MIXED>
__global__ void k_halo_pack_all(LevView L, double *__restrict__ a, HaloBufs hb, int unpack) {
  const int dir = blockIdx.z, pr = hb.present[dir];
  if (MIXED ? (pr != HALO_PEER && !(pr == HALO_SELF && unpack)) : !pr) return;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  long long e, t;
  if (!halo_elem(L, dir, q, blockIdx.y, unpack, e, t)) return;
  if (MIXED && pr == HALO_SELF) {
    long long es, ts;
    halo_elem(L, halo_opp(dir), q, blockIdx.y, 0, es, ts);
    a[e] = a[es];
    return;
  }
  double *__restrict__ buf = hb.b[dir];
  if (unpack) a[e] = buf[t]; else buf[t] = a[e];
}

// ---- peer-to-peer halo transport (xGMI, no host in the loop) --------------------------------------------------
// Push: edges are written straight into the NEIGHBOURS' receive buffers (fine-grained device memory opened through
// hipIpc), every block fences at system scope, and the last block to finish raises the sequence number in each
// neighbour's flag.  Unpack: a block spins (bounded) on the LOCAL flag of its direction, then copies the received edge
// into the halo.  Receive buffers alternate by the parity of the per-level sequence number:
// a rank cannot push exchange n+2 before it has unpacked n+1, which its neighbour pushed after unpacking n.
// bound of every wait on a peer's flag, in ticks of the 100 MHz constant clock (5 s; MGX_P2P_TIMEOUT_MS / mgxk_set_p2p_timeout shorten it for tests)
__device__ long long g_p2p_timeout_ticks = 500000000LL;
struct HaloP2P {
  int drop;                     // test hook: this launch does not raise the neighbours' flags (a rank that went silent)
  unsigned long long *flag[8];  // push: the neighbour's flag to raise; unpack: the local flag to wait on
  unsigned long long seq;
  unsigned int *counter;        // blocks-done counter of the push launch (device memory, left at 0)
  int *err;                     // host-mapped error word: 1 = a wait timed out
  int mSW, mSE, mNE, mNW;       // unpack: mixed corners (one side physical, the other a neighbour), see k_halo_mixed_corners
  int blk0[9];                  // compact 1-D grid: blocks blk0[d] .. blk0[d+1]-1 serve direction d (empty when absent)
  int ipt;                      // items per thread (> 1 only for very long edges: keeps the grid within what is resident)
  int nreal;                    // blocks that serve a real peer: the ones that push, report in and wait
};
// item w of direction d is buffer element w = k*n_d + q: consecutive lanes = consecutive buffer elements
__device__ __forceinline__ int halo_dir(const HaloP2P &pp) {
  int dir = 0;
#pragma unroll
  for (int d = 1; d < 8; d++) if ((int)blockIdx.x >= pp.blk0[d]) dir = d;
  return dir;
}
__device__ __forceinline__ bool halo_item(const LevView &L, const HaloP2P &pp, int dir, int r, int unpack, int &q, int &k, long long &e, long long &t) {
  const int n = (dir == 0 || dir == 2) ? L.nx : ((dir == 1 || dir == 3) ? L.ny : 1);
  const int w = (((int)blockIdx.x - pp.blk0[dir]) * pp.ipt + r) * blockDim.x + threadIdx.x;
  if (w >= n * L.nz) return false;
  k = w / n; q = w - k * n;
  return halo_elem(L, dir, q, k, unpack, e, t);
}
// One launch per halo fill: every block first pushes its part of direction d into the neighbour's receive buffer, the last
// block to finish pushing raises the neighbours' flags, then every block waits (bounded) on the LOCAL flag of its
// direction and unpacks the same part of the edge it received.  The grid is at most ~128 blocks (compact, present
// directions only, several items per thread on long edges), well below what the GPU keeps resident, so a block that
// spins never keeps a pushing block from starting; should that ever fail the 5 s time-out turns it into an error.
struct HaloXchg { double *rbuf[8]; double *lbuf[8]; unsigned long long *rflag[8]; unsigned long long *lflag[8]; int present[8]; };
// hx.present[d] = HALO_SELF / HALO_MIRROR (a mixed level of option "periodic": the wrap is local in one direction, the other has real peers): the
// blocks of such a direction take no part in the protocol -- no slab, no counter, no flag raised or waited on.  They assign halo element (d, q, k)
// the interior element that halo_elem packs for opp(d) (the rank is its own neighbour) or for d (the image of a closed side), with the same
// mixed-corner stores, and return.  Every halo cell is written from interior cells only, so the directions need no order among them.
__device__ __forceinline__ void halo_store(const LevView &L, const HaloP2P &pp, double *__restrict__ a, int dir, int q, int k, long long e, double v) {
  const int nx = L.nx, ny = L.ny;
  a[e] = v;
  // mixed corners (mg_mpi_exchange.f90:720-743): the corner next to a physical side mirrors the edge halo cell that was
  // just received -- written here by the thread that unpacked that cell instead of a separate launch
  const long long ro = (long long)k * L.RS, W0 = ro, E0 = (long long)(nx + 1) * L.plane + ro;
  if (dir == 0) { if (q == 0 && pp.mSW == 1) a[W0 + jpos(L, 0)] = v; if (q == nx - 1 && pp.mSE == 1) a[E0 + jpos(L, 0)] = v; }
  else if (dir == 2) { if (q == 0 && pp.mNW == 1) a[W0 + jpos(L, ny + 1)] = v; if (q == nx - 1 && pp.mNE == 1) a[E0 + jpos(L, ny + 1)] = v; }
  else if (dir == 3) { if (q == 0 && pp.mSW == 2) a[W0 + jpos(L, 0)] = v; if (q == ny - 1 && pp.mNW == 2) a[W0 + jpos(L, ny + 1)] = v; }
  else if (dir == 1) { if (q == 0 && pp.mSE == 2) a[E0 + jpos(L, 0)] = v; if (q == ny - 1 && pp.mNE == 2) a[E0 + jpos(L, ny + 1)] = v; }
}
// MIXED = false (every present direction is another rank: every level of a closed grid) is the kernel as it was before the option existed.
template <bool MIXED>
__global__ __launch_bounds__(256) void k_halo_exchange(LevView L, double *__restrict__ a, HaloXchg hx, HaloP2P pp) {
  const int dir = halo_dir(pp);  // block-uniform
  int q, k; long long e, t;
  if (MIXED && hx.present[dir] != HALO_PEER) {  // block-uniform: the rank itself, or a closed side's image
    const int sdir = hx.present[dir] == HALO_SELF ? halo_opp(dir) : dir;
    for (int r = 0; r < pp.ipt; r++) {
      if (!halo_item(L, pp, dir, r, 1, q, k, e, t)) continue;
      long long es, ts;
      halo_elem(L, sdir, q, k, 0, es, ts);
      halo_store(L, pp, a, dir, q, k, e, a[es]);
    }
    return;
  }
  for (int r = 0; r < pp.ipt; r++)
    if (halo_item(L, pp, dir, r, 0, q, k, e, t)) hx.rbuf[dir][t] = a[e];
  // every storing wave drains its remote writes, the block meets, ONE lane issues the system-scope release before the block reports in
  // (256 lanes fencing cost 2-4x one lane's: MI355X_MICROARCH.md, inter-workgroup visibility)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ int ok;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(pp.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (MIXED ? (unsigned int)pp.nreal : gridDim.x) - 1) {
      __hip_atomic_store(pp.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      for (int d = 0; d < 8; d++)
        if ((MIXED ? hx.present[d] == HALO_PEER : hx.present[d] != 0) && !pp.drop) __hip_atomic_store(hx.rflag[d], pp.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    ok = 0;
    const long long t0 = wall_clock64(), tmax = g_p2p_timeout_ticks;
    while (true) {
      if (__hip_atomic_load(hx.lflag[dir], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) >= pp.seq) { ok = 1; break; }
      if (wall_clock64() - t0 > tmax) break;  // 5 s of the 100 MHz constant clock: the neighbour is gone
      __builtin_amdgcn_s_sleep(4);
    }
  }
  __syncthreads();
  if (!ok) { if (threadIdx.x == 0) *pp.err = 1; return; }
  __threadfence_system();
  for (int r = 0; r < pp.ipt; r++) {
    if (!halo_item(L, pp, dir, r, 1, q, k, e, t)) continue;
    halo_store(L, pp, a, dir, q, k, e, __builtin_nontemporal_load(hx.lbuf[dir] + t));
  }
}

// gather (mg_gather.f90:95-174): copy the interior of member block (l,m) (reference layout incl. halo, as received)
// into the JS coarse b at offset (l*nxc, m*nyc)
__global__ void k_gather_place(LevView C, double *__restrict__ dstjs, const double *__restrict__ blk, int nxc, int nyc, int l, int m) {
  const long long n = (long long)C.nz * nyc * nxc;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int k = (int)(t % C.nz);
  const long long ji = t / C.nz;
  const int j = 1 + (int)(ji % nyc), i = 1 + (int)(ji / nyc);
  const double v = blk[((long long)i * (nyc + 2) + j) * C.nz + k];
  dstjs[(long long)(i + l * nxc) * C.plane + (long long)k * C.RS + jpos(C, j + m * nyc)] = v;
}
// pre-gather block (JS level view Cs of the small block) -> contiguous reference-layout block incl. halo
__global__ void k_block_to_ref(LevView Cs, const double *__restrict__ js, double *__restrict__ blk) {
  const long long n = (long long)Cs.nz * (Cs.ny + 2) * (Cs.nx + 2);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int k = (int)(t % Cs.nz);
  const long long ji = t / Cs.nz;
  const int j = (int)(ji % (Cs.ny + 2)), i = (int)(ji / (Cs.ny + 2));
  blk[t] = js[(long long)i * Cs.plane + (long long)k * Cs.RS + jpos(Cs, j)];
}
// Peer-to-peer gather (same protocol as the halo pushes): my restricted block, converted to the reference layout on
// the fly, is written into slot `me` of every group member's gather buffer (mine included); the last block raises my
// flag at the other members.  k_gather_place_wait then waits for member q's flag before placing its block.
struct GatherP2P { double *dst[4]; unsigned long long *flag[4]; int ng, me; unsigned long long seq; unsigned int *counter; int *err; };
__global__ void k_gather_push(LevView Cs, const double *__restrict__ js, GatherP2P gp) {
  // block layout in the gather buffers: (i, k, j) with j fastest (halo included) -- lanes run along j on both sides
  const long long n = (long long)Cs.nz * (Cs.ny + 2) * (Cs.nx + 2);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(t % (Cs.ny + 2));
    const long long ik = t / (Cs.ny + 2);
    const int k = (int)(ik % Cs.nz), i = (int)(ik / Cs.nz);
    const double v = js[(long long)i * Cs.plane + (long long)k * Cs.RS + jpos(Cs, j)];
    for (int q = 0; q < gp.ng; q++) gp.dst[q][t] = v;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // as k_halo_exchange: waves drain, the block meets, one lane releases at system scope
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(gp.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      __hip_atomic_store(gp.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      for (int q = 0; q < gp.ng; q++)
        if (q != gp.me) __hip_atomic_store(gp.flag[q], gp.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
__global__ void k_gather_place_wait(LevView C, double *__restrict__ dstjs, const double *__restrict__ blk, int nxc, int nyc, int l, int m,
                                    unsigned long long *flag, unsigned long long seq, int *err) {
  if (flag) {
    __shared__ int ok;
    if (threadIdx.x == 0) {
      ok = 0;
      const long long t0 = wall_clock64(), tmax = g_p2p_timeout_ticks;
      while (true) {
        if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) >= seq) { ok = 1; break; }
        if (wall_clock64() - t0 > tmax) break;
        __builtin_amdgcn_s_sleep(4);
      }
    }
    __syncthreads();
    if (!ok) { if (threadIdx.x == 0) *err = 1; return; }
    __threadfence_system();
  }
  const long long n = (long long)C.nz * nyc * nxc;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int j = 1 + (int)(t % nyc);
    const long long ik = t / nyc;
    const int k = (int)(ik % C.nz), i = 1 + (int)(ik / C.nz);
    const double v = __builtin_nontemporal_load(blk + ((long long)i * C.nz + k) * (nyc + 2) + j);
    dstjs[(long long)(i + l * nxc) * C.plane + (long long)k * C.RS + jpos(C, j + m * nyc)] = v;
  }
}
// split (mg_gather.f90:177-220): own quadrant of the gathered p, halo included, into the small JS block
__global__ void k_split(LevView C, LevView Cs, const double *__restrict__ pc, double *__restrict__ dst, int l, int m) {
  const long long n = (long long)Cs.nz * (Cs.ny + 2) * (Cs.nx + 2);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int k = (int)(t % Cs.nz);
  const long long ji = t / Cs.nz;
  const int j = (int)(ji % (Cs.ny + 2)), i = (int)(ji / (Cs.ny + 2));
  dst[(long long)i * Cs.plane + (long long)k * Cs.RS + jpos(Cs, j)] =
      pc[(long long)(i + l * Cs.nx) * C.plane + (long long)k * C.RS + jpos(C, j + m * Cs.ny)];
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
extern "C" {

void mgxk_halo_phys(hipStream_t st, const LevView *L, double *a, Sides ph) {
  const int n = L->nx + L->ny + 1;
  hipLaunchKernelGGL(k_halo_phys, dim3((n + 255) / 256, L->nz), dim3(256), 0, st, *L, a, ph);
}
void mgxk_halo_wrap(hipStream_t st, const LevView *L, double *a, int im, int jm) {
  const WrapChoice c = choose_halo_wrap(lev_shape(L), im, jm);
  if (c.none) return;
  with_bool(c.nt, [&](auto NT) { hipLaunchKernelGGL((k_halo_wrap<NT()>), dim3(c.grid, 3), dim3(256), 0, st, *L, a, im, jm); });
}
void mgxk_halo_mixed_corners(hipStream_t st, const LevView *L, double *a, int mSW, int mSE, int mNE, int mNW) {
  hipLaunchKernelGGL(k_halo_mixed_corners, dim3((L->nz + 63) / 64), dim3(64), 0, st, *L, a, mSW, mSE, mNE, mNW);
}
void mgxk_halo_pack_all(hipStream_t st, const LevView *L, double *a, double *const *bufs, const int *present, int unpack) {
  HaloBufs hb;
  for (int d = 0; d < 8; d++) { hb.b[d] = bufs[d]; hb.present[d] = present[d]; }
  const PackChoice c = choose_halo_pack(lev_shape(L), present);
  with_bool(c.mixed, [&](auto MIXED) { hipLaunchKernelGGL((k_halo_pack_all<MIXED()>), dim3(c.gx, c.gy, 8), dim3(64), 0, st, *L, a, hb, unpack); });
}
void mgxk_halo_p2p(hipStream_t st, const LevView *L, double *a, double *const *rbuf, double *const *lbuf, unsigned long long *const *rflag,
                   unsigned long long *const *lflag, const int *present, unsigned long long seq, unsigned int *counter, int *err, const int *mixed, int drop) {
  const P2pPlan c = choose_halo_p2p(lev_shape(L), present, mgx_switches());
  if (c.nb == 0 || c.nreal == 0) return;
  HaloXchg hx; HaloP2P pp;
  for (int d = 0; d < 8; d++) {
    hx.rbuf[d] = rbuf[d]; hx.lbuf[d] = lbuf[d]; hx.rflag[d] = rflag[d]; hx.lflag[d] = lflag[d]; hx.present[d] = present[d];
    pp.flag[d] = nullptr;
  }
  for (int d = 0; d < 9; d++) pp.blk0[d] = c.blk0[d];
  pp.drop = drop; pp.ipt = c.ipt; pp.nreal = c.nreal;
  pp.seq = seq; pp.counter = counter; pp.err = err;
  pp.mSW = mixed[0]; pp.mSE = mixed[1]; pp.mNE = mixed[2]; pp.mNW = mixed[3];
  with_bool(c.mixed, [&](auto MIXED) { hipLaunchKernelGGL((k_halo_exchange<MIXED()>), dim3(c.nb), dim3(256), 0, st, *L, a, hx, pp); });
}
// the bound of every p2p flag wait, in milliseconds (device global of this library; all instances of the process)
int mgxk_set_p2p_timeout(double ms) {
  const long long ticks = (long long)(ms * 1e5);
  return hipMemcpyToSymbol(HIP_SYMBOL(g_p2p_timeout_ticks), &ticks, sizeof ticks) == hipSuccess ? 0 : 1;
}
// out[0] = 1.0 when the host-mapped error word is set or `extra` is non-zero, else 0.0 -- in stream order, so that a time-out of a kernel
// still in flight reaches the all-reduce that follows (collective agreement on the health of the peer-to-peer transport)
__global__ void k_err_to_double(const int *err, int extra, double *out) { out[0] = (err && *err != 0) || extra ? 1.0 : 0.0; }
void mgxk_err_to_double(hipStream_t st, const int *err, int extra, double *out) { hipLaunchKernelGGL(k_err_to_double, dim3(1), dim3(1), 0, st, err, extra, out); }
void mgxk_gather_place(hipStream_t st, const LevView *C, double *dstjs, const double *blk, int nxc, int nyc, int l, int m) {
  const long long n = (long long)C->nz * nyc * nxc;
  hipLaunchKernelGGL(k_gather_place, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *C, dstjs, blk, nxc, nyc, l, m);
}
void mgxk_block_to_ref(hipStream_t st, const LevView *Cs, const double *js, double *blk) {
  const long long n = (long long)Cs->nz * (Cs->ny + 2) * (Cs->nx + 2);
  hipLaunchKernelGGL(k_block_to_ref, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *Cs, js, blk);
}
void mgxk_gather_push(hipStream_t st, const LevView *Cs, const double *js, double *const *dst, unsigned long long *const *flags, int ng, int me,
                      unsigned long long seq, unsigned int *counter, int *err) {
  GatherP2P gp;
  for (int q = 0; q < 4; q++) { gp.dst[q] = q < ng ? dst[q] : nullptr; gp.flag[q] = q < ng ? flags[q] : nullptr; }
  gp.ng = ng; gp.me = me; gp.seq = seq; gp.counter = counter; gp.err = err;
  hipLaunchKernelGGL(k_gather_push, dim3(choose_gather_push(lev_shape(Cs))), dim3(256), 0, st, *Cs, js, gp);
}
void mgxk_gather_place_wait(hipStream_t st, const LevView *C, double *dstjs, const double *blk, int nxc, int nyc, int l, int m,
                            unsigned long long *flag, unsigned long long seq, int *err) {
  hipLaunchKernelGGL(k_gather_place_wait, dim3(choose_gather_place_wait(C->nz, nxc, nyc, flag != nullptr)), dim3(256), 0, st, *C, dstjs, blk, nxc, nyc, l, m, flag, seq, err);
}
void mgxk_split(hipStream_t st, const LevView *C, const LevView *Cs, const double *pc, double *dst, int l, int m) {
  const long long n = (long long)Cs->nz * (Cs->ny + 2) * (Cs->nx + 2);
  hipLaunchKernelGGL(k_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *C, *Cs, pc, dst, l, m);
}

}  // extern "C"
