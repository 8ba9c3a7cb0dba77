// The transfers between the levels of the multigrid cycle for gfx950 (MI355X): restriction, prolongation + correction.  Hand-written, fp64.
//
// All arithmetic keeps the reference's operation order and is compiled with -ffp-contract=off, so a
// colour pass of the four-colour smoother, the residual and the transfers are bit-identical to the
// reference's CPU loops (only reductions differ in summation order).
//
// Thread mapping everywhere: one lane = one (j,i) column, lanes run along the unit-stride half-row of
// the JS layout (mgx_internal.h), so every global access of a wave is one contiguous 512-byte run.
#include "mgx_switches.h"
#include "mgx_device.h"

// ------------------------------------------------------------------------------------------------
// Fcycle's first leg below level 1 (mg_solvers.f90:110-115): for lev = l0 .. l0+DEP-1: grid(lev+1)%b = restriction of grid(lev)%r,
// grid(lev+1)%r = grid(lev+1)%b, grid(lev+1)%p = 0 -- a chain in which every level is the 8-cell sum of the one above and nothing else.
// One workgroup takes a (2^DEP)^3 block of the finest level of the chain into LDS and carries it down DEP levels there (4096, 512, 64,
// 8, 1 cells), storing every level's b, r and zeroed p with their physical images on the way: one launch instead of DEP (the small
// levels are launch-bound: 6.3 + 5.5 + 4.6 + 4.3 us and three kernel boundaries for the 256x256x32 -> 16x16x2 chain of the bench).
// Same 8-term sum in the same order as k_fine2coarse (left to right: (k,jA,iA) + (k,jA,iB) + (k,jB,iA) + (k,jB,iB), then the same of
// k+1): bit-identical.  Closed levels only (the mirrors then reach every halo cell), none of them gathered.
struct LevChain { LevView v[5]; };
template <int DEP>
__global__ __launch_bounds__(256) void k_restrict_chain(LevChain Ch, Sides ph) {
  constexpr int E = 1 << DEP;
  __shared__ double buf[E * E * E + (E / 2) * (E / 2) * (E / 2)];
  double *cur = buf, *nxt = buf + E * E * E;
  const LevView &F = Ch.v[0];
  const int nbj = F.ny / E, nbk = F.nz / E;
  int bb = blockIdx.x;
  const int kb = bb % nbk; bb /= nbk;
  const int jb = bb % nbj, ib = bb / nbj;
  // the fine block, (i, k, j) with j split by parity so that a lane run is a contiguous half-row run: idx = (ii * E + kk) * E + jj
  for (int t = threadIdx.x; t < E * E * E; t += 256) {
    const int hj = t % (E / 2), par = (t / (E / 2)) & 1, kk = (t / E) % E, ii = t / (E * E);
    const int jj = 2 * hj + par;               // 0-based inside the block: even jj = odd j (1-based)
    const int i = ib * E + ii + 1, j = jb * E + jj + 1, k = kb * E + kk + 1;
    cur[(ii * E + kk) * E + jj] = F.r[(long long)i * F.plane + (long long)(k - 1) * F.RS + jpos(F, j)];
  }
  __syncthreads();
#pragma unroll
  for (int d = 1; d <= DEP; d++) {
    const int e = E >> (d - 1), h = e >> 1;    // edge of the level above and of this one
    const LevView &C = Ch.v[d];
    for (int t = threadIdx.x; t < h * h * h; t += 256) {
      const int jc = t % h, kc = (t / h) % h, ic = t / (h * h);
      const int iA = 2 * ic, iB = iA + 1, k0 = 2 * kc, k1 = k0 + 1, jA = 2 * jc, jB = jA + 1;
#define CH(ii_, kk_, jj_) cur[((ii_) * e + (kk_)) * e + (jj_)]
      const double z = CH(iA, k0, jA) + CH(iB, k0, jA) + CH(iA, k0, jB) + CH(iB, k0, jB) + CH(iA, k1, jA) + CH(iB, k1, jA) + CH(iA, k1, jB) + CH(iB, k1, jB);
#undef CH
      nxt[(ic * h + kc) * h + jc] = z;
      const int i2 = ib * h + ic + 1, j2 = jb * h + jc + 1, k2 = kb * h + kc + 1, cj = jpos(C, j2);
      const long long rc = (long long)(k2 - 1) * C.RS, oc = (long long)i2 * C.plane + rc + cj;
      C.b[oc] = z; mirror_store(C, C.b, rc, j2, i2, cj, z, ph);
      C.r[oc] = z; mirror_store(C, C.r, rc, j2, i2, cj, z, ph);
      C.p[oc] = 0.0; mirror_store(C, C.p, rc, j2, i2, cj, 0.0, ph);
    }
    __syncthreads();
    double *sw = cur; cur = nxt; nxt = sw;
  }
}

// ------------------------------------------------------------------------------------------------
// restriction: coarse b = sum of the 8 fine r.  mg_intergrids.f90:139-162.  One lane = one coarse column.
// `dst` is the coarse b, or the pre-gather block (nxc x nyc) when the coarse level is gathered.
// ------------------------------------------------------------------------------------------------
// blockIdx.z: a run of KC coarse levels -- nothing here is sequential in k, and one wave per coarse column-chunk (1024 waves at 512x512x64:
// one per SIMD, a memory round trip per level, 41 us) is a latency chain, not a stream.
__global__ __launch_bounds__(256) void k_fine2coarse(LevView F, LevView C, double *__restrict__ dst, Sides ph, int stream, double *__restrict__ dup, double *__restrict__ zero, int KC) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int i2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (j2 > C.ny || i2 > C.nx) return;
  const int ka = 1 + blockIdx.z * KC, kb = ka + KC - 1 < C.nz ? ka + KC - 1 : C.nz;
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j = 2*j2-1 (odd) and 2*j2 (even)
  const double *__restrict__ x = F.r;
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  const long long oc = (long long)i2 * C.plane + jpos(C, j2);
  for (int k2 = ka; k2 <= kb; k2++) {
    const long long r0 = (long long)(2 * k2 - 2) * F.RS, r1 = r0 + F.RS;
    const double z = ld_rt(x + o0 + r0 + po, stream) + ld_rt(x + o1 + r0 + po, stream) + ld_rt(x + o0 + r0 + pe, stream) + ld_rt(x + o1 + r0 + pe, stream)
                   + ld_rt(x + o0 + r1 + po, stream) + ld_rt(x + o1 + r1 + po, stream) + ld_rt(x + o0 + r1 + pe, stream) + ld_rt(x + o1 + r1 + pe, stream);
    dst[oc + (long long)(k2 - 1) * C.RS] = z;
    mirror_store(C, dst, (long long)(k2 - 1) * C.RS, j2, i2, jpos(C, j2), z, ph);
    // closed levels only (the mirrors then reach every halo cell): r_c = b_c of Fcycle (mg_solvers.f90:113) and p_c = 0
    // (mg_intergrids.f90:70) written here instead of a copy and a memset launch
    if (dup) { dup[oc + (long long)(k2 - 1) * C.RS] = z; mirror_store(C, dup, (long long)(k2 - 1) * C.RS, j2, i2, jpos(C, j2), z, ph); }
    if (zero) { zero[oc + (long long)(k2 - 1) * C.RS] = 0.0; mirror_store(C, zero, (long long)(k2 - 1) * C.RS, j2, i2, jpos(C, j2), 0.0, ph); }
  }
}

// ------------------------------------------------------------------------------------------------
// prolongation + correction: fine r = interp(coarse p); fine p += fine r (interior).
// mg_intergrids.f90:366-450 (tri-linear, top level x 1/2), :336-363 (nearest), :226 (p = p + r).
// `src` is the coarse p (or the split block).  k_coarse2fine_nearest: one lane = one coarse cell = 2x2x2 fine cells; the tri-linear default is
// k_coarse2fine_run below.
// WR = false: the interpolated correction is added to p without being stored in the fine r.  Inside a cycle nothing reads that r
// before the next compute_residual rewrites it (mg_solvers.f90:129-151), and at level 1 it is a third of this kernel's traffic.
// ------------------------------------------------------------------------------------------------
template <bool WR>
__global__ __launch_bounds__(256) void k_coarse2fine_nearest(LevView F, LevView C, const double *__restrict__ xc, Sides ph, int stream) {
  const int j2 = 1 + blockIdx.x * WAVE + threadIdx.x;
  const int k2 = 1 + blockIdx.y * blockDim.y + threadIdx.y;
  const int i2 = 1 + blockIdx.z;
  if (j2 > C.ny || k2 > C.nz) return;
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j (odd) and j+1 (even)
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  double *__restrict__ rf = F.r;
  double *__restrict__ pf = F.p;
#define PUT(k, OO, PP, val) { const long long ro_ = (long long)((k)-1) * F.RS, t_ = OO + ro_ + PP; const double v_ = (val), w_ = ld_rt(pf + t_, stream) + v_; if (WR) st_rt(rf + t_, v_, stream); st_rt(pf + t_, w_, stream); \
    const int jf_ = (PP == po) ? 2 * j2 - 1 : 2 * j2, if_ = (OO == o0) ? i : i + 1; \
    if (WR) mirror_store(F, rf, ro_, jf_, if_, PP, v_, ph); mirror_store(F, pf, ro_, jf_, if_, PP, w_, ph); }
  const double v = xc[(long long)i2 * C.plane + (long long)(k2 - 1) * C.RS + jpos(C, j2)];
  const int k = 2 * k2 - 1;
  PUT(k, o0, po, v); PUT(k + 1, o0, po, v); PUT(k, o0, pe, v); PUT(k + 1, o0, pe, v);
  PUT(k, o1, po, v); PUT(k + 1, o1, po, v); PUT(k, o1, pe, v); PUT(k + 1, o1, pe, v);
#undef PUT
}

// Tri-linear prolongation + correction, one lane = a run of KC coarse levels of one coarse column.
// (The kernel this one replaced, one lane per coarse cell, fetched 18 coarse values per lane for 8 fine cells -- the 3x3 neighbourhood of
// two coarse levels: 2.25 cache accesses per fine cell next to the one load and one store the cell itself needs; the texture path was busy
// 80 % of the kernel, rocprofv3 MemUnitStalled, and the level-1 launch ran at 4 TB/s.  Measured, decided and removed.)
// Here a lane reads only its OWN column of the three coarse planes i2-1, i2, i2+1, takes the j2-1 / j2+1 columns from its neighbour lanes (the first and last lane of the wave
// fetch theirs), and keeps a three-level window while it walks up: 3 / (8 KC) coarse loads per fine cell instead of 2.25; the fine
// p of the next coarse level are requested before the current level is stored (without that look-ahead the run is a chain of
// load -> store round trips and loses: 106 us; with it 71 us against 83 us of the per-cell kernel at 512x512x64, WR = false).
// The reference's expressions in the reference's order (mg_intergrids.f90:392-446): bit-identical.
// SK: the fine columns (i odd, j odd) are left alone -- the first colour of the four-colour sweep that follows overwrites them without
// reading them (a line solve reads only the other columns; mg_relax.f90:212-230), which is a quarter of this kernel's traffic.  Except
// next to a physical south / west boundary: there the column reads its own old value through the mirrored halo cell (p(0) = p(1)),
// so columns j = 1 and i = 1 are updated (and mirrored) as usual.
template <bool WR, bool SK>
__global__ __launch_bounds__(256) void k_coarse2fine_run(LevView F, LevView C, const double *__restrict__ xc, Sides ph, int stream, int KC) {
  const int lane = threadIdx.x;
  const int j2 = 1 + blockIdx.x * WAVE + lane;
  const int i2 = 1 + blockIdx.z;
  const int nz = C.nz;
  const int ka = 1 + (blockIdx.y * blockDim.y + threadIdx.y) * KC;   // wave-uniform
  if (ka > nz) return;
  const int kb = ka + KC - 1 < nz ? ka + KC - 1 : nz;
  const bool live = j2 <= C.ny;
  const int jl = live ? j2 : C.ny + 1;  // lanes past the row still hand their neighbour a value (the halo column ny+1)
  const int i = 2 * i2 - 1;
  const int po = F.HO + (j2 - 1), pe = F.EO + j2;  // fine j (odd) and j+1 (even)
  const int c0 = jpos(C, jl), cm = jpos(C, jl - 1), cp = jpos(C, jl + 1 <= C.ny + 1 ? jl + 1 : jl);
  const long long q0 = (long long)i2 * C.plane, qm = q0 - C.plane, qp = q0 + C.plane;
  const long long o0 = (long long)i * F.plane, o1 = o0 + F.plane;
  double *__restrict__ rf = F.r;
  double *__restrict__ pf = F.p;
  // one coarse level: v[3*a + b], a = plane (i2-1, i2, i2+1), b = column (j2-1, j2, j2+1)
#define ROW(kk, v)                                                                                                  \
  {                                                                                                                 \
    const long long ro_ = (long long)(((kk) < 1 ? 1 : ((kk) > nz ? nz : (kk))) - 1) * C.RS;                          \
    const double t0_ = xc[qm + ro_ + c0], t1_ = xc[q0 + ro_ + c0], t2_ = xc[qp + ro_ + c0];                         \
    v[1] = t0_; v[4] = t1_; v[7] = t2_;                                                                             \
    v[0] = __shfl_up(t0_, 1, WAVE); v[3] = __shfl_up(t1_, 1, WAVE); v[6] = __shfl_up(t2_, 1, WAVE);                 \
    v[2] = __shfl_down(t0_, 1, WAVE); v[5] = __shfl_down(t1_, 1, WAVE); v[8] = __shfl_down(t2_, 1, WAVE);           \
    /* the wave's two outer columns: ONE request per plane, in which lane 0 asks for its j2-1, the last lane for its j2+1 (the others */ \
    /* repeat their own column) -- selected, not branched to */                                                      \
    const double e0_ = xc[qm + ro_ + ce], e1_ = xc[q0 + ro_ + ce], e2_ = xc[qp + ro_ + ce];                         \
    if (lane == 0) { v[0] = e0_; v[3] = e1_; v[6] = e2_; }                                                          \
    if (lane == WAVE - 1) { v[2] = e0_; v[5] = e1_; v[8] = e2_; }                                                   \
  }
  // the eight fine p of coarse level kk: [4*half + 2*(plane i+1) + (column j+1)], loaded one level ahead of their use
  // (every request of the walk is unconditional -- levels past the run are clamped, lanes past the row shadow the last column: a request
  // inside a branch makes the number of outstanding loads path-dependent and the compiler then waits for vmcnt(0) at every step)
#define LOADP(kk, v)                                                                                                \
  {                                                                                                                 \
    const int kq_ = (kk) <= kb ? (kk) : kb;                                                                         \
    _Pragma("unroll") for (int h_ = 0; h_ < 2; h_++) {                                                              \
      const long long ro_ = (long long)(2 * kq_ - 2 + h_) * F.RS;                                                   \
      if (!SK) v[4 * h_ + 0] = ld_rt(pf + o0 + ro_ + pol, stream);                                                  \
      v[4 * h_ + 1] = ld_rt(pf + o0 + ro_ + pel, stream);                                                           \
      v[4 * h_ + 2] = ld_rt(pf + o1 + ro_ + pol, stream); v[4 * h_ + 3] = ld_rt(pf + o1 + ro_ + pel, stream);       \
    }                                                                                                               \
  }
  // SK: the (i odd, j odd) column is read only next to a physical south / west boundary (a lane- or plane-dependent branch: kept apart)
#define LOADP0(kk, v)                                                                                               \
  if (SK && edge0 && live) {                                                                                        \
    const int kq_ = (kk) <= kb ? (kk) : kb;                                                                         \
    _Pragma("unroll") for (int h_ = 0; h_ < 2; h_++) v[4 * h_ + 0] = ld_rt(pf + o0 + (long long)(2 * kq_ - 2 + h_) * F.RS + po, stream); \
  }
  // fine cell Q of the 2x2 block: bit 1 = plane i+1, bit 0 = column j+1 (Q = 0 is the first colour's column)
#define PUT(k, Q, val) if (!(SK && (Q) == 0) || edge0) { const long long OO_ = ((Q) & 2) ? o1 : o0; const int PP_ = ((Q) & 1) ? pe : po;                      \
    const long long ro_ = (long long)((k)-1) * F.RS, t_ = OO_ + ro_ + PP_; const double v_ = (val), w_ = pc[4 * half + (Q)] + v_;                     \
    if (WR) st_rt(rf + t_, v_, stream); st_rt(pf + t_, w_, stream);                                                                                    \
    const int jf_ = ((Q) & 1) ? 2 * j2 : 2 * j2 - 1, if_ = ((Q) & 2) ? i + 1 : i;                                                                      \
    if (WR) mirror_store(F, rf, ro_, jf_, if_, PP_, v_, ph); mirror_store(F, pf, ro_, jf_, if_, PP_, w_, ph); }
  const bool edge0 = (ph.S && j2 == 1) || (ph.W && i2 == 1);  // SK: the (i odd, j odd) column of this lane is read through a mirror
  const int ce = lane == 0 ? cm : (lane == WAVE - 1 ? cp : c0);
  const int pol = live ? po : F.HO + (C.ny - 1), pel = live ? pe : F.EO + C.ny;  // columns the loads of a lane past the row fall on
  const double a = 9. / 16., b = 3. / 16., c = 1. / 16., d = 27. / 64., e = 9. / 64., f = 3. / 64., g = 1. / 64.;
  double pc[8], pa[8], pb[8];  // fine p of the level in work and of the next one (two levels ahead measured slower: 76 vs 71 us)
  double lo[9], x[9], hi[9], nw[9];  // coarse levels k2-1, k2, k2+1 and, requested one step before its first use, k2+2
#pragma unroll
  for (int q = 0; q < 9; q++) lo[q] = hi[q] = nw[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 8; q++) pa[q] = pb[q] = 0.0;
  LOADP(ka, pa) LOADP0(ka, pa)
  ROW(ka - 1, lo)  // (level 0 does not exist and is never used: clamped)
  ROW(ka, x)
  ROW(ka + 1, hi)
  // one coarse level: CUR holds its fine p, NXT receives those of level kk + 1
#define STEP(kk, CUR, NXT)                                                                                          \
  {                                                                                                                 \
    const int k2 = (kk);                                                                                            \
    LOADP(k2 + 1, NXT) LOADP0(k2 + 1, NXT)                                                                          \
    ROW(k2 + 2, nw)                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 8; q++) pc[q] = CUR[q];                                                   \
    if (live) {                                                                                                     \
      const double xmm = x[0], x0m = x[1], xpm = x[2], xm0 = x[3], x00 = x[4], xp0 = x[5], xmp = x[6], x0p = x[7], xpp = x[8]; \
      _Pragma("unroll") for (int half = 0; half < 2; half++) {                                                      \
        const int k = 2 * k2 - 1 + half;  /* fine level */                                                          \
        if (k == 1) {                      /* bottom level: bilinear (mg_intergrids.f90:392-405) */                  \
          PUT(1, 0, +a * x00 + c * xmm + b * xm0 + b * x0m);                                                   \
          PUT(1, 1, +a * x00 + c * xpm + b * xp0 + b * x0m);                                                   \
          PUT(1, 2, +a * x00 + c * xmp + b * xm0 + b * x0p);                                                   \
          PUT(1, 3, +a * x00 + c * xpp + b * xp0 + b * x0p);                                                   \
        } else if (k == 2 * nz) {          /* top level: 1/2 bilinear (:434-446) */                                  \
          PUT(k, 0, 0.5 * (a * x00 + c * xmm + b * xm0 + b * x0m));                                            \
          PUT(k, 1, 0.5 * (a * x00 + c * xpm + b * xp0 + b * x0m));                                            \
          PUT(k, 2, 0.5 * (a * x00 + c * xmp + b * xm0 + b * x0p));                                            \
          PUT(k, 3, 0.5 * (a * x00 + c * xpp + b * xp0 + b * x0p));                                            \
        } else {                           /* interior: tri-linear, kp = k2-1 for odd k, k2+1 for even k (:407-432) */ \
          const double *__restrict__ y = half ? hi : lo;                                                            \
          const double ymm = y[0], y0m = y[1], ypm = y[2], ym0 = y[3], y00 = y[4], yp0 = y[5], ymp = y[6], y0p = y[7], ypp = y[8]; \
          PUT(k, 0, +d * x00 + f * xmm + e * xm0 + e * x0m + e * y00 + g * ymm + f * ym0 + f * y0m);           \
          PUT(k, 1, +d * x00 + f * xpm + e * xp0 + e * x0m + e * y00 + g * ypm + f * yp0 + f * y0m);           \
          PUT(k, 2, +d * x00 + f * xmp + e * xm0 + e * x0p + e * y00 + g * ymp + f * ym0 + f * y0p);           \
          PUT(k, 3, +d * x00 + f * xpp + e * xp0 + e * x0p + e * y00 + g * ypp + f * yp0 + f * y0p);           \
        }                                                                                                           \
      }                                                                                                             \
    }                                                                                                               \
    _Pragma("unroll") for (int q = 0; q < 9; q++) { lo[q] = x[q]; x[q] = hi[q]; hi[q] = nw[q]; }                    \
  }
  int kk = ka;
  for (; kk + 1 <= kb; kk += 2) {  // no branch around a step inside the loop
    STEP(kk, pa, pb)
    STEP(kk + 1, pb, pa)
  }
  if (kk <= kb) STEP(kk, pa, pb)
#undef STEP
#undef ROW
#undef PUT
#undef LOADP
#undef LOADP0
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
extern "C" {

// does one launch serve the chain of dep restrictions below levels[0]?  (fcycle() asks before it calls mgxk_restrict_chain)
int mgxk_restrict_chain_served(const LevView *const *levels, int dep) { return choose_restrict_chain(lev_shape(levels[0]), dep).served; }
// levels[0 .. dep]: the views of lev, lev+1, ... (dep restrictions, 1 <= dep <= 4); every level closed, not gathered, level 0's nx, ny, nz multiples of 2^dep
void mgxk_restrict_chain(hipStream_t st, const LevView *const *levels, int dep, Sides ph) {
  LevChain Ch;
  for (int q = 0; q <= dep && q < 5; q++) Ch.v[q] = *levels[q];
  for (int q = dep + 1; q < 5; q++) Ch.v[q] = *levels[dep];
  const dim3 grd(choose_restrict_chain(lev_shape(levels[0]), dep).grid);
  const auto launch = [&](auto DEP) { hipLaunchKernelGGL(k_restrict_chain<DEP()>, grd, dim3(256), 0, st, Ch, ph); };
  if (!with_int<1, 2, 3>(dep, launch)) launch(std::integral_constant<int, 4>{});
}
void mgxk_fine2coarse(hipStream_t st, const LevView *F, const LevView *C, double *dst, Sides ph, double *dup, double *zero) {
  const F2cChoice c = choose_fine2coarse(lev_shape(F), lev_shape(C));
  hipLaunchKernelGGL(k_fine2coarse, dim3(c.gx, c.gy, c.gz), dim3(WAVE, 4), 0, st, *F, *C, dst, ph, c.stream, dup, zero, c.kc);
}
// skip1: the caller guarantees that a four-colour relax of the fine level follows (cycles only; see k_coarse2fine_run, SK)
void mgxk_coarse2fine(hipStream_t st, const LevView *F, const LevView *C, const double *src, int linear, Sides ph, int keep_r, int skip1) {
  const C2fChoice c = choose_coarse2fine(lev_shape(F), lev_shape(C), linear, keep_r, skip1, mgx_switches());
  const dim3 grd(c.gx, c.gy, c.gz), blk(WAVE, c.by);
  if (c.run) with_wr_sk(c.wr, c.sk, [&](auto WR, auto SK) { hipLaunchKernelGGL((k_coarse2fine_run<WR(), SK()>), grd, blk, 0, st, *F, *C, src, ph, c.nt, c.kc); });
  else with_bool(c.wr, [&](auto WR) { hipLaunchKernelGGL((k_coarse2fine_nearest<WR()>), grd, blk, 0, st, *F, *C, src, ph, c.nt); });
}

}  // extern "C"
