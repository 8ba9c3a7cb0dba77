// Kernels of the Krylov-accelerated solve_p (option "krylov" = m, mgx_cycle.cpp: solve_p_krylov) for gfx950 (MI355X): truncated GCR /
// Orthomin(m) around the F-cycle.  Three launches per iteration on level 1, each followed by a one-launch reduction of its per-workgroup
// partial sums in index order (the order of k_reduce_partials, mgx_kernels.hip): a solve is reproducible run to run.
//   1. k_kr_apply[_mf]: q = A z and the inner products (q, q_i) with the retained q_i
//   2. k_kr_ortho:      q -= sum beta_i q_i, z -= sum beta_i z_i (beta_i = (q, q_i) / (q_i, q_i)), s = (q, q), t = (r, q)
//   3. k_kr_update:     p += (t / s) z, r -= (t / s) q, ||r||^2
// The scalars stay in device memory between the launches (kernels 2 and 3 read them there).  The operator is the one of k_residual /
// k_residual_mf with b = 0 and the sign turned: the same products subtracted in the same order, so q is bit for bit the negative of what
// compute_residual writes for a zero right-hand side.  Kernels 2 and 3 are streaming passes over WHOLE arrays (halo and padding included:
// z and p keep consistent halos by linearity, q and r are zero / untouched there) with 16-byte accesses; only interior cells enter the sums.
#include "mgx_device.h"

#define KR_MAX 8
struct KrDirs { const double *q[KR_MAX]; const double *z[KR_MAX]; int slot[KR_MAX]; int n; };  // slot: where (q_i, q_i) is filed

typedef double d2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d2_t ld2(const double *p, int nt) { return nt ? __builtin_nontemporal_load((const d2_t *)p) : *(const d2_t *)p; }
__device__ __forceinline__ void st2(double *p, d2_t v, int nt) { if (nt) __builtin_nontemporal_store(v, (d2_t *)p); else *(d2_t *)p = v; }

// workgroup sums of NV per-lane values in a fixed order (wave shuffle, then the waves in index order) -> partial[v * nblk + blk]
template <int NV>
__device__ __forceinline__ void kr_block_sums(double (&acc)[NV], int nv, double *__restrict__ partial, int blk, int nblk) {
  __shared__ double red[NV][4];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x, w = tid >> 6;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    if (v < nv) {
      double a = acc[v];
      for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
      if ((tid & 63) == 0) red[v][w] = a;
    }
  }
  __syncthreads();
  if (tid < nv) partial[(long long)tid * nblk + blk] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// the block -> (j-chunk, plane group, j parity) map of k_residual: each XCD owns a contiguous range of plane groups
__device__ __forceinline__ void kr_block_map(int gx, int gy, int &bx, int &by, int &bz) {
  const int per = gx * 2;
  int grp, local;
  if ((gy & 7) == 0) { const int xcd = blockIdx.x & 7; local = blockIdx.x >> 3; grp = xcd * (gy >> 3) + local / per; local -= (local / per) * per; }
  else { grp = blockIdx.x / per; local = blockIdx.x - grp * per; }
  by = grp; bz = local / gx; bx = local - bz * gx;
}

// ------------------------------------------------------------------------------------------------
// 1. q = A z from the stored slots (the operator of k_residual, mg_relax.f90:421-515), z = L.p with valid halos
// ------------------------------------------------------------------------------------------------
template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply(LevView L, double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  kr_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const long long RS = L.RS;
    const int nz = L.nz;
    const double *__restrict__ p = L.p;
    const double *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1], *__restrict__ a3 = L.cA[2],
                 *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4], *__restrict__ a6 = L.cA[5],
                 *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7];
    const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;
    double pjm_m, pjm_0, pjm_p, pim_m, pim_0, pim_p, pc_m, pc_0, pc_p, a2_0, a2_p;
    double m3_m, m3_0, m4_0, m5_p, n6_m, n6_0, n7_0, n8_p, m3_p, m4_p, n6_p, n7_p;
#define LOAD_ROW(q, PJM, PIM, PC, A2, M3, M4, M5, N6, N7, N8)                  \
  {                                                                            \
    const long long ro = (long long)((q)-1) * RS;                              \
    PJM = p[o + ro + jm]; PIM = p[om + ro + c]; PC = p[o + ro + c]; A2 = a2[o + ro + c]; \
    const double pj_ = p[o + ro + jp], pi_ = p[op + ro + c];                   \
    M3 = a3[o + ro + jp] * pj_; M4 = a4[o + ro + jp] * pj_; M5 = a5[o + ro + jp] * pj_; \
    N6 = a6[op + ro + c] * pi_; N7 = a7[op + ro + c] * pi_; N8 = a8[op + ro + c] * pi_; \
  }
#define PUT_ROW(ko, rr)                                                        \
  { const double qv = -(rr);                                                   \
    st_rt(qout + (ko), qv, stream);                                            \
    _Pragma("unroll") for (int n = 0; n < KR_MAX; n++) if (n < D.n) acc[n] = acc[n] + qv * D.q[n][ko]; }
    const double zero = 0.0;
    double dum5, dum8;
    LOAD_ROW(1, pjm_0, pim_0, pc_0, a2_0, m3_0, m4_0, dum5, n6_0, n7_0, dum8);
    LOAD_ROW(2, pjm_p, pim_p, pc_p, a2_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);
    (void)dum5; (void)dum8;
    double rr = zero - a1[o + c] * pc_0 - a2_p * pc_p - a3[o + c] * pjm_p - a4[o + c] * pjm_0 - m4_0 - m5_p
                - a6[o + c] * pim_p - a7[o + c] * pim_0 - n7_0 - n8_p;
    if (REAL)
      rr = rr - a5[o + c] * p[om + jp] - a5[op + jm] * p[op + jm] - a8[o + c] * p[om + jm] - a8[op + jp] * p[op + jp];
    PUT_ROW(o + c, rr)
    for (int k = 2; k <= nz - 1; k++) {
      pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p; pc_m = pc_0; pc_0 = pc_p; a2_0 = a2_p;
      m3_m = m3_0; m3_0 = m3_p; m4_0 = m4_p; n6_m = n6_0; n6_0 = n6_p; n7_0 = n7_p;
      LOAD_ROW(k + 1, pjm_p, pim_p, pc_p, a2_p, m3_p, m4_p, m5_p, n6_p, n7_p, n8_p);
      const long long ko = o + (long long)(k - 1) * RS + c;
      rr = zero - a1[ko] * pc_0 - a2_0 * pc_m - a2_p * pc_p - a3[ko] * pjm_p - m3_m - a4[ko] * pjm_0 - m4_0
                - a5[ko] * pjm_m - m5_p - a6[ko] * pim_p - n6_m - a7[ko] * pim_0 - n7_0 - a8[ko] * pim_m - n8_p;
      PUT_ROW(ko, rr)
    }
    {
      pjm_m = pjm_0; pjm_0 = pjm_p; pim_m = pim_0; pim_0 = pim_p; pc_m = pc_0; pc_0 = pc_p; a2_0 = a2_p;
      m3_m = m3_0; m4_0 = m4_p; n6_m = n6_0; n7_0 = n7_p;
      const long long ko = o + (long long)(nz - 1) * RS + c;
      rr = zero - a1[ko] * pc_0 - a2_0 * pc_m - m3_m - a4[ko] * pjm_0 - m4_0 - a5[ko] * pjm_m - n6_m
                - a7[ko] * pim_0 - n7_0 - a8[ko] * pim_m;
      PUT_ROW(ko, rr)
    }
#undef LOAD_ROW
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}

// 1. matrix-free: the operator of k_residual_mf (cross terms from the slopes, the interior rows' diagonal rebuilt in the reference's order)
template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply_mf(LevView L, double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  kr_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const long long RS = L.RS;
    const int nz = L.nz;
    const double *__restrict__ p = L.p;
    const double *__restrict__ a1 = L.cA[0], *__restrict__ a2 = L.cA[1], *__restrict__ a4 = L.cA[3], *__restrict__ a5 = L.cA[4],
                 *__restrict__ a7 = L.cA[6], *__restrict__ a8 = L.cA[7], *__restrict__ zy = L.zy, *__restrict__ zx = L.zx;
    const long long o = (long long)i * L.plane, om = o - L.plane, op = o + L.plane;
    const double qrt = 0.25, zero = 0.0;
    // as in k_residual_mf: every request unconditional (rows past the top clamped to nz) and issued one step before its first use
    double pc_m = 0, pc_0, pc_p, pc_n, pjm_m = 0, pjm_0, pjm_p, pjm_n, pim_m = 0, pim_0, pim_p, pim_n, pjp_m = 0, pjp_0, pjp_p, pjp_n, pip_m = 0, pip_0, pip_p, pip_n;
    double zy_m = 0, zy_0, zy_p, zy_n, zx_m = 0, zx_0, zx_p, zx_n, a2_0, a2_p, a2_n;
    double zyjm, zyjp, zxim, zxip, a4o, a4jp, a7o, a7ip, zyjm_n, zyjp_n, zxim_n, zxip_n, a4o_n, a4jp_n, a7o_n, a7ip_n;
#define LOAD_WIN(q, PC, PJM, PIM, PJP, PIP, ZY, ZX, A2)                        \
  { const long long ro = (long long)(((q) <= nz ? (q) : nz) - 1) * RS;         \
    PC = p[o + ro + c]; LD_PAIR(p + o + ro + jm, PJM, PJP) PIM = p[om + ro + c]; PIP = p[op + ro + c]; \
    ZY = *(zy + o + ro + c); ZX = *(zx + o + ro + c); A2 = ld_rt(a2 + o + ro + c, stream); }
#define LOAD_ROWV(q, ZYJM, ZYJP, ZXIM, ZXIP, A4O, A4JP, A7O, A7IP)             \
  { const long long ro = (long long)(((q) <= nz ? (q) : nz) - 1) * RS, ko = o + ro + c; \
    LD_PAIR(zy + o + ro + jm, ZYJM, ZYJP) ZXIM = zx[om + ro + c]; ZXIP = zx[op + ro + c]; \
    A4O = *(a4 + ko); A4JP = a4[o + ro + jp]; A7O = *(a7 + ko); A7IP = a7[op + ro + c]; }
    const double d_first = a1[o + c], d_last = a1[o + (long long)(nz - 1) * RS + c];
    double e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0, e6 = 0, e7 = 0;
    if (REAL) { e0 = a5[o + c]; e1 = p[om + jp]; e2 = a5[op + jm]; e3 = p[op + jm]; e4 = a8[o + c]; e5 = p[om + jm]; e6 = a8[op + jp]; e7 = p[op + jp]; }
    LOAD_WIN(1, pc_0, pjm_0, pim_0, pjp_0, pip_0, zy_0, zx_0, a2_0)
    LOAD_ROWV(1, zyjm, zyjp, zxim, zxip, a4o, a4jp, a7o, a7ip)
    LOAD_WIN(2, pc_p, pjm_p, pim_p, pjp_p, pip_p, zy_p, zx_p, a2_p)
    for (int k = 1; k <= nz; k++) {
      const long long ro = (long long)(k - 1) * RS, ko = o + ro + c;
      LOAD_WIN(k + 2, pc_n, pjm_n, pim_n, pjp_n, pip_n, zy_n, zx_n, a2_n)
      LOAD_ROWV(k + 1, zyjm_n, zyjp_n, zxim_n, zxip_n, a4o_n, a4jp_n, a7o_n, a7ip_n)
      double rr;
      if (k == 1) {
        rr = zero - d_first * pc_0 - a2_p * pc_p - (qrt * (zy_p + zyjm)) * pjm_p - a4o * pjm_0 - a4jp * pjp_0
                   - (-qrt * (zyjp + zy_p)) * pjp_p - (qrt * (zx_p + zxim)) * pim_p - a7o * pim_0 - a7ip * pip_0
                   - (-qrt * (zxip + zx_p)) * pip_p;
        if (REAL) rr = rr - e0 * e1 - e2 * e3 - e4 * e5 - e6 * e7;
      } else if (k < nz) {
        const double c3 = qrt * (zy_p + zyjm), c3m = qrt * (zyjp + zy_m), c5 = -qrt * (zy_m + zyjm), c5m = -qrt * (zyjp + zy_p);
        const double c6 = qrt * (zx_p + zxim), c6m = qrt * (zxip + zx_m), c8 = -qrt * (zx_m + zxim), c8m = -qrt * (zxip + zx_p);
        const double dk = -a2_0 - a2_p - a4o - a4jp - a7o - a7ip - c6 - c6m - c8 - c8m - c3 - c3m - c5 - c5m;  // = cA(1,k,j,i), mg_define_matrix.f90:632-639
        rr = zero - dk * pc_0 - a2_0 * pc_m - a2_p * pc_p - c3 * pjm_p - c3m * pjp_m
                   - a4o * pjm_0 - a4jp * pjp_0 - c5 * pjm_m - c5m * pjp_p
                   - c6 * pim_p - c6m * pip_m - a7o * pim_0 - a7ip * pip_0
                   - c8 * pim_m - c8m * pip_p;
      } else {
        rr = zero - d_last * pc_0 - a2_0 * pc_m - (qrt * (zyjp + zy_m)) * pjp_m - a4o * pjm_0 - a4jp * pjp_0
                   - (-qrt * (zy_m + zyjm)) * pjm_m - (qrt * (zxip + zx_m)) * pip_m - a7o * pim_0 - a7ip * pip_0
                   - (-qrt * (zx_m + zxim)) * pim_m;
      }
      PUT_ROW(ko, rr)
      pc_m = pc_0; pc_0 = pc_p; pc_p = pc_n; pjm_m = pjm_0; pjm_0 = pjm_p; pjm_p = pjm_n; pim_m = pim_0; pim_0 = pim_p; pim_p = pim_n;
      pjp_m = pjp_0; pjp_0 = pjp_p; pjp_p = pjp_n; pip_m = pip_0; pip_0 = pip_p; pip_p = pip_n;
      zy_m = zy_0; zy_0 = zy_p; zy_p = zy_n; zx_m = zx_0; zx_0 = zx_p; zx_p = zx_n; a2_0 = a2_p; a2_p = a2_n;
      zyjm = zyjm_n; zyjp = zyjp_n; zxim = zxim_n; zxip = zxip_n; a4o = a4o_n; a4jp = a4jp_n; a7o = a7o_n; a7ip = a7ip_n;
    }
#undef LOAD_ROWV
#undef LOAD_WIN
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}
#undef PUT_ROW

// ------------------------------------------------------------------------------------------------
// streaming passes.  Grid: x = chunks of KR_CHUNK elements of a plane, y = the nx + 2 planes; a lane takes pairs of neighbouring elements
// (RS is a multiple of 16 doubles: every pair is 16-byte aligned and never straddles a row).
// ------------------------------------------------------------------------------------------------
#define KR_CHUNK 2048
// is element `pos` of a row of plane i an interior cell (j = 1..ny)?  odd j: HO .. HO + ny/2 - 1, even j: EO + 1 .. EO + ny/2
__device__ __forceinline__ bool kr_interior(const LevView &L, int i, int pos) {
  const int h = L.ny >> 1;
  return i >= 1 && i <= L.nx && ((pos >= L.HO && pos < L.HO + h) || (pos > L.EO && pos <= L.EO + h));
}

// 2. orthogonalise (z, q) against the retained pairs; s = (q, q), t = (r, q) of the result.  sc[0..n-1] = (q, q_i), qq[slot_i] = (q_i, q_i)
__global__ __launch_bounds__(256) void k_kr_ortho(LevView L, double *__restrict__ z, double *__restrict__ q, const double *__restrict__ r, KrDirs D,
                                                  const double *__restrict__ sc, const double *__restrict__ qq, double *__restrict__ partial, int stream) {
  double beta[KR_MAX];
#pragma unroll
  for (int n = 0; n < KR_MAX; n++) beta[n] = n < D.n ? sc[n] / qq[D.slot[n]] : 0.0;
  const int i = blockIdx.y;
  const long long base = (long long)i * L.plane;
  const int e0 = blockIdx.x * KR_CHUNK, e1 = min(e0 + KR_CHUNK, (int)L.plane);
  double acc[2] = {0, 0};
  for (int e = e0 + 2 * (int)threadIdx.x; e < e1; e += 512) {
    const long long g = base + e;
    d2_t qv = ld2(q + g, stream), zv = ld2(z + g, stream);
    const d2_t rv = ld2(r + g, stream);
#pragma unroll
    for (int n = 0; n < KR_MAX; n++)
      if (n < D.n) { const d2_t qi = ld2(D.q[n] + g, stream), zi = ld2(D.z[n] + g, stream); qv = qv - beta[n] * qi; zv = zv - beta[n] * zi; }
    st2(q + g, qv, stream); st2(z + g, zv, stream);
    const int pos = e % L.RS;
    if (kr_interior(L, i, pos)) { acc[0] = acc[0] + qv.x * qv.x; acc[1] = acc[1] + rv.x * qv.x; }
    if (kr_interior(L, i, pos + 1)) { acc[0] = acc[0] + qv.y * qv.y; acc[1] = acc[1] + rv.y * qv.y; }
  }
  kr_block_sums<2>(acc, 2, partial, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
}

// a step is taken only with usable scalars: s > 0 and s, t finite (s == 0: q vanished; anything else: the cycle produced a non-number)
__device__ __forceinline__ bool kr_step_ok(double s, double t) { return s > 0.0 && s <= 1.79769313486231570e308 && t == t && fabs(t) <= 1.79769313486231570e308; }

// 3. p += alpha z, r -= alpha q, partial sums of r^2; alpha = t / s, st = {s, t}.  No step with unusable scalars: p and r stay as they are.
// Workgroup (0, 0) files s under the slot of the new pair (qq_new) for the orthogonalisations to come.
__global__ __launch_bounds__(256) void k_kr_update(LevView L, double *__restrict__ p, double *__restrict__ r, const double *__restrict__ z, const double *__restrict__ q,
                                                   const double *__restrict__ st, double *__restrict__ qq_new, double *__restrict__ partial, int stream) {
  const double s = st[0], t = st[1];
  const bool ok = kr_step_ok(s, t);
  const double alpha = ok ? t / s : 0.0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *qq_new = s;
  const int i = blockIdx.y;
  const long long base = (long long)i * L.plane;
  const int e0 = blockIdx.x * KR_CHUNK, e1 = min(e0 + KR_CHUNK, (int)L.plane);
  double acc[1] = {0};
  for (int e = e0 + 2 * (int)threadIdx.x; e < e1; e += 512) {
    const long long g = base + e;
    d2_t rv = ld2(r + g, stream);
    if (ok) {
      d2_t pv = ld2(p + g, stream);
      const d2_t zv = ld2(z + g, stream), qv = ld2(q + g, stream);
      pv = pv + alpha * zv; rv = rv - alpha * qv;
      st2(p + g, pv, stream); st2(r + g, rv, stream);
    }
    const int pos = e % L.RS;
    if (kr_interior(L, i, pos)) acc[0] = acc[0] + rv.x * rv.x;
    if (kr_interior(L, i, pos + 1)) acc[0] = acc[0] + rv.y * rv.y;
  }
  kr_block_sums<1>(acc, 1, partial, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
}

// second stage: workgroup v sums partial[v * n .. v * n + n - 1] in the order of k_reduce_partials -> out[v].
// guard != nullptr (the norm of pass 3): out[0] = -1 when the step's scalars guard[0..1] were unusable, which the host reads as "no step was taken"
__global__ __launch_bounds__(256) void k_kr_reduce(const double *__restrict__ partial, int n, double *__restrict__ out, const double *__restrict__ guard) {
  __shared__ double red[256];
  const double *__restrict__ pv = partial + (long long)blockIdx.x * n;
  double s = 0.0;
  for (int q = threadIdx.x; q < n; q += 256) s += pv[q];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (guard && !kr_step_ok(guard[0], guard[1])) ? -1.0 : red[0];
}

extern "C" {

static dim3 kr_stream_grid(const LevView *L) { return dim3((unsigned)((L->plane + KR_CHUNK - 1) / KR_CHUNK), (unsigned)(L->nx + 2)); }
// doubles the partial-sum buffer of a level needs: KR_MAX values per workgroup of pass 1, two per workgroup of pass 2
long long mgxq_partials(const LevView *L) {
  const dim3 g3 = col_grid(L->ny / 2, L->nx, 2), gs = kr_stream_grid(L);
  const long long a = (long long)KR_MAX * g3.x * g3.y * 2, b = 2LL * gs.x * gs.y;
  return a > b ? a : b;
}
// which launch the wrappers below choose for a level (reported by the test hook mgx_krylov_op): out[0] = pass 1 matrix-free (1) or from the
// stored slots (0), out[1] = the non-temporal variant of all three passes, out[2] = gx, out[3] = gy of pass 1's block map
void mgxq_path(const LevView *L, int *out) {
  const dim3 g3 = col_grid(L->ny / 2, L->nx, 2);
  out[0] = L->zy != nullptr && L->nz >= 3; out[1] = level_streams(L); out[2] = (int)g3.x; out[3] = (int)g3.y;
}
// q = A z (z = L->p, halos valid), sc[i] = (q, q_i) for the nd retained q_i
void mgxq_apply(hipStream_t st, const LevView *L, double *qout, const double *const *qi, int nd, double *partial, double *sc, int real) {
  KrDirs D = {};
  D.n = nd;
  for (int n = 0; n < nd; n++) D.q[n] = qi[n];
  dim3 blk(WAVE, 4), g3 = col_grid(L->ny / 2, L->nx, 2), grd(g3.x * g3.y * 2);
  const int gx = g3.x, gy = g3.y, nt = level_streams(L);
  if (L->zy != nullptr && L->nz >= 3) {
    if (real) hipLaunchKernelGGL((k_kr_apply_mf<true>), grd, blk, 0, st, *L, qout, D, partial, gx, gy, nt);
    else hipLaunchKernelGGL((k_kr_apply_mf<false>), grd, blk, 0, st, *L, qout, D, partial, gx, gy, nt);
  } else if (real) hipLaunchKernelGGL((k_kr_apply<true>), grd, blk, 0, st, *L, qout, D, partial, gx, gy, nt);
  else hipLaunchKernelGGL((k_kr_apply<false>), grd, blk, 0, st, *L, qout, D, partial, gx, gy, nt);
  if (nd) hipLaunchKernelGGL(k_kr_reduce, dim3(nd), dim3(256), 0, st, partial, (int)grd.x, sc, (const double *)nullptr);
}
// (z, q) orthogonalised against the nd retained pairs; out[0] = (q, q), out[1] = (r, q)
void mgxq_ortho(hipStream_t st, const LevView *L, double *z, double *q, const double *r, const double *const *zi, const double *const *qi, const int *slot, int nd,
                const double *sc, const double *qq, double *partial, double *out) {
  KrDirs D = {};
  D.n = nd;
  for (int n = 0; n < nd; n++) { D.q[n] = qi[n]; D.z[n] = zi[n]; D.slot[n] = slot[n]; }
  const dim3 grd = kr_stream_grid(L);
  hipLaunchKernelGGL(k_kr_ortho, grd, dim3(256), 0, st, *L, z, q, r, D, sc, qq, partial, level_streams(L));
  hipLaunchKernelGGL(k_kr_reduce, dim3(2), dim3(256), 0, st, partial, (int)(grd.x * grd.y), out, (const double *)nullptr);
}
// p += (t / s) z, r -= (t / s) q with st2 = {s, t}; out[0] = ||r||^2 over the interior, or -1 when no step could be taken; *qq_new = s
void mgxq_update(hipStream_t st, const LevView *L, double *p, double *r, const double *z, const double *q, const double *st2v, double *qq_new,
                 double *partial, double *out) {
  const dim3 grd = kr_stream_grid(L);
  hipLaunchKernelGGL(k_kr_update, grd, dim3(256), 0, st, *L, p, r, z, q, st2v, qq_new, partial, level_streams(L));
  hipLaunchKernelGGL(k_kr_reduce, dim3(1), dim3(256), 0, st, partial, (int)(grd.x * grd.y), out, st2v);
}

}
