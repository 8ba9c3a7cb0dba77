// Kernels of the Krylov-accelerated solve_p (option "krylov" = m, mgx_cycle.cpp: solve_p_krylov) for gfx950 (MI355X): truncated GCR /
// Orthomin(m) around the F-cycle.  Three launches per iteration on level 1, each followed by a one-launch reduction of its per-workgroup
// partial sums in index order (the order of k_reduce_partials, mgx_residual.hip): a solve is reproducible run to run.
//   1. k_kr_apply[_mf]: q = A z and the inner products (q, q_i) with the retained q_i
//   2. k_kr_ortho:      q -= sum beta_i q_i, z -= sum beta_i z_i (beta_i = (q, q_i) / (q_i, q_i)), s = (q, q), t = (r, q)
//   3. k_kr_update:     p += (t / s) z, r -= (t / s) q, ||r||^2
// The scalars stay in device memory between the launches (kernels 2 and 3 read them there).  Pass 1 is the column text of k_residual /
// k_residual_mf itself (mgx_operator.h) with the right-hand side 0 and each row negated on its way out: q is the negative of what
// compute_residual writes for b = 0 because both are compiled from that one text.  Kernels 2 and 3 are streaming passes over WHOLE arrays
// (halo and padding included: z and p keep consistent halos by linearity, q and r are zero / untouched there) with 16-byte accesses; only
// interior cells enter the sums.
// With an fp32 preconditioner (option "krylov_precision" = 32) passes 1 and 3 are k_kr_apply32[_mf] and k_kr_update32: the same passes with
// the promotion of the cycle's fp32 result and the demotion of the next cycle's right-hand side folded in (no conversion launch of their own).
#include "mgx_operator.h"

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

// ------------------------------------------------------------------------------------------------
// 1. q = A z, z = L.p with valid halos: the operator's column (mgx_operator.h) on the right-hand side 0; a row goes, negated, to q and
// into the products with the retained q_i.  From the stored slots, or matrix-free.
// ------------------------------------------------------------------------------------------------
#define KR_RHS(ko) zero
#define KR_SINK(ro, ko, rr)                                                    \
  { const double qv = -(rr);                                                   \
    st_rt(qout + (ko), qv, stream);                                            \
    _Pragma("unroll") for (int n = 0; n < KR_MAX; n++) if (n < D.n) acc[n] = acc[n] + qv * D.q[n][ko]; }
template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply(LevView L, double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const double zero = 0.0;
    OP_COLUMN(OP_P, KR_RHS, KR_SINK)
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}

template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply_mf(LevView L, double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    const double zero = 0.0;
    OP_COLUMN_MF(OP_P, OP_P2, KR_RHS, KR_SINK)
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// 1 with an fp32 preconditioner (option "krylov_precision" = 32): the cycle's result e sits in the level's fp32 shadow S, and
// z = (double)e * isg (isg = 1 / sigma, f = sigma r having been the cycle's right-hand side) is formed here instead of in a pass of its
// own: ONE correctly rounded multiplication per value, the one k_to64 (mgx_mixed.hip) makes.  The operator text reads every p through
// KR32_P / KR32_P2, which promote e on the fly -- the own column and the neighbours other lanes own alike, so nobody reads z back -- and
// find it in the shadow's layout by the names of the text's index parts (s_o / s_om / s_op, s_c / s_jm / s_jp, row kr of s_RS floats).
// The sink stores the row's z (pc_0, the text's own-column value) with q; the lane of a column on the rim stores the promoted halo cells
// next to it as well (the cells mirror32 images): z is written whole, every cell once, as k_to64 writes it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double kr_promote(float e, double isg) { return __dmul_rn((double)e, isg); }
#define KR32_P(pl, ro, kr, pos) kr_promote(ef[s_##pl + (long long)(kr) * s_RS + s_##pos], isg)
#define KR32_P2(pl, ro, kr, pos, A, B) { float2 t2_; __builtin_memcpy(&t2_, ef + s_##pl + (long long)(kr) * s_RS + s_##pos, 8); A = kr_promote(t2_.x, isg); B = kr_promote(t2_.y, isg); }
// the halo cells beside column (j, i), promoted into z: row offsets ro (fp64 layout) and sro (shadow)
__device__ __forceinline__ void kr_promote_rim(const LevView &L, const LevView32 &S, const float *__restrict__ ef, double *__restrict__ zout, const double isg,
                                               const long long ro, const long long sro, const int j, const int i, const int c, const int sc) {
  const bool mS = j == 1, mN = j == L.ny, mW = i == 1, mE = i == L.nx;
  if (!(mS | mN | mW | mE)) return;
  const int cS = L.EO, cN = jpos(L, L.ny + 1), sS = S.EO, sN = jpos32(S, L.ny + 1);
  const long long o = (long long)i * L.plane + ro, oW = ro, oE = (long long)(L.nx + 1) * L.plane + ro;
  const long long so = (long long)i * S.plane + sro, sW = sro, sE = (long long)(L.nx + 1) * S.plane + sro;
  if (mS) zout[o + cS] = kr_promote(ef[so + sS], isg);
  if (mN) zout[o + cN] = kr_promote(ef[so + sN], isg);
  if (mW) { zout[oW + c] = kr_promote(ef[sW + sc], isg); if (mS) zout[oW + cS] = kr_promote(ef[sW + sS], isg); if (mN) zout[oW + cN] = kr_promote(ef[sW + sN], isg); }
  if (mE) { zout[oE + c] = kr_promote(ef[sE + sc], isg); if (mS) zout[oE + cS] = kr_promote(ef[sE + sS], isg); if (mN) zout[oE + cN] = kr_promote(ef[sE + sN], isg); }
}
#define KR32_SINK(ro, ko, rr)                                                  \
  { st_rt(zout + (ko), pc_0, stream);                                          \
    kr_promote_rim(L, S, ef, zout, isg, ro, s_ro, jc, i, c, s_c);              \
    s_ro += s_RS;                                                              \
    KR_SINK(ro, ko, rr) }
// the shadow's counterparts of the text's o, om, op, c, jm, jp and RS
#define KR32_POS(S, i, jh, jodd)                                                                         \
  const long long s_RS = S.RS, s_o = (long long)i * S.plane, s_om = s_o - S.plane, s_op = s_o + S.plane; \
  const int s_c = jodd ? S.HO + jh : S.EO + jh + 1, s_jm = jodd ? S.EO + jh : S.HO + jh, s_jp = s_jm + 1; \
  const int jc = jodd ? 2 * jh + 1 : 2 * jh + 2;                                                         \
  long long s_ro = 0;
template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply32(LevView L, LevView32 S, const float *__restrict__ ef, double isg, double *__restrict__ zout,
                                                    double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    KR32_POS(S, i, jh, jodd)
    const double zero = 0.0;
    OP_COLUMN(KR32_P, KR_RHS, KR32_SINK)
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}

template <bool REAL>
__global__ __launch_bounds__(256) void k_kr_apply32_mf(LevView L, LevView32 S, const float *__restrict__ ef, double isg, double *__restrict__ zout,
                                                       double *__restrict__ qout, KrDirs D, double *__restrict__ partial, int gx, int gy, int stream) {
  int bx, by, bz;
  op_block_map(gx, gy, bx, by, bz);
  const int jh = bx * WAVE + threadIdx.x;
  const int i = 1 + by * blockDim.y + threadIdx.y;
  const int jodd = bz == 0;
  double acc[KR_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (jh < (L.ny >> 1) && i <= L.nx) {
    int c, jm, jp;
    COL_POS(L, jh, jodd, c, jm, jp)
    KR32_POS(S, i, jh, jodd)
    const double zero = 0.0;
    OP_COLUMN_MF(KR32_P, KR32_P2, KR_RHS, KR32_SINK)
  }
  if (D.n) kr_block_sums<KR_MAX>(acc, D.n, partial, blockIdx.x, gridDim.x);
}

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

// where element `pos` of a row sits in a row of the fp32 shadow (EO / HO differ, mgx_internal.h), or -1 for the padding between the half-rows.
// Even positions go to even positions (EO and EO32 are odd, HO and HO32 even): a pair that stays inside a half-row stays an aligned pair.
__device__ __forceinline__ int kr_pos32(const LevView &L, const LevView32 &S, int pos) {
  const int h = L.ny >> 1;
  if (pos >= L.HO) return pos <= L.HO + h ? pos - L.HO + S.HO : -1;
  return (pos >= L.EO && pos <= L.EO + h) ? pos - L.EO + S.EO : -1;
}

// 3 with an fp32 preconditioner: k_kr_update, and in the same sweep the next cycle's right-hand side f = (float)(sigma r_new) into the fp32
// shadow (the conversion k_to32 makes, at the index map above; halo cells as k_to32 converts them).  st = {s, t}.  No step: p, r and f stay.
// f keeps the default cache policy whatever the level's: the cycle's first kernel reads it next, and it is a twelfth of this pass's traffic.
__global__ __launch_bounds__(256) void k_kr_update32(LevView L, LevView32 S, double *__restrict__ p, double *__restrict__ r, const double *__restrict__ z,
                                                     const double *__restrict__ q, float *__restrict__ f, double sigma, const double *__restrict__ st,
                                                     double *__restrict__ qq_new, double *__restrict__ partial, int stream) {
  const double s = st[0], t = st[1];
  const bool ok = kr_step_ok(s, t);
  const double alpha = ok ? t / s : 0.0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *qq_new = s;
  const int i = blockIdx.y;
  const long long base = (long long)i * L.plane, base32 = (long long)i * S.plane;
  const int e0 = blockIdx.x * KR_CHUNK, e1 = min(e0 + KR_CHUNK, (int)L.plane);
  double acc[1] = {0};
  for (int e = e0 + 2 * (int)threadIdx.x; e < e1; e += 512) {
    const long long g = base + e;
    d2_t rv = ld2(r + g, stream);
    const int row = e / L.RS, pos = e - row * L.RS;
    if (ok) {
      d2_t pv = ld2(p + g, stream);
      const d2_t zv = ld2(z + g, stream), qv = ld2(q + g, stream);
      pv = pv + alpha * zv; rv = rv - alpha * qv;
      st2(p + g, pv, stream); st2(r + g, rv, stream);
      const int m0 = kr_pos32(L, S, pos), m1 = kr_pos32(L, S, pos + 1);
      float *__restrict__ fr = f + base32 + (long long)row * S.RS;
      const float f0 = (float)(rv.x * sigma), f1 = (float)(rv.y * sigma);
      if (m0 >= 0 && m1 == m0 + 1) *(float2 *)(fr + m0) = make_float2(f0, f1);
      else { if (m0 >= 0) fr[m0] = f0; if (m1 >= 0) fr[m1] = f1; }
    }
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

static dim3 kr_stream_grid(const LevView *L) { const KrChoice c = choose_kr_stream(lev_shape(L)); return dim3(c.gx, c.gy); }
static_assert(KR_CHUNK == CH_KR_CHUNK, "the grid of passes 2 and 3 is sized by the chunk their kernels walk");
// doubles the partial-sum buffer of a level needs: KR_MAX values per workgroup of pass 1, two per workgroup of pass 2
long long mgxq_partials(const LevView *L) {
  const KrChoice gs = choose_kr_stream(lev_shape(L));
  const long long a = (long long)KR_MAX * choose_operator(lev_shape(L)).grid, b = 2LL * gs.gx * gs.gy;
  return a > b ? a : b;
}
// which launch the wrappers below choose for a level (reported by the test hook mgx_krylov_op): out[0] = pass 1 matrix-free (1) or from the
// stored slots (0), out[1] = the non-temporal variant of all three passes, out[2] = gx, out[3] = gy of pass 1's block map
void mgxq_path(const LevView *L, int *out) {
  const OpChoice c = choose_operator(lev_shape(L));
  out[0] = c.mf; out[1] = c.stream; out[2] = c.gx; out[3] = c.gy;
}
static KrDirs kr_dirs(const double *const *qi, int nd) {
  KrDirs D = {};
  D.n = nd;
  for (int n = 0; n < nd; n++) D.q[n] = qi[n];
  return D;
}
// q = A z (z = L->p, halos valid), sc[i] = (q, q_i) for the nd retained q_i
void mgxq_apply(hipStream_t st, const LevView *L, double *qout, const double *const *qi, int nd, double *partial, double *sc, int real) {
  const KrDirs D = kr_dirs(qi, nd);
  const OpChoice c = choose_operator(lev_shape(L));
  op_launch(c, real, [&](auto MF, auto REAL) {
    if constexpr (MF()) hipLaunchKernelGGL((k_kr_apply_mf<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, qout, D, partial, c.gx, c.gy, c.stream);
    else hipLaunchKernelGGL((k_kr_apply<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, qout, D, partial, c.gx, c.gy, c.stream);
  });
  if (nd) hipLaunchKernelGGL(k_kr_reduce, dim3(nd), dim3(256), 0, st, partial, (int)c.grid, sc, (const double *)nullptr);
}
// the same from the cycle's fp32 result: z = (double)e * isg written whole into zout, q = A z, sc[i] = (q, q_i); e = S->e
void mgxq_apply32(hipStream_t st, const LevView *L, const LevView32 *S, double isg, double *zout, double *qout, const double *const *qi, int nd, double *partial,
                  double *sc, int real) {
  const KrDirs D = kr_dirs(qi, nd);
  const OpChoice c = choose_operator(lev_shape(L));
  op_launch(c, real, [&](auto MF, auto REAL) {
    if constexpr (MF()) hipLaunchKernelGGL((k_kr_apply32_mf<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, *S, S->e, isg, zout, qout, D, partial, c.gx, c.gy, c.stream);
    else hipLaunchKernelGGL((k_kr_apply32<REAL()>), dim3(c.grid), OP_BLOCK, 0, st, *L, *S, S->e, isg, zout, qout, D, partial, c.gx, c.gy, c.stream);
  });
  if (nd) hipLaunchKernelGGL(k_kr_reduce, dim3(nd), dim3(256), 0, st, partial, (int)c.grid, sc, (const double *)nullptr);
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
// the same, and S->f = (float)(sigma r) of the new r
void mgxq_update32(hipStream_t st, const LevView *L, const LevView32 *S, double *p, double *r, const double *z, const double *q, double sigma, const double *st2v,
                   double *qq_new, double *partial, double *out) {
  const dim3 grd = kr_stream_grid(L);
  hipLaunchKernelGGL(k_kr_update32, grd, dim3(256), 0, st, *L, *S, p, r, z, q, S->f, sigma, st2v, qq_new, partial, level_streams(L));
  hipLaunchKernelGGL(k_kr_reduce, dim3(1), dim3(256), 0, st, partial, (int)(grd.x * grd.y), out, st2v);
}

}
