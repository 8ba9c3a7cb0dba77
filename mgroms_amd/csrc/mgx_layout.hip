// Layout conversions between the reference layout (k,j,i), k fastest, and JS (mgx_internal.h), and the self-test of the constant-divisor quotient.
#include "mgx_device.h"

// ------------------------------------------------------------------------------------------------
// layout conversion between the reference layout (k,j,i) k fastest and JS.  dir 0: ref -> JS, 1: JS -> ref
// ------------------------------------------------------------------------------------------------
__global__ void k_convert(LevView L, double *__restrict__ js, double *__restrict__ ref, int nslot, int slot, int dir) {
  const long long n = (long long)L.nz * (L.ny + 2) * (L.nx + 2);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int k = (int)(t % L.nz);
  const long long ji = t / L.nz;
  const int j = (int)(ji % (L.ny + 2)), i = (int)(ji / (L.ny + 2));
  const long long e = (long long)i * L.plane + (long long)k * L.RS + jpos(L, j);
  if (dir == 0) js[e] = ref[t * nslot + slot]; else ref[t * nslot + slot] = js[e];
}

// Set-up scratch -> JS for NS slot-major arrays (nz, 0:ny+1, 0:nx+1) at ref, ref + n3, ... (the eight coefficient slots; the two slope
// arrays).  A block takes one slot (blockIdx.z), one plane and TJ consecutive columns: one contiguous run of TJ*nz doubles, staged in
// LDS with the even and the odd columns apart ([parity][column pair][k], column stride padded by one double), then written row by row:
// for every k one wave stores TJ/2 consecutive even-j entries and one TJ/2 consecutive odd-j entries -- 512-byte runs at TJ = 128
// (the first version moved all eight slots of 16 columns per block: 64-byte runs, 2.1 TB/s at 512x512x64).
struct Slots8 { double *s[8]; };
__global__ __launch_bounds__(256) void k_convert_slots(LevView L, Slots8 out, const double *__restrict__ ref, int TJ) {
  extern __shared__ double lds[];
  const int nz = L.nz, cs = nz + 1, H = (TJ >> 1) * cs;
  const int i = blockIdx.y, j0 = blockIdx.x * TJ, sl = blockIdx.z;
  const int nj = min(TJ, L.ny + 2 - j0);
  const long long n3 = (long long)nz * (L.ny + 2) * (L.nx + 2);
  const double *__restrict__ src = ref + (long long)sl * n3 + ((long long)i * (L.ny + 2) + j0) * nz;
  const int run = nj * nz;
  const bool p2 = (nz & (nz - 1)) == 0;
  const int lz = 31 - __builtin_clz(nz);
  // eight loads in flight per thread before the first LDS store (one load per iteration made the block a chain of 32 memory round trips)
  constexpr int U = 8;
  const int nt = blockDim.x;
  for (int r0 = threadIdx.x; r0 < run; r0 += U * nt) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int r = r0 + u * nt; v[u] = r < run ? src[r] : 0.0; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int r = r0 + u * nt;
      if (r < run) { const int jl = p2 ? (r >> lz) : r / nz, k = r - jl * nz; lds[(jl & 1) * H + (jl >> 1) * cs + k] = v[u]; }
    }
  }
  __syncthreads();
  double *__restrict__ os = out.s[sl] + (long long)i * L.plane;
  const int hj = TJ >> 1;  // column pairs per tile; j0 is even (TJ is), so local parity = global parity
  for (int t = threadIdx.x; t < TJ * nz; t += nt) {
    const int q = t % hj, par = (t / hj) & 1, k = t / TJ;
    const int jl = 2 * q + par;
    if (jl < nj) os[(long long)k * L.RS + (par ? L.HO : L.EO) + ((j0 + jl) >> 1)] = lds[par * H + q * cs + k];
  }
}

// self-test of the constant-divisor quotient (mgx_device.h, DIVC): a / b by the hardware sequence against the refined-reciprocal form
__global__ void k_divc_selftest(const double *__restrict__ a, const double *__restrict__ b, int n, unsigned long long *bad) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double q = a[t] / b[t], rb = RCP_REF(b[t]), c = DIVC(a[t], b[t], rb);
  if (__double_as_longlong(q) != __double_as_longlong(c)) atomicAdd(bad, 1ull);
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
extern "C" {

void mgxk_divc_selftest(hipStream_t st, const double *a, const double *b, int n, unsigned long long *bad) {
  hipLaunchKernelGGL(k_divc_selftest, dim3((n + 255) / 256), dim3(256), 0, st, a, b, n, bad);
}
void mgxk_convert(hipStream_t st, const LevView *L, double *js, double *ref, int nslot, int slot, int dir) {
  const long long n = (long long)L->nz * (L->ny + 2) * (L->nx + 2);
  hipLaunchKernelGGL(k_convert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *L, js, ref, nslot, slot, dir);
}
static void convert_slots(hipStream_t st, const LevView *L, const Slots8 &o, int ns, const double *ref) {
  const ConvChoice c = choose_convert_slots(lev_shape(L));
  // > 64 KB from nz = 64 on; a refusal shows up as a launch error at the next synchronising call (sync_stream)
  static bool attr = false;
  // a refused attribute makes the launch below fail, and THAT is reported by the next synchronising call; the attribute call's own status is consumed here
  if (!attr) { if (hipFuncSetAttribute((const void *)k_convert_slots, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void)hipGetLastError(); attr = true; }
  hipLaunchKernelGGL(k_convert_slots, dim3(c.gx, c.gy, ns), dim3(256), c.lds, st, *L, o, ref, c.tj);
}
void mgxk_convert8(hipStream_t st, const LevView *L, const double *ref) {
  Slots8 o;
  for (int q = 0; q < 8; q++) o.s[q] = L->cA[q];
  convert_slots(st, L, o, 8, ref);
}
// two slot-major arrays (nz, 0:ny+1, 0:nx+1) at ref, ref + n3 -> the JS arrays out0, out1 (the slopes zy, zx)
void mgxk_convert2(hipStream_t st, const LevView *L, double *out0, double *out1, const double *ref) {
  Slots8 o;
  for (int q = 0; q < 8; q++) o.s[q] = nullptr;
  o.s[0] = out0; o.s[1] = out1;
  convert_slots(st, L, o, 2, ref);
}

}  // extern "C"
