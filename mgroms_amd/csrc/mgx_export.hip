// The CSR export of a level's operator and transfers (include/mgx.h: mgx_operator_csr, mgx_transfer_csr): the kernels around the probes.
// The host (mgx_api.cpp: export_csr) writes the 0/1 pattern of one colour into a level field (k_probe_fill), fills its halo with the level's
// own fill, applies the library's own residual / fine2coarse / coarse2fine, and hands the result to k_csr_mark (first sweep over the colours:
// which colours a row answers to) or k_csr_scatter (second sweep: the entries, sorted by column).  Between the sweeps the rows' counts are
// scanned into rowptr (k_csr_sums, k_csr_scan_sums, k_csr_rowptr).  mgx_export.h holds the geometry -- which cells share a colour and which
// column a colour means in a row -- in one text for these kernels and for the host test.
// One lane owns a row throughout: no atomics, no waits between workgroups.  Rows run k-fastest (the index convention of the export), so the
// mask, rowptr, col and val accesses are unit-stride; the level field is read through the JS layout at whatever stride that gives.  None of
// this is a hot path: an export costs a few dozen operator applications.
#include "mgx_device.h"
#include "mgx_export.h"

// cell (k, j, i) of row index t on a level of ny x nz columns
__device__ __forceinline__ void ex_cell(long long t, int ny, int nz, int &k, int &j, int &i) {
  k = (int)(t % nz) + 1;
  const long long c = t / nz;
  j = (int)(c % ny) + 1;
  i = (int)(c / ny) + 1;
}
__device__ __forceinline__ long long ex_js(const LevView &L, int k, int j, int i) { return (long long)i * L.plane + (long long)(k - 1) * L.RS + jpos(L, j); }

// the probe of one colour: a one in every interior cell of that colour, a zero in the others (L: the COLUMN level of the map; halos: the caller's fill)
__global__ __launch_bounds__(EX_BLOCK) void k_probe_fill(LevView L, double *__restrict__ a, ExMap m, int colour) {
  const long long t = (long long)blockIdx.x * EX_BLOCK + threadIdx.x;
  if (t >= (long long)L.nx * L.ny * L.nz) return;
  int k, j, i;
  ex_cell(t, L.ny, L.nz, k, j, i);
  a[ex_js(L, k, j, i)] = ex_cell_colour(m, k, j, i) == colour ? 1.0 : 0.0;
}

// first sweep: row t answers to this colour where the probed value is not zero (L: the ROW level, a: the field the operator wrote)
__global__ __launch_bounds__(EX_BLOCK) void k_csr_mark(LevView L, const double *__restrict__ a, ExMap m, int colour, unsigned long long *__restrict__ mask) {
  const long long t = (long long)blockIdx.x * EX_BLOCK + threadIdx.x;
  if (t >= (long long)L.nx * L.ny * L.nz) return;
  int k, j, i;
  ex_cell(t, L.ny, L.nz, k, j, i);
  if (a[ex_js(L, k, j, i)] != 0.0 && ex_column(m, k, j, i, colour) >= 0) mask[t] |= 1ULL << colour;
}

// entries of row t (0 for t = n: the scan runs over n + 1 entries so that rowptr[n] comes out as nnz)
__device__ __forceinline__ int ex_count(const unsigned long long *__restrict__ mask, long long t, long long n) { return t < n ? __popcll(mask[t]) : 0; }
// the sum over the workgroup of one value per lane, and the lane's exclusive prefix (EX_BLOCK lanes)
__device__ __forceinline__ long long ex_block_scan(long long v, long long &total) {
  __shared__ long long sh[EX_BLOCK];
  const int l = threadIdx.x;
  sh[l] = v;
  __syncthreads();
  for (int d = 1; d < EX_BLOCK; d <<= 1) {
    const long long u = l >= d ? sh[l - d] : 0;
    __syncthreads();
    sh[l] += u;
    __syncthreads();
  }
  total = sh[EX_BLOCK - 1];
  const long long ex = sh[l] - v;
  __syncthreads();
  return ex;
}
// the entries of each workgroup's EX_SCAN_ROWS rows
__global__ __launch_bounds__(EX_BLOCK) void k_csr_sums(const unsigned long long *__restrict__ mask, long long n, long long *__restrict__ sums) {
  const long long t0 = ((long long)blockIdx.x * EX_BLOCK + threadIdx.x) * EX_SCAN_ITEMS;
  long long v = 0;
  for (int q = 0; q < EX_SCAN_ITEMS; q++) v += ex_count(mask, t0 + q, n);
  long long total;
  ex_block_scan(v, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[0 .. nb-1] become their exclusive prefixes, sums[nb] the total (= nnz)
__global__ __launch_bounds__(EX_BLOCK) void k_csr_scan_sums(long long *__restrict__ sums, int nb) {
  long long carry = 0;
  for (int b0 = 0; b0 < nb; b0 += EX_BLOCK) {
    const int b = b0 + threadIdx.x;
    const long long v = b < nb ? sums[b] : 0;
    long long total;
    const long long ex = ex_block_scan(v, total);
    if (b < nb) sums[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}
// rowptr[0 .. n] from the workgroups' prefixes (the caller has checked that nnz fits an int)
__global__ __launch_bounds__(EX_BLOCK) void k_csr_rowptr(const unsigned long long *__restrict__ mask, long long n, const long long *__restrict__ sums, int *__restrict__ rowptr) {
  const long long t0 = ((long long)blockIdx.x * EX_BLOCK + threadIdx.x) * EX_SCAN_ITEMS;
  int cnt[EX_SCAN_ITEMS];
  long long v = 0;
  for (int q = 0; q < EX_SCAN_ITEMS; q++) { cnt[q] = ex_count(mask, t0 + q, n); v += cnt[q]; }
  long long total;
  long long off = sums[blockIdx.x] + ex_block_scan(v, total);
  for (int q = 0; q < EX_SCAN_ITEMS; q++) {
    if (t0 + q <= n) rowptr[t0 + q] = (int)off;
    off += cnt[q];
  }
}

// second sweep: the entry of this colour in row t goes to the slot its column has among the row's columns; sign = -1 for A (r = b - A p)
__global__ __launch_bounds__(EX_BLOCK) void k_csr_scatter(LevView L, const double *__restrict__ a, ExMap m, int colour, const unsigned long long *__restrict__ mask,
                                                          const int *__restrict__ rowptr, int *__restrict__ col, double *__restrict__ val, double sign) {
  const long long t = (long long)blockIdx.x * EX_BLOCK + threadIdx.x;
  if (t >= (long long)L.nx * L.ny * L.nz) return;
  const unsigned long long bits = mask[t];
  if (!(bits >> colour & 1ULL)) return;
  int k, j, i;
  ex_cell(t, L.ny, L.nz, k, j, i);
  const long long mine = ex_column(m, k, j, i, colour);
  int slot = 0;
  for (unsigned long long rest = bits & ~(1ULL << colour); rest; rest &= rest - 1) slot += ex_column(m, k, j, i, __ffsll((long long)rest) - 1) < mine;
  const long long at = (long long)rowptr[t] + slot;
  col[at] = (int)mine;
  val[at] = sign * a[ex_js(L, k, j, i)];
}

extern "C" {

void mgxe_probe_fill(hipStream_t st, const LevView *L, double *a, const ExMap *m, int colour) {
  const ExChoice c = choose_export((long long)L->nx * L->ny * L->nz);
  hipLaunchKernelGGL(k_probe_fill, dim3(c.grid_rows), dim3(c.block), 0, st, *L, a, *m, colour);
}
void mgxe_csr_mark(hipStream_t st, const LevView *L, const double *a, const ExMap *m, int colour, unsigned long long *mask) {
  const ExChoice c = choose_export((long long)L->nx * L->ny * L->nz);
  hipLaunchKernelGGL(k_csr_mark, dim3(c.grid_rows), dim3(c.block), 0, st, *L, a, *m, colour, mask);
}
// sums: mgxe_csr_sums_len(n) long longs; afterwards sums[mgxe_csr_sums_len(n) - 1] = nnz.  Two launches.
int mgxe_csr_sums_len(long long n) { return (int)choose_export(n).grid_scan + 1; }
void mgxe_csr_count(hipStream_t st, const unsigned long long *mask, long long n, long long *sums) {
  const ExChoice c = choose_export(n);
  hipLaunchKernelGGL(k_csr_sums, dim3(c.grid_scan), dim3(c.block), 0, st, mask, n, sums);
  hipLaunchKernelGGL(k_csr_scan_sums, dim3(1), dim3(c.block), 0, st, sums, (int)c.grid_scan);
}
void mgxe_csr_rowptr(hipStream_t st, const unsigned long long *mask, long long n, const long long *sums, int *rowptr) {
  const ExChoice c = choose_export(n);
  hipLaunchKernelGGL(k_csr_rowptr, dim3(c.grid_scan), dim3(c.block), 0, st, mask, n, sums, rowptr);
}
void mgxe_csr_scatter(hipStream_t st, const LevView *L, const double *a, const ExMap *m, int colour, const unsigned long long *mask, const int *rowptr,
                      int *col, double *val, double sign) {
  const ExChoice c = choose_export((long long)L->nx * L->ny * L->nz);
  hipLaunchKernelGGL(k_csr_scatter, dim3(c.grid_rows), dim3(c.block), 0, st, *L, a, *m, colour, mask, rowptr, col, val, sign);
}

}  // extern "C"
