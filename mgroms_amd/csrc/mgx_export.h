// The geometry of the CSR export (mgx_export.hip; include/mgx.h: mgx_operator_csr, mgx_transfer_csr): which unit vectors share a probe, which
// column a probed value belongs to, and the launches.  Pure functions of integers -- no HIP call, no state, no environment -- compiled for
// the host and for the device from this one text, and free of every other header so that tests/export_host/export_main.cpp can walk them
// with any C++ compiler (tests/test_export_host.py).
//
// The export never restates the operator: it applies the library's own residual / fine2coarse / coarse2fine to sums of unit vectors and
// reads the entries off the result.  A sum may hold two unit vectors only if no row sees both, so the unknowns are coloured:
//   A, P  per axis a colouring in which any three consecutive cells differ, the product of the three axes as the colour of a cell.  A row of
//         A sees the cells within one step of its own cell, a row of P the coarse cells within one step of its parent (a superset of the
//         2 x 2 x 2 it interpolates from), each after the level's halo rule has folded a halo cell onto its interior source.
//   R     a row sees its own 2 x 2 x 2 children (2 x 2 x 1 on a held pair) and the children of two rows are disjoint: the colour of a
//         fine cell is its place among its siblings, 8 (4) colours whatever the halo rule.
// Cells are 1-based per axis as everywhere in the library; an unknown's index is ((i-1)*ny + (j-1))*nz + (k-1), the reference's k-fastest order.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGX_EX_HD __host__ __device__
#else
#define MGX_EX_HD
#endif

// what lies past the ends of an axis
enum {
  EX_OPEN = 0,    // nothing: the k axis (the kernels have no rows 0 and nz + 1)
  EX_MIRROR = 1,  // a closed side: halo cell 0 is the image of cell 1, n + 1 of n
  EX_WRAP = 2,    // option "periodic": halo cell 0 is cell n, n + 1 is cell 1
};
enum { EX_A = 0, EX_R = 1, EX_P = 2 };
constexpr int EX_MAX_COLOURS = 64;   // one bit per colour in a row's mask

// One axis of n cells.  Any three consecutive cells get different colours, cyclically on a wrapped axis: there the run 0 1 2 repeats where
// 3 divides n; otherwise n = 4 b + 3 a with b = n mod 3 leading runs of 0 1 2 3 (possible from n = 6 on: 7 = 4 + 3, 8 = 4 + 4, 10 = 4 + 3 + 3);
// below 6 every cell has a colour of its own.
struct ExAxis { int n, rule, ncol, lead4; };
MGX_EX_HD inline ExAxis ex_axis(int n, int rule) {
  ExAxis a;
  a.n = n; a.rule = rule; a.lead4 = 0;
  if (rule != EX_WRAP) { a.ncol = n < 3 ? n : 3; return a; }
  if (n < 6) { a.ncol = n; return a; }
  a.lead4 = 4 * (n % 3);
  a.ncol = a.lead4 ? 4 : 3;
  return a;
}
MGX_EX_HD inline int ex_colour(const ExAxis &a, int x) {   // x = 1 .. n
  const int x0 = x - 1;
  if (a.rule == EX_WRAP && a.n < 6) return x0;
  return x0 < a.lead4 ? x0 % 4 : (x0 - a.lead4) % 3;
}
// the interior cell that position x = 0 .. n + 1 stands for, 0 = none
MGX_EX_HD inline int ex_fold(const ExAxis &a, int x) {
  if (x >= 1 && x <= a.n) return x;
  if (a.rule == EX_OPEN || x < 0 || x > a.n + 1) return 0;
  if (a.rule == EX_MIRROR) return x == 0 ? 1 : a.n;
  return x == 0 ? a.n : 1;
}
// the cell of colour c among the cells within one step of `centre` (0 .. n + 1), 0 = none of them has it
MGX_EX_HD inline int ex_find(const ExAxis &a, int centre, int c) {
  for (int d = -1; d <= 1; d++) {
    const int x = ex_fold(a, centre + d);
    if (x && ex_colour(a, x) == c) return x;
  }
  return 0;
}

// One export.  Rows are the cells of rn* (A: the level; R: the coarse level; P: the fine level), columns the cells of cn* (A: the level;
// R: the fine level; P: the coarse level); ak, aj, ai: the axes of the COLUMN level (A, P; R does not colour by axis).
struct ExMap {
  int mode, held;
  int rnx, rny, rnz, cnx, cny, cnz;
  ExAxis ak, aj, ai;
};
// rule_j, rule_i: EX_MIRROR or EX_WRAP of the COLUMN level's j and i sides
MGX_EX_HD inline ExMap ex_map(int mode, int rnx, int rny, int rnz, int cnx, int cny, int cnz, int rule_j, int rule_i) {
  ExMap m;
  m.mode = mode; m.held = mode != EX_A && rnz == cnz;
  m.rnx = rnx; m.rny = rny; m.rnz = rnz; m.cnx = cnx; m.cny = cny; m.cnz = cnz;
  m.ak = ex_axis(cnz, EX_OPEN); m.aj = ex_axis(cny, rule_j); m.ai = ex_axis(cnx, rule_i);
  return m;
}
MGX_EX_HD inline int ex_ncolours(const ExMap &m) { return m.mode == EX_R ? (m.held ? 4 : 8) : m.ak.ncol * m.aj.ncol * m.ai.ncol; }
// the colour of column-level cell (k, j, i): the probe of that colour holds a one there
MGX_EX_HD inline int ex_cell_colour(const ExMap &m, int k, int j, int i) {
  if (m.mode == EX_R) return m.held ? ((j - 1) & 1) + 2 * ((i - 1) & 1) : ((k - 1) & 1) + 2 * ((j - 1) & 1) + 4 * ((i - 1) & 1);
  return ex_colour(m.ak, k) + m.ak.ncol * (ex_colour(m.aj, j) + m.aj.ncol * ex_colour(m.ai, i));
}
MGX_EX_HD inline long long ex_index(int nz, int ny, int k, int j, int i) { return ((long long)(i - 1) * ny + (j - 1)) * nz + (k - 1); }
// the column that colour c stands for in row (k, j, i): the one cell of that colour the row can see; -1 = it sees none
MGX_EX_HD inline long long ex_column(const ExMap &m, int k, int j, int i, int c) {
  int ck, cj, ci;
  if (m.mode == EX_R) {
    if (m.held) { ck = k; cj = 2 * j - 1 + (c & 1); ci = 2 * i - 1 + ((c >> 1) & 1); }
    else { ck = 2 * k - 1 + (c & 1); cj = 2 * j - 1 + ((c >> 1) & 1); ci = 2 * i - 1 + ((c >> 2) & 1); }
    if (ck > m.cnz || cj > m.cny || ci > m.cnx) return -1;
  } else {
    const bool parent = m.mode == EX_P;   // the centre of a row of P is its parent cell on the coarse level
    const int zk = parent && !m.held ? (k + 1) / 2 : k, zj = parent ? (j + 1) / 2 : j, zi = parent ? (i + 1) / 2 : i;
    ck = ex_find(m.ak, zk, c % m.ak.ncol);
    cj = ex_find(m.aj, zj, (c / m.ak.ncol) % m.aj.ncol);
    ci = ex_find(m.ai, zi, c / (m.ak.ncol * m.aj.ncol));
    if (!ck || !cj || !ci) return -1;
  }
  return ex_index(m.cnz, m.cny, ck, cj, ci);
}

// ---- the launches: one lane per row (or per cell of the probe), 256 lanes per workgroup; the row counts are summed EX_SCAN_ROWS rows per
// workgroup, the workgroups' sums scanned by one workgroup, the rows' offsets written by a second pass over the same blocks ----
constexpr int EX_BLOCK = 256;
constexpr int EX_SCAN_ITEMS = 8;                          // rows per lane of the two scan passes
constexpr int EX_SCAN_ROWS = EX_BLOCK * EX_SCAN_ITEMS;    // rows per workgroup there
struct ExChoice { unsigned block, grid_rows, grid_scan; };
// n: rows (or probe cells); the scan covers n + 1 entries, the last being rowptr[n] = nnz
inline ExChoice choose_export(long long n) {
  ExChoice c;
  c.block = EX_BLOCK;
  c.grid_rows = (unsigned)((n + EX_BLOCK - 1) / EX_BLOCK);
  c.grid_scan = (unsigned)((n + 1 + EX_SCAN_ROWS - 1) / EX_SCAN_ROWS);
  return c;
}
// rowptr and col are ints: what must fit one.  0 = fits, 1 = the rows do not, 2 = the entries do not
inline int ex_fits_int(long long nrows, long long ncols, long long nnz) {
  const long long lim = 2147483647LL;
  if (nrows < 0 || nrows >= lim || ncols < 0 || ncols >= lim) return 1;   // (rowptr has nrows + 1 entries)
  return nnz < 0 || nnz > lim ? 2 : 0;
}
