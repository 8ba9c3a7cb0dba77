// The geometry of the CSR export walked on the host: a stand-alone program (no GPU, no HIP runtime, any C++17 compiler) over the pure
// functions of mgroms_amd/csrc/mgx_export.h, in the pattern of tests/kernel_choice/.  tests/test_export_host.py builds and runs it.
//
//   export_main colouring [q] for closed, singly and doubly periodic levels of every listed size per axis and for A, R and P:
//                             (1) no two cells that one row can see share a colour, (2) the column recovered for (row, colour of a visible
//                             cell) is that cell, (3) a colour no visible cell has gives no column.  What a row can see is spelled out HERE
//                             (the stencil's reach and the halo rule), not taken from the header.  One line per configuration, "FAIL ..." lines
//                             for the first offences, exit status 1 if there were any.
//   export_main axis          the colours along one axis: "axis <rule> <n> : c1 c2 ... cn" for n = 1 .. 40 and the three rules
//   export_main choice        "choice <n> <block> <grid_rows> <grid_scan>" for row counts either side of every block boundary, and
//                             "fits <nrows> <ncols> <nnz> <answer>" either side of the int limit
#include "mgx_export.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define FAIL(...) do { if (g_fail++ < 20) { printf("FAIL "); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the interior cell a position 0 .. n + 1 of an axis stands for under a halo rule; 0 = none (this file's own spelling)
static int fold(int x, int n, int rule) {
  if (x >= 1 && x <= n) return x;
  if (x != 0 && x != n + 1) return 0;
  if (rule == EX_MIRROR) return x == 0 ? 1 : n;
  if (rule == EX_WRAP) return x == 0 ? n : 1;
  return 0;
}

struct Cell { int k, j, i; };
// at most 27 distinct cells
struct Cells {
  Cell c[27]; int n = 0;
  void insert(const Cell &x) { for (int q = 0; q < n; q++) if (c[q].k == x.k && c[q].j == x.j && c[q].i == x.i) return; c[n++] = x; }
  const Cell *begin() const { return c; }
  const Cell *end() const { return c + n; }
};

// the column-level cells row (k, j, i) can see
static Cells visible(const ExMap &m, int rule_j, int rule_i, int k, int j, int i) {
  Cells s;
  if (m.mode == EX_R) {   // the row's children
    for (int dk = 0; dk < (m.held ? 1 : 2); dk++) for (int dj = 0; dj < 2; dj++) for (int di = 0; di < 2; di++) {
      const Cell c = {m.held ? k : 2 * k - 1 + dk, 2 * j - 1 + dj, 2 * i - 1 + di};
      if (c.k <= m.cnz && c.j <= m.cny && c.i <= m.cnx) s.insert(c);
    }
    return s;
  }
  // A: within one step of the cell; P: within one step of the parent (the 2 x 2 x 2 of the interpolation lie inside)
  const bool par = m.mode == EX_P;
  const int zk = par && !m.held ? (k + 1) / 2 : k, zj = par ? (j + 1) / 2 : j, zi = par ? (i + 1) / 2 : i;
  for (int dk = -1; dk <= 1; dk++) for (int dj = -1; dj <= 1; dj++) for (int di = -1; di <= 1; di++) {
    const Cell c = {fold(zk + dk, m.cnz, EX_OPEN), fold(zj + dj, m.cny, rule_j), fold(zi + di, m.cnx, rule_i)};
    if (c.k && c.j && c.i) s.insert(c);
  }
  return s;
}

// odd: the fine level of P has an odd nz = 2 cnz + 1, whose top row the halving pair drops (nz 5 -> 2)
static void check(int mode, int held, int cnx, int cny, int cnz, int rule_j, int rule_i, int odd = 0) {
  int rnx = cnx, rny = cny, rnz = cnz;
  if (mode == EX_R) { if (cnx & 1 || cny & 1) return; rnx = cnx / 2; rny = cny / 2; rnz = held ? cnz : cnz / 2; if (rnz < 1) return; }
  if (mode == EX_P) { rnx = 2 * cnx; rny = 2 * cny; rnz = held ? cnz : 2 * cnz + odd; }
  const ExMap m = ex_map(mode, rnx, rny, rnz, cnx, cny, cnz, rule_j, rule_i);
  if (m.held != held) return;   // (nz_c == nz_f reads as a held pair: no halving pair has it)
  const int nc = ex_ncolours(m);
  const int before = g_fail;
  long long rows = 0, seen = 0;
  if (nc > EX_MAX_COLOURS) FAIL("mode %d %dx%dx%d rules %d %d: %d colours", mode, cnx, cny, cnz, rule_j, rule_i, nc);
  for (int i = 1; i <= rnx; i++) for (int j = 1; j <= rny; j++) for (int k = 1; k <= rnz; k++) {
    const Cells vis = visible(m, rule_j, rule_i, k, j, i);
    std::vector<int> owner(nc, 0);
    rows++;
    for (const Cell &c : vis) {
      const int col = ex_cell_colour(m, c.k, c.j, c.i);
      seen++;
      if (col < 0 || col >= nc) { FAIL("mode %d %dx%dx%d rules %d %d: cell %d %d %d has colour %d of %d", mode, cnx, cny, cnz, rule_j, rule_i, c.k, c.j, c.i, col, nc); continue; }
      if (owner[col]++) FAIL("mode %d %dx%dx%d rules %d %d: row %d %d %d sees colour %d twice", mode, cnx, cny, cnz, rule_j, rule_i, k, j, i, col);
      const long long want = ((long long)(c.i - 1) * cny + (c.j - 1)) * cnz + (c.k - 1), got = ex_column(m, k, j, i, col);
      if (got != want) FAIL("mode %d %dx%dx%d rules %d %d: row %d %d %d colour %d -> column %lld, coloured cell %d %d %d = %lld", mode, cnx, cny, cnz, rule_j, rule_i, k, j, i, col, got, c.k, c.j, c.i, want);
    }
    for (int col = 0; col < nc; col++)
      if (!owner[col] && ex_column(m, k, j, i, col) >= 0) FAIL("mode %d %dx%dx%d rules %d %d: row %d %d %d has a column for colour %d, which it cannot see", mode, cnx, cny, cnz, rule_j, rule_i, k, j, i, col);
  }
  printf("%s mode=%d held=%d columns=%dx%dx%d rule_j=%d rule_i=%d colours=%d rows=%lld visible=%lld\n", g_fail == before ? "ok" : "BAD", mode, held, cnx, cny, cnz, rule_j, rule_i, nc, rows, seen);
}

int main(int argc, char **argv) {
  const char *what = argc > 1 ? argv[1] : "";
  if (!strcmp(what, "colouring")) {
    static const int NXY[] = {2, 4, 6, 8, 10, 12, 20}, NZ[] = {2, 3, 4, 5, 8};
    static const int RULES[][2] = {{EX_MIRROR, EX_MIRROR}, {EX_WRAP, EX_MIRROR}, {EX_MIRROR, EX_WRAP}, {EX_WRAP, EX_WRAP}};
    const int only = argc > 2 ? atoi(argv[2]) : -1;   // one pair of rules (0 .. 3), so that the caller may run the four side by side
    for (int q = 0; q < 4; q++) {
      if (only >= 0 && q != only) continue;
      const int *r = RULES[q];
      for (const int nx : NXY) for (const int ny : NXY) for (const int nz : NZ)
        for (int mode = EX_A; mode <= EX_P; mode++)
          for (int held = 0; held <= (mode == EX_A ? 0 : 1); held++) check(mode, held, nx, ny, nz, r[0], r[1]);
      for (const int nz : NZ) check(EX_P, 0, 8, 6, nz, r[0], r[1], 1);
    }
    return g_fail ? 1 : 0;
  }
  if (!strcmp(what, "axis")) {
    for (int rule = EX_OPEN; rule <= EX_WRAP; rule++)
      for (int n = 1; n <= 40; n++) {
        const ExAxis a = ex_axis(n, rule);
        printf("axis %d %d %d :", rule, n, a.ncol);
        for (int x = 1; x <= n; x++) printf(" %d", ex_colour(a, x));
        printf("\n");
      }
    return 0;
  }
  if (!strcmp(what, "choice")) {
    static const long long N[] = {1, 2, 255, 256, 257, 2046, 2047, 2048, 2049, 4095, 4096, 2048LL * 256 - 1, 2048LL * 256, 16LL * 16 * 8, 512LL * 512 * 64, 2147483646LL};
    for (const long long n : N) { const ExChoice c = choose_export(n); printf("choice %lld %u %u %u\n", n, c.block, c.grid_rows, c.grid_scan); }
    static const long long F[][3] = {{1, 1, 0}, {2147483646LL, 8, 19}, {2147483647LL, 8, 19}, {8, 2147483647LL, 19}, {1 << 20, 1 << 20, 2147483647LL}, {1 << 20, 1 << 20, 2147483648LL}, {1 << 27, 1 << 27, 19LL << 27}};
    for (const auto &f : F) printf("fits %lld %lld %lld %d\n", f[0], f[1], f[2], ex_fits_int(f[0], f[1], f[2]));
    return 0;
  }
  fprintf(stderr, "usage: %s colouring|axis|choice\n", argv[0]);
  return 2;
}
