// Which kernel serves which level: a stand-alone host program (no GPU, no HIP runtime) that calls the extern "C" wrappers of
// mgx_wrappers.h -- the smoother's, the sequential-order red-black walk's, the fused residual + restriction's -- over a table of shapes,
// flags and A/B switches and prints, per call, one line per kernel launch (the demangled template instance, grid, block, dynamic LDS
// bytes, scalar arguments) and the wrapper's return value.
//
// Built from mgx_relax.hip, mgx_relax_coarse.hip, mgx_relax_ks.hip, mgx_relax_tall.hip, mgx_rbseq.hip and mgx_resrest.hip compiled
// host-only behind record_shim.h, which sends their launches here; the stand-ins at the end of this file replace what the units and the
// compiler's registration code ask of the HIP runtime.
// tests/test_kernel_choice_host.py builds and runs it and compares digests with tests/golden/kernel_choice.json.
//
//   record_main [refuse|fail|names]     refuse: every hipFuncSetAttribute is refused; fail: hipGetLastError reports an error after every launch
#include <hip/hip_runtime.h>
#include "mgx_internal.h"
#include "mgx_switches.h"
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// ---- what the units link against besides the wrappers ----
static Switches g_sw;
const Switches &mgx_switches() { return g_sw; }
thread_local hipError_t mgx_pending_error = hipSuccess;

static bool g_refuse = false, g_fail = false;
static hipError_t g_err = hipSuccess;
static std::string g_line;

static std::string demangled(const char *sym0) {
  std::string sym = sym0;
  const size_t pad = sym.find("__sanitized_padded_global");   // AddressSanitizer's name for a kernel handle it padded
  if (pad != std::string::npos) sym.erase(pad);
  int st = 0;
  char *d = abi::__cxa_demangle(sym.c_str(), nullptr, nullptr, &st);
  std::string s = (st == 0 && d) ? d : sym;
  free(d);
  const std::string stub = "__device_stub__";
  const size_t at = s.find(stub);
  if (at != std::string::npos) s.erase(at, stub.size());
  return s;
}
static std::string kernel_name(const void *k) {
  Dl_info di;
  return dladdr(k, &di) && di.dli_sname ? demangled(di.dli_sname) : "?";
}

void rec_launch(const void *kernel, dim3 g, dim3 b, size_t lds) {
  char buf[160];
  snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u,%u,%u lds=%zu args=", g.x, g.y, g.z, b.x, b.y, b.z, lds);
  g_line = "  launch " + kernel_name(kernel) + buf;
  if (g_fail) g_err = hipErrorLaunchFailure;
}
void rec_arg(long long v) { g_line += std::to_string(v) + " "; }
void rec_arg(const void *p) { g_line += p ? "ptr " : "null "; }
void rec_arg(const Sides &s) { char b[32]; snprintf(b, sizeof b, "S%d%d%d%d/%d ", s.S, s.E, s.N, s.W, s.part); g_line += b; }
void rec_arg(const LevView &L) { char b[96]; snprintf(b, sizeof b, "L(%d,%d,%d,zy=%d,d0w=%d) ", L.nx, L.ny, L.nz, L.zy != nullptr, L.d0w != nullptr); g_line += b; }
void rec_arg(const LevView32 &L) { char b[64]; snprintf(b, sizeof b, "L32(%d,%d,%d) ", L.nx, L.ny, L.nz); g_line += b; }
void rec_fuse(const Sides &ph, const int (&v)[6], long long min_cells, const void *flag, unsigned int seq, const void *err) {
  char b[160];
  rec_arg(ph);
  snprintf(b, sizeof b, "F(KR=%d,nt=%d,nchunk=%d,nkz=%d,nworkers=%d,stall=%d,min=%lld,flag=%d,seq=%u,err=%d) ", v[0], v[1], v[2], v[3], v[4], v[5], min_cells, flag != nullptr, seq, err != nullptr);
  g_line += b;
}
void rec_end() { puts(g_line.c_str()); }
hipError_t rec_last_error() { const hipError_t e = g_err; g_err = hipSuccess; return e; }
hipError_t rec_set_attribute(const void *kernel, hipFuncAttribute attr, int value) {
  printf("  attr %s %d=%d%s\n", kernel_name(kernel).c_str(), (int)attr, value, g_refuse ? " refused" : "");
  if (g_refuse) { g_err = hipErrorInvalidValue; return hipErrorInvalidValue; }
  return hipSuccess;
}

// ---- the table ----
static double g_fake[8];   // never dereferenced: the wrappers only test pointers and pass them on
static LevView level(int nx, int ny, int nz, bool zy, bool d0w) {
  LevView v;
  memset(&v, 0, sizeof v);
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.EO = 15; v.HO = (16 + ny / 2 + 15) / 16 * 16; v.RS = (v.HO + ny / 2 + 1 + 15) / 16 * 16;
  v.plane = (long long)nz * v.RS;
  double *f = g_fake;
  v.p = v.b = v.r = v.bet = v.gam = v.p1 = f;
  for (double *&a : v.cA) a = f;
  if (zy) { v.zy = v.zx = f; }
  if (d0w) v.d0w = f;
  return v;
}
static Sides sides(int which) {   // 0 closed, 1..4 one side open, 5 / 6 part 1 / 2 of a level open to the west and north
  Sides s = {1, 1, 1, 1, 0};
  if (which == 1) s.S = 0;
  if (which == 2) s.E = 0;
  if (which == 3) s.N = 0;
  if (which == 4) s.W = 0;
  if (which >= 5) { s.W = 0; s.N = 0; s.part = which - 4; }
  return s;
}

static void switches_default() {
  memset(&g_sw, 0, sizeof g_sw);
  g_sw.ks8 = g_sw.ks64 = g_sw.ksp_fence = g_sw.rbseq_d0_mid = true;
  g_sw.rbw_prio = 1; g_sw.c2f_nt = -1; g_sw.resrest_flat_max = 256LL * 256 * 64; g_sw.resrest_ahead = 11; g_sw.p2p_maxblk = 128; g_sw.p2p_ipt = 1;
}
// each smoother-related switch on by itself
static const char *const SWITCHES[] = {"default", "no_xcd", "no_reg", "no_tiny", "no_wave", "no_wave_fuse", "no_tall", "no_ks", "no_ks8", "no_ks64", "no_ks2", "no_ksp", "ksp_sc1", "ks_nw4"};
constexpr int NSW = sizeof SWITCHES / sizeof *SWITCHES;
static const char *set_switch(int s) {
  switches_default();
  switch (s) {
    case 1: g_sw.no_xcd = true; break;
    case 2: g_sw.no_reg = true; break;
    case 3: g_sw.no_tiny = true; break;
    case 4: g_sw.no_wave = true; break;
    case 5: g_sw.no_wave_fuse = true; break;
    case 6: g_sw.no_tall = true; break;
    case 7: g_sw.no_ks = true; break;
    case 8: g_sw.ks8 = false; break;
    case 9: g_sw.ks64 = false; break;
    case 10: g_sw.no_ks2 = true; break;
    case 11: g_sw.no_ksp = true; break;
    case 12: g_sw.ksp_fence = false; break;
    case 13: g_sw.ks_nw = 4; break;
    default: break;
  }
  return SWITCHES[s];
}

static const int NZS[] = {2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128};
struct Shape { int nx, ny; };
// one-workgroup kernels: columns either side of 64, 256, 1024, 2048; 2 x 2 blocks either side of 64, 256, 512; columns of a colour either
// side of 64, 256, 1024 (two and four colours); odd nx, odd ny; the 64 KB of k_relax_tiny (16x16 / 16x18 at nz = 2, 10x12 / 12x12 at
// nz = 4); half-rows either side of a wave (2x128 / 2x130) and the largest levels of the walk's LDS (64x32x2, 32x32x4: below 160 KB)
static const Shape SMALL[] = {{8, 8}, {8, 10}, {8, 16}, {8, 18}, {10, 12}, {12, 12}, {15, 16}, {16, 15}, {16, 16}, {16, 18}, {16, 32}, {16, 34},
                              {32, 32}, {32, 34}, {34, 32}, {32, 64}, {32, 66}, {64, 32}, {64, 34}, {64, 64}, {64, 66}, {2, 128}, {2, 130}, {4, 256}, {128, 128}};
// colour passes: gx0 * nplanes either side of 512 and 2048, ny / 2 either side of 64, nx either side of 128, odd sizes
static const Shape PASS[] = {{16, 16}, {15, 17}, {32, 32}, {64, 64}, {128, 128}, {126, 130}, {130, 126}, {256, 256}, {258, 256}, {254, 258}, {512, 256}, {516, 256}, {512, 512}, {1022, 256}, {1024, 256},
                             {1026, 256}, {512, 1024}, {510, 1026}, {1024, 1024}, {2048, 256}, {2046, 256}, {4096, 256}, {4094, 256}, {4098, 256}};

static void call_head(const char *w, int nz, int method, const char *fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  if (method >= 0) printf("call %s nz=%d method=%d | %s\n", w, nz, method, b);
  else printf("call %s nz=%d method=- | %s\n", w, nz, b);
  g_err = hipSuccess;
}
static void call_ret(int r) { printf("  -> %d\n", r); }

// depth 2: every combination, and around (closed, slopes, one sweep) one factor at a time: the sides, no slopes, d0w, nsweeps 0 and 40;
// depth 1: every combination; depth 0 (a switch on): cmatrix = 'real' only, folded transfers all or none.  nz > 8: three shapes (no kernel).
static void small_calls(int nz, const char *sw, int depth) {
  const int nshape = nz > 8 ? 3 : (int)(sizeof SMALL / sizeof *SMALL);
  for (int is = 0; is < nshape; is++)
    for (int method = 0; method <= 2; method++)
      for (int real = depth ? 0 : 1; real <= 1; real++)
        for (int mode = 0; mode <= 2; mode++)
          for (int any = 0; any <= 1; any++) {
            const Shape &s = SMALL[is];
            const int nvar = depth == 2 && (mode == 0 || (method == 1 && real)) ? 11 : 1;
            for (int var = 0; var < nvar; var++) {
              const int sd = var >= 1 && var <= 6 ? var : 0, ns = var == 9 ? 0 : (var == 10 ? 40 : 1);
              const LevView L = level(s.nx, s.ny, nz, var != 7, var == 8);
              call_head("mgxk_relax_small", nz, method, "%dx%d real=%d mode=%d any=%d sides=%d zy=%d d0w=%d nsweeps=%d sw=%s", s.nx, s.ny, real, mode, any, sd, var != 7, var == 8, ns, sw);
              call_ret(mgxk_relax_small(nullptr, &L, ns, method, real, sides(sd), mode, any));
              call_head("mgxk_relax_wave", nz, method, "%dx%d real=%d mode=%d any=%d sides=%d zy=%d d0w=%d nsweeps=%d sw=%s", s.nx, s.ny, real, mode, any, sd, var != 7, var == 8, ns, sw);
              call_ret(mgxk_relax_wave(nullptr, &L, ns, method, real, sides(sd), mode, any));
              if (any) continue;
              for (int flags = 0; flags <= 3; flags += (depth && var == 0 ? 1 : 3))
                for (int cv = 0; cv < (depth && var == 0 && flags == 3 ? 4 : 1); cv++) {   // the coarse level: half the size, none, not half in nx, not half in nz
                  const LevView C = level(cv == 2 ? s.nx : s.nx / 2, s.ny / 2, cv == 3 ? nz : nz / 2, true, false);
                  const int nsf = var == 9 ? -1 : ns;   // the fused entry refuses a negative count
                  call_head("mgxk_relax_wave_fused", nz, method, "%dx%d real=%d mode=%d flags=%d coarse=%d sides=%d zy=%d d0w=%d nsweeps=%d sw=%s", s.nx, s.ny, real, mode, flags, cv, sd, var != 7, var == 8, nsf, sw);
                  call_ret(mgxk_relax_wave_fused(nullptr, &L, cv == 1 ? nullptr : &C, nsf, method, real, sides(sd), flags, mode));
                }
            }
          }
  for (int is = 0; is < nshape; is++)
    for (int any = 0; any <= 1; any++) {
      const Shape &s = SMALL[is];
      const LevView L = level(s.nx, s.ny, nz, true, false);
      call_head("mgxk_coarse_direct_cells", nz, -1, "%dx%d any=%d sw=%s", s.nx, s.ny, any, sw);
      call_ret(mgxk_coarse_direct_cells(&L, any));
      for (int method = 1; method <= 2; method++)
        for (int mode = 0; mode <= 2; mode += 2) {
          call_head("mgxk_coarse_direct_build", nz, method, "%dx%d real=1 mode=%d any=%d nsweeps=40 sw=%s", s.nx, s.ny, mode, any, sw);
          call_ret(mgxk_coarse_direct_build(nullptr, &L, 40, method, 1, sides(0), mode, g_fake, 1000, g_fake, any));
        }
      call_head("mgxk_coarse_direct_apply", nz, -1, "%dx%d any=%d sw=%s", s.nx, s.ny, any, sw);
      call_ret(mgxk_coarse_direct_apply(nullptr, &L, g_fake, g_fake, (unsigned int *)g_fake, sides(0), any));
    }
}

// depth 2: (real, snap) as the cycle asks for them x d0w x three kinds of pass, the sides on the first shapes, and the hyperplane sweep;
// depth 1: without the sides and the sweep; depth 0 (a switch on): no d0w, no plane loop, levels without slopes on the first shapes
static void pass_calls(int nz, const char *sw, int depth) {
  int is = -1;
  for (const Shape &s : PASS) {
    is++;
    for (int zy = depth || is < 4 ? 0 : 1; zy <= 1; zy++) {
      const LevView Lh = level(s.nx, s.ny, nz, zy, false);
      call_head("mgxk_has_reg_kernel", nz, -1, "%dx%d zy=%d sw=%s", s.nx, s.ny, zy, sw);
      call_ret(mgxk_has_reg_kernel(&Lh));
      for (int rs = 0; rs < 3; rs++) {   // (real, snap): the three the cycle asks for
        const int real = rs > 0, snap = rs > 1;
        for (int d0w = 0; d0w <= (snap && depth ? 1 : 0); d0w++)
          for (int geo = 0; geo < 3; geo += depth ? 1 : 2) {   // a red-black pass over all planes, one plane of the plane loop, a four-colour pass
            const int i0 = geo == 2 ? 2 : 1, istep = geo == 2 ? 2 : 1, nplanes = geo == 0 ? s.nx : (geo == 1 ? 1 : s.nx / 2);
            const int jodd = geo == 2 ? 1 : -1, rb = geo == 2 ? 0 : 1;
            for (int sd = 0; sd < (depth == 2 && geo != 1 && is < 6 ? 7 : 1); sd++) {
              const LevView L = level(s.nx, s.ny, nz, zy, d0w);
              const char *const fmt = "%dx%d real=%d snap=%d i0=%d istep=%d nplanes=%d jodd=%d rb=%d sides=%d zy=%d d0w=%d sw=%s";
              call_head("mgxk_relax_colour", nz, -1, fmt, s.nx, s.ny, real, snap, i0, istep, nplanes, jodd, rb, sd, zy, d0w, sw);
              call_ret(mgxk_relax_colour(nullptr, &L, i0, istep, nplanes, jodd, rb, real, snap, sides(sd)));
              call_head("mgxk_relax_ks", nz, -1, fmt, s.nx, s.ny, real, snap, i0, istep, nplanes, jodd, rb, sd, zy, d0w, sw);
              call_ret(mgxk_relax_ks(nullptr, &L, i0, istep, nplanes, jodd, rb, real, snap, sides(sd)));
              call_head("mgxk_relax_tall", nz, -1, fmt, s.nx, s.ny, real, snap, i0, istep, nplanes, jodd, rb, sd, zy, d0w, sw);
              call_ret(mgxk_relax_tall(nullptr, &L, i0, istep, nplanes, jodd, rb, real, snap, sides(sd)));
            }
          }
      }
      for (int real = depth ? 0 : 1; real <= 1; real++)
        for (int sd = 0; sd < (depth == 2 ? 5 : 1); sd++)
          for (int fc1 = 1; fc1 <= 2; fc1++) {
            call_head("mgxk_relax_ks_pair", nz, -1, "%dx%d real=%d i0=%d nplanes=%d sides=%d zy=%d sw=%s", s.nx, s.ny, real, fc1, s.nx / 2, sd, zy, sw);
            call_ret(mgxk_relax_ks_pair(nullptr, &Lh, fc1, s.nx / 2, real, sides(sd)));
          }
    }
  }
  // the hyperplane sweep: ny + 2 nx - 2 launches, small shapes only (the last one has fronts of more than one wave)
  static const Shape GS[] = {{4, 4}, {3, 5}, {70, 132}};
  if (depth == 2)
    for (const Shape &s : GS)
      for (int real = 0; real <= 1; real++) {
        const LevView L = level(s.nx, s.ny, nz, true, false);
        call_head("mgxk_relax_gs_sweep", nz, -1, "%dx%d real=%d sw=%s", s.nx, s.ny, real, sw);
        call_ret(mgxk_relax_gs_sweep(nullptr, &L, real));
      }
}

// ---- mgx_rbseq.hip: the sequential-order red-black walk ----
static int g_dev = -1;              // what the stand-in hipGetDevice answers; < 0: no device
static bool g_probe_equal = true;   // what the stand-in copy leaves in the placement probe's answer (rbseq_placement_ok asks once per device)
static const char *const RB_SWITCHES[] = {"default", "rbseq_d0_kernel", "rbseq_no_d0_mid", "no_rbseq_walk_apply", "rbseq_window_no_xmap", "rbw_prio0"};
constexpr int NRBSW = sizeof RB_SWITCHES / sizeof *RB_SWITCHES;
static const char *set_rb_switch(int s) {
  switches_default();
  switch (s) {
    case 1: g_sw.rbseq_d0_kernel = true; break;
    case 2: g_sw.rbseq_d0_mid = false; break;
    case 3: g_sw.no_rbseq_walk_apply = true; break;
    case 4: g_sw.rbseq_window_no_xmap = true; break;
    case 5: g_sw.rbw_prio = 0; break;
    default: break;
  }
  return RB_SWITCHES[s];
}
static LevView level_rb(int nx, int ny, int nz, bool gk) {
  LevView v = level(nx, ny, nz, true, false);
  if (gk) v.gk = v.ag58 = v.u1 = g_fake;
  return v;
}
// what the colour pass is told about d0 (the test: a walk that reads d0 from u1 has asked for it)
static void wants_d0_line(const LevView &L) { printf("  wants_d0 %d\n", mgxk_rbseq_wants_d0(&L)); }

// half-rows of 64, 128, 256, 512, 1024 columns, one more, and partial ones in between
static const int RB_NY[] = {2, 100, 128, 130, 200, 256, 258, 400, 512, 514, 1000, 1024, 1026, 2000, 2048, 2050};
// odd; divisible by 16, by 8, 4, 2 only; either side of 128; operands either side of 2 MB (254 / 256 x 512) and of the 32 helpers; either side of 1 << 13
static const int RB_NX[] = {15, 16, 24, 12, 10, 64, 128, 130, 254, 256, 512, 2048, 8190, 8192};

// both colours, the snapshot written or not; depth 2: once per shape no error word and no gk
static void scan_calls(int nz, const char *sw, int depth) {
  for (const int ny : RB_NY)
    for (const int nx : RB_NX) {
      const LevView L = level_rb(nx, ny, nz, true), L0 = level_rb(nx, ny, nz, false);
      const long long cells = (long long)nx * (ny / 2) * nz;
      int err = 0;
      for (int rb = 0; rb <= 1; rb++)
        for (int have_d0 = 0; have_d0 <= 1; have_d0++) {
          if (nz == 5 || nz == 12 || nz == 64) {   // (the plain walk does not look at nz)
            call_head("mgxk_rbseq_scan", nz, -1, "%dx%d rb=%d have_d0=%d gk=1 sw=%s", nx, ny, rb, have_d0, sw);
            const int r = mgxk_rbseq_scan(nullptr, &L, rb, have_d0);
            wants_d0_line(L);
            call_ret(r);
          }
          for (int snapw = 0; snapw <= 1; snapw++)
            for (int below = 0; below <= 1; below++) {   // min_cells = the level's cells of a colour (fused from there on), and one more
              call_head("mgxk_rbseq_scan_apply", nz, -1, "%dx%d rb=%d have_d0=%d snapw=%d min_cells=cells+%d err=1 gk=1 sw=%s", nx, ny, rb, have_d0, snapw, below, sw);
              const int r = mgxk_rbseq_scan_apply(nullptr, &L, rb, sides(0), snapw, have_d0, (unsigned int *)g_fake, 3, &err, 0, cells + below);
              wants_d0_line(L);
              call_ret(r);
            }
        }
      if (depth != 2) continue;
      call_head("mgxk_rbseq_scan_apply", nz, -1, "%dx%d rb=1 have_d0=1 snapw=1 min_cells=0 err=0 gk=1 sw=%s", nx, ny, sw);
      int r = mgxk_rbseq_scan_apply(nullptr, &L, 1, sides(0), 1, 1, (unsigned int *)g_fake, 3, nullptr, 0, 0);
      wants_d0_line(L);
      call_ret(r);
      call_head("mgxk_rbseq_scan_apply", nz, -1, "%dx%d rb=1 have_d0=1 snapw=1 min_cells=0 err=1 gk=0 sw=%s", nx, ny, sw);
      r = mgxk_rbseq_scan_apply(nullptr, &L0, 1, sides(0), 1, 1, (unsigned int *)g_fake, 3, &err, 0, 0);
      wants_d0_line(L0);
      call_ret(r);
    }
}
static void walk_apply_calls(int nz, const char *sw, int depth) {
  static const int NX[] = {2, 15, 64, 66, 128, 130}, NY[] = {2, 100, 128, 130};
  for (const int nx : NX)
    for (const int ny : NY)
      for (int gk = depth == 2 ? 0 : 1; gk <= 1; gk++)
        for (int rb = depth && gk ? 0 : 1; rb <= 1; rb++)
          for (int snapw = depth && gk ? 0 : 1; snapw <= 1; snapw++) {
            const LevView L = level_rb(nx, ny, nz, gk);
            call_head("mgxk_rbseq_walk_apply", nz, -1, "%dx%d rb=%d snapw=%d gk=%d sw=%s", nx, ny, rb, snapw, gk, sw);
            const int r = mgxk_rbseq_walk_apply(nullptr, &L, rb, sides(0), snapw);
            wants_d0_line(L);
            call_ret(r);
          }
}
// kcut = 0, 1, mid, nz, nz + 1 at m = 14 (what the seamount levels take); m = 0, 1, RBW_MAXM = 48 and one more at kcut = nz
static void window_calls(int nz, const char *sw, int depth) {
  static const int NX[] = {8, 12, 64, 65528, 65535, 65536}, NY[] = {2, 63, 100, 128, 130, 512};
  for (const int nx : NX)
    for (const int ny : NY)
      for (int var = 0; var < 10; var++) {
        const int kcut = var == 0 ? 0 : (var == 1 ? 1 : (var == 2 ? nz / 2 : (var == 4 ? nz + 1 : nz)));
        const int m = var == 5 ? 0 : (var == 6 ? 1 : (var == 7 ? 48 : (var == 8 ? 49 : 14)));
        const int gk = var != 9;
        for (int rb = depth == 2 && var == 0 ? 0 : 1; rb <= 1; rb++)
          for (int snapw = depth && var < 5 ? 0 : 1; snapw <= 1; snapw++) {
            const LevView L = level_rb(nx, ny, nz, gk);
            call_head("mgxk_rbseq_window", nz, -1, "%dx%d rb=%d snapw=%d m=%d kcut=%d gk=%d sw=%s", nx, ny, rb, snapw, m, kcut, gk, sw);
            call_ret(mgxk_rbseq_window(nullptr, &L, rb, sides(0), snapw, m, kcut));
          }
      }
}
// waves of a colour times row groups either side of 4096
static void apply_calls(int nz, const char *sw, int depth) {
  static const Shape SH[] = {{16, 16}, {15, 17}, {64, 128}, {128, 128}, {256, 256}, {254, 258}, {512, 512}, {1024, 256}, {4096, 512}};
  for (const Shape &s : SH)
    for (int rb = depth == 2 ? 0 : 1; rb <= 1; rb++)
      for (int snapw = depth ? 0 : 1; snapw <= 1; snapw++) {
        const LevView L = level_rb(s.nx, s.ny, nz, true);
        call_head("mgxk_rbseq_apply", nz, -1, "%dx%d rb=%d snapw=%d sw=%s", s.nx, s.ny, rb, snapw, sw);
        mgxk_rbseq_apply(nullptr, &L, rb, sides(0), snapw);
        call_ret(0);
      }
}
// the launches that choose nothing (one kernel each, sized by the level), the two host functions beside them, and the placement probe's outcomes
static void rbseq_other_calls() {
  switches_default();
  static const Shape SH[] = {{16, 16}, {15, 17}, {256, 256}, {130, 1026}};
  for (const int nz : {2, 5, 64}) {
    for (const Shape &s : SH) {
      const LevView L = level_rb(s.nx, s.ny, nz, true);
      call_head("mgxk_rbseq_setup", nz, -1, "%dx%d", s.nx, s.ny); mgxk_rbseq_setup(nullptr, &L); call_ret(0);
      call_head("mgxk_rbseq_rho", nz, -1, "%dx%d", s.nx, s.ny); mgxk_rbseq_rho(nullptr, &L, g_fake); call_ret(0);
      call_head("mgxk_rbseq_gdecay", nz, -1, "%dx%d", s.nx, s.ny); mgxk_rbseq_gdecay(nullptr, &L, g_fake); call_ret(0);
      call_head("mgxk_rbseq_d0", nz, -1, "%dx%d", s.nx, s.ny); mgxk_rbseq_d0(nullptr, &L, 1); call_ret(0);
    }
    double decay[64];
    for (int cut = 0; cut <= nz; cut++) {
      for (int k = 0; k < nz; k++) decay[k] = k < cut ? 1.0 / (k + 1) : 1e-20;
      call_head("mgxk_rbseq_window_rows", nz, -1, "rows above 2^-64: %d", cut);
      call_ret(mgxk_rbseq_window_rows(decay, nz));
    }
  }
  for (const double rho : {-1.0, 0.0, 1e-301, 0.03, 0.3, 0.39, 0.4, 0.99, 1.0}) {
    call_head("mgxk_rbseq_window_planes", 0, -1, "rho=%g", rho);
    call_ret(mgxk_rbseq_window_planes(rho));
  }
  call_head("mgxk_set_rbseq_timeout", 0, -1, "ms=100");
  call_ret(mgxk_set_rbseq_timeout(100.0));
  // a device whose workgroups 0, 8, 16 ... do not share an XCD (asked, then remembered), a device number past the table, no device: never fused
  int err = 0;
  const LevView L = level_rb(256, 256, 64, true);
  static const int DEV[] = {2, 2, 64, -1, 1};
  for (const int dev : DEV) {
    g_dev = dev; g_probe_equal = dev == 1;
    call_head("mgxk_rbseq_scan_apply", 64, -1, "256x256 rb=1 have_d0=1 snapw=1 min_cells=0 err=1 gk=1 device=%d probe=%s", dev, g_probe_equal ? "equal" : "unequal");
    call_ret(mgxk_rbseq_scan_apply(nullptr, &L, 1, sides(0), 1, 1, (unsigned int *)g_fake, 3, &err, 0, 0));
  }
}

// ---- mgx_resrest.hip: the fused residual + restriction ----
static const char *const RR_SWITCHES[] = {"default", "no_resrest", "resrest_no_zw"};
// zw: bit q set = the q-th of the nine fields the generated slots 4 and 7 need is present
static LevView level_rr(int nx, int ny, int nz, bool zy, int zw) {
  LevView v = level(nx, ny, nz, zy, false);
  double **const f[] = {&v.m4, &v.d4, &v.m7, &v.d7, &v.h2, &v.hi2, &v.ze2};
  for (int q = 0; q < 7; q++) if (zw >> q & 1) *f[q] = g_fake;
  if (zw >> 7 & 1) v.cffw = g_fake;
  if (zw >> 8 & 1) v.csw = g_fake;
  return v;
}
static void rr_call(int nz, const Shape &s, int cv, int real, int partial, int zy, int zw, const char *what, const char *sw) {
  const LevView F = level_rr(s.nx, s.ny, nz, zy, zw);
  const LevView C = level(cv == 1 ? s.nx : s.nx / 2, cv == 2 ? s.ny : s.ny / 2, cv == 3 ? nz : nz / 2, true, false);
  call_head("mgxk_residual_restrict_ex", nz, -1, "%dx%d coarse=%d real=%d partial=%d zy=%d zw=%03x min=%lld flat_max=%lld flat_s=%d ahead=%d (%s) sw=%s", s.nx, s.ny, cv, real, partial, zy, zw,
            g_sw.resrest_min, g_sw.resrest_flat_max, g_sw.resrest_flat_s, g_sw.resrest_ahead, what, sw);
  const int r = mgxk_residual_restrict_ex(nullptr, &F, &C, g_fake, real, sides(0), g_fake, partial ? g_fake : nullptr, nullptr);
  if (partial) printf("  restrict_grid %d\n", mgxk_residual_restrict_grid(&F, &C));   // the norm's partials are sized by it (the test: = the launch's workgroups)
  call_ret(r);
}
// Per shape the flat form (resrest_flat_max = the level's cells: `<=`) and the walking one (one cell less) with every value of their switches, the
// nine fields absent in turn, resrest_min at the level's cells (`<`: served) and one more, and the coarse level not half the fine one
static void resrest_calls(int nz, int isw, int depth) {
  static const Shape SH[] = {{16, 16}, {30, 34}, {64, 64}, {128, 128}, {256, 256}, {258, 256}, {512, 512}};
  const char *sw = RR_SWITCHES[isw];
  for (const Shape &s : SH) {
    const long long cells = (long long)s.nx * s.ny * nz;
    for (int form = 0; form < 3; form++) {   // as the defaults have it, flat, walking
      static const int FLAT_S[] = {0, 2, 4}, AHEAD[] = {11, 12, 21, 13};
      const int nv = form == 0 ? 1 : (form == 1 ? 3 : 4);
      for (int v = 0; v < nv; v++)
        for (int real = depth ? 0 : 1; real <= 1; real++)
          for (int partial = 0; partial <= 1; partial++)
            for (int zw = 0; zw <= 0x1ff; zw += 0x1ff) {
              switches_default();
              g_sw.no_resrest = isw == 1; g_sw.resrest_no_zw = isw == 2;
              if (form) g_sw.resrest_flat_max = form == 1 ? cells : cells - 1;
              if (form == 1) g_sw.resrest_flat_s = FLAT_S[v];
              if (form == 2) g_sw.resrest_ahead = AHEAD[v];
              rr_call(nz, s, 0, real, partial, 1, zw, form == 0 ? "default" : (form == 1 ? "flat" : "walk"), sw);
            }
    }
    switches_default();
    g_sw.no_resrest = isw == 1; g_sw.resrest_no_zw = isw == 2;
    g_sw.resrest_flat_max = cells - 1;
    for (int q = 0; q < 9; q++) rr_call(nz, s, 0, 1, 0, 1, 0x1ff & ~(1 << q), "walk, one field absent", sw);
    if (!depth) continue;
    switches_default();
    for (int more = 0; more <= 1; more++) { g_sw.resrest_min = cells + more; rr_call(nz, s, 0, 1, 1, 1, 0x1ff, "min", sw); }
    switches_default();
    for (int cv = 1; cv <= 3; cv++) rr_call(nz, s, cv, 1, 1, 1, 0x1ff, "coarse not half", sw);
    rr_call(nz, s, 0, 1, 1, 0, 0x1ff, "no slopes", sw);
    const LevView F = level_rr(s.nx, s.ny, nz, true, 0x1ff), C = level(s.nx / 2, s.ny / 2, nz / 2, true, false);
    call_head("mgxk_residual_restrict", nz, -1, "%dx%d real=1 sw=%s", s.nx, s.ny, sw);
    call_ret(mgxk_residual_restrict(nullptr, &F, &C, g_fake, 1, sides(0), g_fake));
  }
  switches_default();
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "names")) {   // mangled stub names on stdin -> the spelling of the launch lines
    char sym[4096];
    while (fgets(sym, sizeof sym, stdin)) {
      sym[strcspn(sym, "\n")] = 0;
      puts(demangled(sym).c_str());
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "refuse")) g_refuse = true;
  else if (argc > 1 && !strcmp(argv[1], "fail")) g_fail = true;
  else if (argc > 1) { fprintf(stderr, "usage: %s [refuse|fail|names]\n", argv[0]); return 2; }
  // the two fall-back passes: the default switches, no variation of sides, slopes and sweep counts
  for (int s = 0; s < (g_refuse || g_fail ? 1 : NSW); s++) {
    const char *sw = set_switch(s);
    const int depth = g_refuse || g_fail ? 1 : (s == 0 ? 2 : 0);
    for (const int nz : NZS) {
      small_calls(nz, sw, depth);
      pass_calls(nz, sw, depth);
    }
  }
  // the snapshot in front of a parallel red-black pass: one launch, sized by the level
  switches_default();
  for (const Shape &s : PASS) {
    const LevView L = level(s.nx, s.ny, 8, true, false);
    call_head("mgxk_snapshot_k1", 8, -1, "%dx%d", s.nx, s.ny);
    mgxk_snapshot_k1(nullptr, &L);
    call_ret(0);
  }
  // the walk of the sequential-order red-black sweep, on a device whose placement probe answers yes
  g_dev = 1; g_probe_equal = true;
  for (int s = 0; s < (g_refuse || g_fail ? 1 : NRBSW); s++) {
    const char *sw = set_rb_switch(s);
    const int depth = g_refuse || g_fail ? 1 : (s == 0 ? 2 : 0);
    for (const int nz : NZS) {
      if (s <= 2) scan_calls(nz, sw, depth);
      if (s == 0 || s == 3) walk_apply_calls(nz, sw, depth);
      if (s == 0 || s >= 4) window_calls(nz, sw, depth);
      if (s == 0) apply_calls(nz, sw, depth);
    }
  }
  rbseq_other_calls();
  for (int s = 0; s < (g_refuse || g_fail ? 1 : 3); s++)
    for (const int nz : NZS) resrest_calls(nz, s, g_refuse || g_fail || s ? 0 : 1);
  return 0;
}

// ---- stand-ins for the HIP runtime: the compiler's registration code and the kernels' host stubs refer to them; none is ever called
// with effect (a launch never reaches a stub: record_shim.h) ----
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned int, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
hipError_t __hipPopCallConfiguration(dim3 *, dim3 *, size_t *, hipStream_t *) { return hipSuccess; }
hipError_t hipLaunchKernel(const void *, dim3, dim3, void **, size_t, hipStream_t) { return hipSuccess; }
// the placement probe of mgx_rbseq.hip (rbseq_placement_ok): the device number the table steers, host memory for the probe's answer, and a
// copy that leaves there what the table asks for -- one XCD for the workgroups 0, 8, 16 ..., or one each
hipError_t hipGetDevice(int *dev) { if (g_dev < 0) return hipErrorNoDevice; *dev = g_dev; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *, size_t n, hipMemcpyKind, hipStream_t) {
  unsigned int *h = (unsigned int *)dst;
  for (size_t q = 0; q < n / sizeof *h; q++) h[q] = g_probe_equal ? (unsigned int)(q % 8) : (unsigned int)q;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
// asked for by the time-limit setters (mgxk_set_rbseq_timeout is called once: it reports the failure) and by wrappers this program does not call (mgxk_relax_ks_persist)
hipError_t hipGetDeviceProperties(hipDeviceProp_t *, int) { return hipErrorNoDevice; }
hipError_t hipMemcpyToSymbol(const void *, const void *, size_t, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *, const void *, int, size_t) { return hipErrorNoDevice; }
}
