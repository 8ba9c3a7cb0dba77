// Which kernel serves which level: a stand-alone host program (no GPU, no HIP runtime) that calls the extern "C" wrappers of
// mgx_wrappers.h -- the smoother's, the sequential-order red-black walk's, the fused residual + restriction's, and those of the operator,
// the transfers, the halo and gather transport, the layout conversions, the Krylov passes and the model coupling -- over a table of shapes,
// flags and A/B switches and prints, per call, one line per kernel launch (the demangled template instance, grid, block, dynamic LDS
// bytes, scalar arguments, by-value structs by their members) and the wrapper's return value.
//
// Built from the units that tests/test_kernel_choice_host.py lists (UNITS), each compiled
// host-only behind record_shim.h, which sends their launches here; the stand-ins at the end of this file replace what the units and the
// compiler's registration code ask of the HIP runtime.
// tests/test_kernel_choice_host.py builds and runs it and compares digests with tests/golden/kernel_choice.json.
//
//   record_main [refuse|fail|names|p2p]     refuse: every hipFuncSetAttribute is refused; fail: hipGetLastError reports an error after every launch;
//                                           p2p: no wrapper is called -- the sweep of the peer-to-peer block plan (p2p_plan_sweep below)
#include <hip/hip_runtime.h>
#include "mgx_choice.h"
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
void rec_text(const char *fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_line += b;
}
void rec_arg(const GeoView &G) { rec_text("G(%d,%d,%d,bmask=%d) ", G.nx, G.ny, G.nz, G.bmask); }
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

static bool g_group_per_wrapper = false;
static void call_head(const char *w, int nz, int method, const char *fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  if (g_group_per_wrapper) printf("call %s nz=* method=- | nz=%d %s\n", w, nz, b);   // one digest per wrapper: the units that only choose a launch
  else if (method >= 0) printf("call %s nz=%d method=%d | %s\n", w, nz, method, b);
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

// ---- mgx_residual.hip, mgx_krylov.hip: the operator of a level and the Krylov passes ----
static LevView32 level32(int nx, int ny, int nz) {
  LevView32 v;
  memset(&v, 0, sizeof v);
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.EO = 31; v.HO = (32 + ny / 2 + 31) / 32 * 32; v.RS = (v.HO + ny / 2 + 1 + 31) / 32 * 32;
  v.plane = (long long)nz * v.RS;
  v.e = v.f = v.r = (float *)g_fake;
  return v;
}
// stored slots or matrix-free either side of nz = 3; cells either side of the Infinity Cache (ch_beyond_cache); odd sizes; more than one block row
static const Shape OPS[] = {{16, 16}, {15, 18}, {130, 126}, {256, 256}, {236, 256}, {238, 256}, {512, 512}, {1024, 1024}};
static void operator_calls(int nz) {
  for (const Shape &s : OPS)
    for (int zy = 0; zy <= 1; zy++) {
      const LevView L = level(s.nx, s.ny, nz, zy, false);
      const LevView32 S = level32(s.nx, s.ny, nz);
      const double *qi[8] = {g_fake, g_fake, g_fake, g_fake, g_fake, g_fake, g_fake, g_fake};
      const int slot[8] = {3, 1, 4, 1, 5, 9, 2, 6};
      int path[4];
      call_head("mgxk_residual_nblocks", nz, -1, "%dx%d zy=%d", s.nx, s.ny, zy);
      call_ret(mgxk_residual_nblocks(&L));
      call_head("mgxq_partials", nz, -1, "%dx%d zy=%d", s.nx, s.ny, zy);
      call_ret((int)mgxq_partials(&L));
      call_head("mgxq_path", nz, -1, "%dx%d zy=%d", s.nx, s.ny, zy);
      mgxq_path(&L, path);
      printf("  path %d %d %d %d\n", path[0], path[1], path[2], path[3]);
      call_ret(0);
      for (int real = 0; real <= 1; real++) {
        for (int norm = 0; norm <= 1; norm++)
          for (int sd = 0; sd <= 1; sd++) {
            call_head("mgxk_residual", nz, -1, "%dx%d zy=%d real=%d norm=%d sides=%d", s.nx, s.ny, zy, real, norm, sd);
            mgxk_residual(nullptr, &L, g_fake, g_fake, real, norm, sides(sd)); call_ret(0);
          }
        for (const int nd : {0, 1, 8}) {
          call_head("mgxq_apply", nz, -1, "%dx%d zy=%d real=%d nd=%d", s.nx, s.ny, zy, real, nd);
          mgxq_apply(nullptr, &L, g_fake, qi, nd, g_fake, g_fake, real); call_ret(0);
          call_head("mgxq_apply32", nz, -1, "%dx%d zy=%d real=%d nd=%d", s.nx, s.ny, zy, real, nd);
          mgxq_apply32(nullptr, &L, &S, 0.5, g_fake, g_fake, qi, nd, g_fake, g_fake, real); call_ret(0);
        }
      }
      if (zy) continue;
      call_head("mgxk_sumsq", nz, -1, "%dx%d", s.nx, s.ny); mgxk_sumsq(nullptr, &L, g_fake, g_fake, g_fake); call_ret(0);
      call_head("mgxk_dot", nz, -1, "%dx%d", s.nx, s.ny); mgxk_dot(nullptr, &L, g_fake, g_fake, g_fake, g_fake); call_ret(0);
      for (const int nd : {0, 3}) {
        call_head("mgxq_ortho", nz, -1, "%dx%d nd=%d", s.nx, s.ny, nd);
        mgxq_ortho(nullptr, &L, g_fake, g_fake, g_fake, qi, qi, slot, nd, g_fake, g_fake, g_fake, g_fake); call_ret(0);
      }
      call_head("mgxq_update", nz, -1, "%dx%d", s.nx, s.ny); mgxq_update(nullptr, &L, g_fake, g_fake, g_fake, g_fake, g_fake, g_fake, g_fake, g_fake); call_ret(0);
      call_head("mgxq_update32", nz, -1, "%dx%d", s.nx, s.ny); mgxq_update32(nullptr, &L, &S, g_fake, g_fake, g_fake, g_fake, 2.0, g_fake, g_fake, g_fake, g_fake); call_ret(0);
    }
  call_head("mgxk_reduce", nz, -1, "n=%d", 100 * nz); mgxk_reduce(nullptr, g_fake, 100 * nz, g_fake); call_ret(0);
}

// ---- mgx_transfer.hip, mgx_hold.hip ----
// The coarse level.  Restriction: its waves either side of 8192 (508 / 512 x 1024), runs of every length down to one level and of the whole
// column.  Prolongation: waves x runs either side of 2048 with runs of 16, 8, 4, 2, 1 levels (at nz = 32: 256, 254, 128, 96, 64 planes) and
// of more levels than the column has (the small nz); rows of more and of less than a wave; odd sizes
static const Shape TR[] = {{8, 8}, {15, 17}, {64, 64}, {96, 128}, {128, 128}, {254, 256}, {256, 256}, {512, 512}, {508, 1024}, {512, 1024}, {1024, 1024}};
static const char *const TR_SWITCHES[] = {"default", "c2f_kc4", "c2f_kc32", "c2f_nt0", "c2f_nt1"};
constexpr int NTRSW = sizeof TR_SWITCHES / sizeof *TR_SWITCHES;
static const char *set_tr_switch(int s) {
  switches_default();
  if (s == 1) g_sw.c2f_kc = 4;
  if (s == 2) g_sw.c2f_kc = 32;
  if (s == 3) g_sw.c2f_nt = 0;
  if (s == 4) g_sw.c2f_nt = 1;
  return TR_SWITCHES[s];
}
// nz: the fine level's; depth 0 (a switch on): the prolongation alone, fine level of twice the size
static void transfer_calls(int nz, const char *sw, int depth) {
  const int nzc = nz / 2;
  for (const Shape &c : TR) {
    const LevView C = level(c.nx, c.ny, nzc, true, false);
    for (int odd = 0; odd < (depth ? 3 : 1); odd++) {   // the fine level: twice the coarse one, one plane more, one column more (SK: even nx, ny only)
      const LevView F = level(2 * c.nx + (odd == 1), 2 * c.ny + (odd == 2), nz, true, false);
      for (int linear = 0; linear <= 1; linear++)
        for (int keep_r = 0; keep_r <= 1; keep_r++)
          for (int skip1 = 0; skip1 <= 1; skip1++) {
            call_head("mgxk_coarse2fine", nz, -1, "%dx%dx%d -> %dx%d linear=%d keep_r=%d skip1=%d sw=%s", c.nx, c.ny, nzc, F.nx, F.ny, linear, keep_r, skip1, sw);
            mgxk_coarse2fine(nullptr, &F, &C, g_fake, linear, sides(0), keep_r, skip1); call_ret(0);
            if (!depth) continue;
            const LevView Ch = level(c.nx, c.ny, nz, true, false);   // a held pair: the same nz
            call_head("mgxk_coarse2fine_held", nz, -1, "%dx%d -> %dx%d linear=%d keep_r=%d skip1=%d", c.nx, c.ny, F.nx, F.ny, linear, keep_r, skip1);
            mgxk_coarse2fine_held(nullptr, &F, &Ch, g_fake, linear, sides(0), keep_r, skip1); call_ret(0);
          }
      if (!depth || odd) continue;
      for (int extra = 0; extra <= 1; extra++) {   // r_c = b_c and p_c = 0 written too, or not
        call_head("mgxk_fine2coarse", nz, -1, "%dx%d -> %dx%dx%d dup=%d zero=%d", F.nx, F.ny, c.nx, c.ny, nzc, extra, extra);
        mgxk_fine2coarse(nullptr, &F, &C, g_fake, sides(extra), extra ? g_fake : nullptr, extra ? g_fake : nullptr); call_ret(0);
        const LevView Ch = level(c.nx, c.ny, nz, true, false);
        call_head("mgxk_fine2coarse_held", nz, -1, "%dx%d -> %dx%d dup=%d zero=%d", F.nx, F.ny, c.nx, c.ny, extra, extra);
        mgxk_fine2coarse_held(nullptr, &F, &Ch, g_fake, sides(extra), extra ? g_fake : nullptr, extra ? g_fake : nullptr); call_ret(0);
      }
    }
  }
}
// chains of 1 to 4 restrictions from a finest level whose nx, ny, nz are multiples of 2^dep, or one of them is not
static void chain_calls() {
  static const int FINE[][3] = {{16, 16, 16}, {32, 48, 16}, {256, 256, 32}, {24, 16, 16}, {16, 40, 16}, {16, 16, 8}, {16, 16, 12}, {18, 16, 16}, {16, 16, 2}, {30, 34, 6}};
  for (const auto &f : FINE)
    for (int dep = 1; dep <= 4; dep++) {
      LevView v[5];
      const LevView *vs[5];
      for (int q = 0; q < 5; q++) {
        const int dv = 1 << (q <= dep ? q : dep);
        v[q] = level(f[0] / dv > 0 ? f[0] / dv : 1, f[1] / dv > 0 ? f[1] / dv : 1, f[2] / dv > 0 ? f[2] / dv : 1, true, false);
        vs[q] = &v[q];
      }
      call_head("mgxk_restrict_chain", f[2], -1, "%dx%d dep=%d", f[0], f[1], dep);
      const int served = mgxk_restrict_chain_served(vs, dep);
      mgxk_restrict_chain(nullptr, vs, dep, sides(0));   // (the wrapper trusts its caller)
      call_ret(served);
    }
}

// ---- mgx_halo.hip ----
static const int PRESENT[][8] = {
    {0, 0, 0, 0, 0, 0, 0, 0},                                                   // no neighbour
    {1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 1, 0},   // one peer: an edge along i, along j, a corner
    {1, 1, 1, 1, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 1, 0, 0},                          // four peers: the edges; two edges and their corner among closed sides
    {1, 1, 1, 1, 1, 1, 1, 1},                                                   // eight peers
    {2, 1, 2, 1, 1, 1, 1, 1}, {1, 2, 1, 2, 1, 1, 1, 1},                          // the wrap local in one direction, peers in the other (their corners: peers)
    {3, 1, 3, 1, 0, 0, 0, 0}, {1, 3, 0, 1, 0, 3, 0, 0},                          // images of closed sides still due beside peers
    {2, 2, 2, 2, 2, 2, 2, 2}, {2, 0, 2, 0, 0, 0, 0, 0},                          // the rank itself everywhere: no peer
};
static const char *const P2P_SWITCHES[] = {"default", "p2p_maxblk1", "p2p_ipt3", "p2p_maxblk1_ipt3"};
static const char *set_p2p_switch(int s) {
  switches_default();
  if (s & 1) g_sw.p2p_maxblk = 1;
  if (s & 2) g_sw.p2p_ipt = 3;
  return P2P_SWITCHES[s];
}
// edges of one block, of several, of more items than 128 blocks take one each (ipt > 1), the sizes whose plan has more than 128 pushing blocks
static const Shape HALO[] = {{2, 2}, {16, 16}, {15, 100}, {128, 128}, {512, 512}, {1000, 1024}, {1738, 2048}, {4096, 4096}};
static void halo_calls(int nz, const char *sw, int depth) {
  double *bufs[8];
  unsigned long long *flags[8];
  for (int d = 0; d < 8; d++) { bufs[d] = g_fake; flags[d] = (unsigned long long *)g_fake; }
  int err = 0, np = -1;
  for (const Shape &s : HALO) {
    const LevView L = level(s.nx, s.ny, nz, true, false);
    for (const auto &present : PRESENT) {
      np++;
      char pat[9];
      for (int d = 0; d < 8; d++) pat[d] = '0' + present[d];
      pat[8] = 0;
      const int mixed[4] = {np % 3, (np + 1) % 3, (np + 2) % 3, np % 2};
      for (int drop = 0; drop <= (depth == 2 ? 1 : 0); drop++) {
        call_head("mgxk_halo_p2p", nz, -1, "%dx%d present=%s drop=%d sw=%s", s.nx, s.ny, pat, drop, sw);
        mgxk_halo_p2p(nullptr, &L, g_fake, bufs, bufs, flags, flags, present, 7 + np, (unsigned int *)g_fake, &err, mixed, drop); call_ret(0);
      }
      if (!depth) continue;
      for (int unpack = 0; unpack <= 1; unpack++) {
        call_head("mgxk_halo_pack_all", nz, -1, "%dx%d present=%s unpack=%d", s.nx, s.ny, pat, unpack);
        mgxk_halo_pack_all(nullptr, &L, g_fake, bufs, present, unpack); call_ret(0);
      }
    }
    if (!depth) continue;
    for (int im = 0; im <= 2; im++)
      for (int jm = 0; jm <= 2; jm++) {
        call_head("mgxk_halo_wrap", nz, -1, "%dx%d im=%d jm=%d", s.nx, s.ny, im, jm);
        mgxk_halo_wrap(nullptr, &L, g_fake, im, jm); call_ret(0);
      }
    call_head("mgxk_halo_phys", nz, -1, "%dx%d", s.nx, s.ny); mgxk_halo_phys(nullptr, &L, g_fake, sides(1)); call_ret(0);
    call_head("mgxk_halo_mixed_corners", nz, -1, "%dx%d", s.nx, s.ny); mgxk_halo_mixed_corners(nullptr, &L, g_fake, 1, 2, 0, 1); call_ret(0);
  }
}
// the gather and the split of a coarse level, the layout conversions (the blocks of a push either side of 256, of a waiting placement either side
// of 128; the conversion tile at nz = 64, 128, 160 and below) and the two one-thread launches
static void gather_layout_calls(int nz) {
  static const Shape SH[] = {{4, 4}, {15, 17}, {30, 32}, {32, 32}, {62, 64}, {64, 64}, {254, 256}, {512, 512}};
  double *dst[4] = {g_fake, g_fake, g_fake, g_fake};
  unsigned long long *flags[4];
  for (auto &f : flags) f = (unsigned long long *)g_fake;
  int err = 0;
  for (const Shape &s : SH) {
    const LevView Cs = level(s.nx, s.ny, nz, true, false), C = level(2 * s.nx, 2 * s.ny, nz, true, false);
    for (const int ng : {2, 4}) {
      call_head("mgxk_gather_push", nz, -1, "%dx%d ng=%d", s.nx, s.ny, ng);
      mgxk_gather_push(nullptr, &Cs, g_fake, dst, flags, ng, 1, 5, (unsigned int *)g_fake, &err); call_ret(0);
    }
    for (int wait = 0; wait <= 1; wait++) {
      call_head("mgxk_gather_place_wait", nz, -1, "%dx%d wait=%d", s.nx, s.ny, wait);
      mgxk_gather_place_wait(nullptr, &C, g_fake, g_fake, s.nx, s.ny, 1, 0, wait ? flags[0] : nullptr, 5, &err); call_ret(0);
    }
    call_head("mgxk_gather_place", nz, -1, "%dx%d", s.nx, s.ny); mgxk_gather_place(nullptr, &C, g_fake, g_fake, s.nx, s.ny, 0, 1); call_ret(0);
    call_head("mgxk_block_to_ref", nz, -1, "%dx%d", s.nx, s.ny); mgxk_block_to_ref(nullptr, &Cs, g_fake, g_fake); call_ret(0);
    call_head("mgxk_split", nz, -1, "%dx%d", s.nx, s.ny); mgxk_split(nullptr, &C, &Cs, g_fake, g_fake, 1, 1); call_ret(0);
    for (int dir = 0; dir <= 1; dir++) {
      call_head("mgxk_convert", nz, -1, "%dx%d dir=%d", s.nx, s.ny, dir); mgxk_convert(nullptr, &Cs, g_fake, g_fake, 8, 3, dir); call_ret(0);
    }
    call_head("mgxk_convert8", nz, -1, "%dx%d", s.nx, s.ny); mgxk_convert8(nullptr, &Cs, g_fake); call_ret(0);
    call_head("mgxk_convert2", nz, -1, "%dx%d", s.nx, s.ny); mgxk_convert2(nullptr, &Cs, g_fake, g_fake, g_fake); call_ret(0);
  }
}
static void one_thread_calls() {
  int err = 0;
  call_head("mgxk_set_p2p_timeout", 0, -1, "ms=100"); call_ret(mgxk_set_p2p_timeout(100.0));
  for (int extra = 0; extra <= 1; extra++) { call_head("mgxk_err_to_double", 0, -1, "extra=%d", extra); mgxk_err_to_double(nullptr, &err, extra, g_fake); call_ret(0); }
  for (const int n : {1, 256, 257}) { call_head("mgxk_divc_selftest", 0, -1, "n=%d", n); mgxk_divc_selftest(nullptr, g_fake, g_fake, n, (unsigned long long *)g_fake); call_ret(0); }
}

// ---- mgx_model.hip ----
static const char *const MODEL_SWITCHES[] = {"default", "model_kr1", "model_kr7", "model_kr8"};
static const int MODEL_KR[] = {0, 1, 7, 8};
// rows: the eight-row floor, the run of the divergence pass either side of 16, columns longer than a run target; waves either side of 16 384
static const int MODEL_NZ[] = {2, 15, 16, 17, 64, 129};
static void model_calls(int nz, const char *sw) {
  static const Shape SH[] = {{16, 16}, {100, 30}, {512, 512}, {1022, 1022}, {1024, 1024}, {2048, 2048}};
  for (const Shape &s : SH) {
    GeoView G;
    memset(&G, 0, sizeof G);
    G.nx = s.nx; G.ny = s.ny; G.nz = nz;
    const LevView L = level(s.nx, s.ny, nz, true, false);
    for (int f32 = 0; f32 <= 1; f32++) {
      const ModelView M = {g_fake, g_fake, g_fake, nullptr, 0, f32};
      call_head("mgxm_rhs_uf", nz, -1, "%dx%d f32=%d sw=%s", s.nx, s.ny, f32, sw); mgxm_rhs_uf(nullptr, &G, &M, g_fake); call_ret(0);
      call_head("mgxm_rhs_vf", nz, -1, "%dx%d f32=%d sw=%s", s.nx, s.ny, f32, sw); mgxm_rhs_vf(nullptr, &G, &M, g_fake); call_ret(0);
      call_head("mgxm_rhs_wf", nz, -1, "%dx%d f32=%d sw=%s", s.nx, s.ny, f32, sw); mgxm_rhs_wf(nullptr, &G, &M, g_fake); call_ret(0);
      call_head("mgxm_correct_uvw", nz, -1, "%dx%d f32=%d sw=%s", s.nx, s.ny, f32, sw); mgxm_correct_uvw(nullptr, &G, g_fake, &M); call_ret(0);
    }
    call_head("mgxm_rhs_accum", nz, -1, "%dx%d sw=%s", s.nx, s.ny, sw); mgxm_rhs_accum(nullptr, &G, g_fake, g_fake, g_fake, g_fake); call_ret(0);
    if (sw != MODEL_SWITCHES[0]) continue;
    call_head("mgxm_ref2model", nz, -1, "%dx%d", s.nx, s.ny); mgxm_ref2model(nullptr, g_fake, g_fake, nz, 2, s.nx, s.ny); call_ret(0);
    call_head("mgxm_ref2model_2d", nz, -1, "%dx%d", s.nx, s.ny); mgxm_ref2model_2d(nullptr, g_fake, g_fake, s.nx, s.ny); call_ret(0);
    call_head("mgxm_js_model", nz, -1, "%dx%d", s.nx, s.ny); mgxm_js_model(nullptr, &L, g_fake, g_fake, 1); call_ret(0);
    for (int face = 0; face <= 1; face++) {
      call_head("mgxm_flux_zero_face", nz, -1, "%dx%d face=%d", s.nx, s.ny, face); mgxm_flux_zero_face(nullptr, &G, g_fake, face, 1); call_ret(0);
      call_head("mgxm_flux_face_copy", nz, -1, "%dx%d face=%d", s.nx, s.ny, face); mgxm_flux_face_copy(nullptr, &G, g_fake, g_fake, face, 1, face); call_ret(0);
    }
  }
}

// ---- the block plan of the peer-to-peer exchange (choose_halo_p2p) by itself: record_main p2p ----
// Over the shapes of halo_calls and a sweep of nz, nx, ny, all 3^4 edge patterns (absent, peer, self; a corner is absent beside an absent edge,
// the rank itself between two self edges, else a peer) and MGX_P2P_MAXBLK = 1, 8, 128: nreal <= maxblk + 7; blk0 does not decrease over the
// present directions and ends at nb, absent directions sit past the end; and nreal <= 128 at maxblk = 128 while nx, ny <= 1024, nz <= 128.
static long long g_p2p_checked = 0, g_p2p_bad = 0;
static int g_p2p_max[3] = {0, 0, 0}, g_p2p_max_small = 0;
static void p2p_check(int nx, int ny, int nz, const int *present, int maxblk, int ipt) {
  switches_default();
  g_sw.p2p_maxblk = maxblk; g_sw.p2p_ipt = ipt;
  const LevShape s = {nx, ny, nz, false, false, false, false, 0};
  const P2pPlan c = choose_halo_p2p(s, present, g_sw);
  bool ok = c.nreal <= maxblk + 7 && c.blk0[8] == c.nb && c.nreal <= c.nb && c.mixed == (c.nreal != c.nb);
  int last = 0;
  for (int d = 0; d < 8; d++) {
    if (!present[d]) { ok = ok && c.blk0[d] == c.nb + 1; continue; }
    ok = ok && c.blk0[d] >= last && c.blk0[d] <= c.nb;
    last = c.blk0[d];
  }
  const bool small = maxblk == 128 && nx <= 1024 && ny <= 1024 && nz <= 128;
  if (small) { ok = ok && c.nreal <= 128; if (c.nreal > g_p2p_max_small) g_p2p_max_small = c.nreal; }
  int &mx = g_p2p_max[maxblk == 1 ? 0 : (maxblk == 8 ? 1 : 2)];
  if (c.nreal > mx) mx = c.nreal;
  g_p2p_checked++;
  if (!ok) {
    g_p2p_bad++;
    printf("violation %dx%dx%d present=%d%d%d%d%d%d%d%d maxblk=%d ipt_min=%d: ipt=%d nb=%d nreal=%d blk0=%d,%d,%d,%d,%d,%d,%d,%d,%d\n", nx, ny, nz, present[0], present[1], present[2],
           present[3], present[4], present[5], present[6], present[7], maxblk, ipt, c.ipt, c.nb, c.nreal, c.blk0[0], c.blk0[1], c.blk0[2], c.blk0[3], c.blk0[4], c.blk0[5], c.blk0[6],
           c.blk0[7], c.blk0[8]);
  }
}
static int p2p_plan_sweep() {
  static const int MAXBLK[] = {1, 8, 128};
  for (const Shape &s : HALO)
    for (const int nz : {1, 2, 3, 16, 64, 80, 128})
      for (const auto &present : PRESENT)
        for (const int maxblk : MAXBLK)
          for (const int ipt : {1, 3}) p2p_check(s.nx, s.ny, nz, present, maxblk, ipt);
  static const int NZ[] = {1, 2, 3, 4, 8, 16, 32, 64, 80, 128}, NXY[] = {2, 16, 100, 128, 512, 1000, 1024, 2048, 4096};
  for (int pat = 0; pat < 81; pat++) {
    int present[8];
    for (int d = 0, q = pat; d < 4; d++, q /= 3) present[d] = q % 3 == 2 ? HALO_SELF : q % 3;
    static const int CORNER[4][2] = {{0, 3}, {0, 1}, {2, 1}, {2, 3}};   // SW, SE, NE, NW: the two edges a corner lies between
    for (int q = 0; q < 4; q++) {
      const int a = present[CORNER[q][0]], b = present[CORNER[q][1]];
      present[4 + q] = !a || !b ? HALO_NONE : (a == HALO_SELF && b == HALO_SELF ? HALO_SELF : HALO_PEER);
    }
    for (const int nz : NZ)
      for (const int nx : NXY)
        for (const int ny : NXY)
          for (const int maxblk : MAXBLK) p2p_check(nx, ny, nz, present, maxblk, 1);
  }
  printf("p2p_plan checked=%lld violations=%lld max_nreal maxblk1=%d maxblk8=%d maxblk128=%d maxblk128_to_1024x1024x128=%d\n", g_p2p_checked, g_p2p_bad, g_p2p_max[0], g_p2p_max[1],
         g_p2p_max[2], g_p2p_max_small);
  return g_p2p_bad ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "p2p")) return p2p_plan_sweep();
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
  else if (argc > 1) { fprintf(stderr, "usage: %s [refuse|fail|names|p2p]\n", argv[0]); return 2; }
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
  // the units that choose a launch and nothing else: they report nothing, so the fall-back passes take their default switches only
  const bool plain = !g_refuse && !g_fail;
  g_group_per_wrapper = true;
  switches_default();
  for (const int nz : NZS) operator_calls(nz);
  for (int s = 0; s < (plain ? NTRSW : 1); s++) {
    const char *sw = set_tr_switch(s);
    for (const int nz : NZS) transfer_calls(nz, sw, s == 0);
  }
  switches_default();
  chain_calls();
  for (int s = 0; s < (plain ? 4 : 1); s++) {
    const char *sw = set_p2p_switch(s);
    for (const int nz : {1, 2, 3, 16, 64, 80, 128}) halo_calls(nz, sw, s == 0 ? (plain ? 2 : 1) : 0);
  }
  switches_default();
  for (const int nz : {1, 2, 5, 32, 64, 128, 160}) gather_layout_calls(nz);
  one_thread_calls();
  for (int s = 0; s < (plain ? 4 : 1); s++) {
    switches_default();
    g_sw.model_kr = MODEL_KR[s];
    for (const int nz : MODEL_NZ) model_calls(nz, MODEL_SWITCHES[s]);
  }
  switches_default();
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
