// Which launch serves the down leg of a held pair, and which smoother kernel a held level gets: a stand-alone host program (no GPU, no HIP
// runtime) in the pattern of record_main.cpp.  It calls the wrappers of mgx_resrest_held.hip -- compiled host-only behind record_shim.h,
// which sends the launch here -- over shapes, flags and A/B switches either side of every condition of choose_resrest_held
// (mgx_choice_transfer.h), and asks the pure choice functions of mgx_choice.h for the colour pass of the levels that option
// "hold_z_levels" creates: a large even nz on a plane of half or a quarter of level 1's.
// tests/test_hold_z_choice_host.py builds and runs it and compares the lines with tests/golden/hold_z_choice.json.
//
//   record_held_main [fail|names]     fail: hipGetLastError reports an error after every launch; names: as record_main
#include <hip/hip_runtime.h>
#include "mgx_choice.h"
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static Switches g_sw;
const Switches &mgx_switches() { return g_sw; }
thread_local hipError_t mgx_pending_error = hipSuccess;

static bool g_fail = false;
static hipError_t g_err = hipSuccess;
static std::string g_line;

static std::string demangled(const char *sym0) {
  std::string sym = sym0;
  const size_t pad = sym.find("__sanitized_padded_global");
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
void rec_fuse(const Sides &, const int (&)[6], long long, const void *, unsigned int, const void *) {}
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
hipError_t rec_set_attribute(const void *, hipFuncAttribute, int) { return hipSuccess; }

static double g_fake[8];   // never dereferenced: the wrapper only tests pointers and passes them on
static LevView level(int nx, int ny, int nz, bool zy) {
  LevView v;
  memset(&v, 0, sizeof v);
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.EO = 15; v.HO = (16 + ny / 2 + 15) / 16 * 16; v.RS = (v.HO + ny / 2 + 1 + 15) / 16 * 16;
  v.plane = (long long)nz * v.RS;
  double *f = g_fake;
  v.p = v.b = v.r = v.bet = v.gam = v.p1 = f;
  for (double *&a : v.cA) a = f;
  if (zy) { v.zy = v.zx = f; }
  return v;
}
static void switches_default() {
  memset(&g_sw, 0, sizeof g_sw);
  g_sw.ks8 = g_sw.ks64 = g_sw.ksp_fence = g_sw.rbseq_d0_mid = true;
  g_sw.rbw_prio = 1; g_sw.c2f_nt = -1; g_sw.resrest_flat_max = 256LL * 256 * 64; g_sw.resrest_ahead = 11; g_sw.p2p_maxblk = 128; g_sw.p2p_ipt = 1;
}

struct Shape { int nx, ny; };
// coarse columns either side of 16 and of a multiple of it, coarse planes either side of 4; the test shapes; the bench plane and its halves;
// a plane beyond the cache at nz = 64 (the streaming hints)
static const Shape FINE[] = {{2, 2}, {4, 32}, {6, 34}, {8, 30}, {10, 62}, {32, 32}, {48, 80}, {64, 64}, {16, 16}, {128, 128}, {256, 256}, {512, 512}, {1024, 512}};
static const int NZS[] = {2, 3, 4, 5, 8, 12, 16, 32, 40, 64, 80};

static void held_calls() {
  for (int sw = 0; sw < 3; sw++)
    for (const int nz : NZS)
      for (const Shape &s : FINE)
        for (int zy = 0; zy <= 1; zy++)
          for (int real = 0; real <= 1; real++)
            for (int norm = 0; norm <= 1; norm++)
              for (int cv = 0; cv < (sw == 0 && real && zy ? 4 : 1); cv++) {   // the coarse level: held, halved in z as well, not half in x, not half in y
                switches_default();
                if (sw == 1) g_sw.no_resrest = true;
                if (sw == 2) g_sw.resrest_min = 32LL * 32 * 16;
                const LevView F = level(s.nx, s.ny, nz, zy);
                const LevView C = level(cv == 2 ? s.nx : s.nx / 2, cv == 3 ? s.ny : s.ny / 2, cv == 1 ? nz / 2 : nz, zy);
                printf("call mgxk_residual_restrict_held | %dx%dx%d zy=%d real=%d norm=%d coarse=%d sw=%d\n", s.nx, s.ny, nz, zy, real, norm, cv, sw);
                g_err = hipSuccess;
                printf("  held_grid %d\n", mgxk_residual_restrict_held_grid(&F, &C));
                const Sides ph = {1, 1, 1, 1, 0};
                const int r = mgxk_residual_restrict_held(nullptr, &F, &C, g_fake, real, ph, norm ? nullptr : g_fake, norm ? g_fake : nullptr, nullptr);
                printf("  -> %d\n", r);
              }
}

// The levels "hold_z_levels" = 1, 2 puts under 512x512x64, 512x512x32, 256x256x64 and 128x128x16, with their slopes and without (bmask):
// the family and instance of a four-colour pass (nx / 2 planes), of a red-black pass (nx planes, with the snapshot) and of the colour pair
static void smoother_choices() {
  static const int HELD[][3] = {{256, 256, 64}, {128, 128, 64}, {256, 256, 32}, {128, 128, 32}, {64, 64, 64}, {64, 64, 16}, {32, 32, 16}, {32, 32, 12}, {24, 40, 12}};
  switches_default();
  const Sides closed = {1, 1, 1, 1, 0};
  for (const auto &h : HELD)
    for (int zy = 0; zy <= 1; zy++) {
      const LevShape s = {h[0], h[1], h[2], zy != 0, false, false, false, 0};
      for (int rb = 0; rb <= 1; rb++) {
        const int nplanes = rb ? h[0] : h[0] / 2;
        const Choice ks = choose_ks(s, nplanes, 1, rb, g_sw), pr = choose_ks_pair(s, h[0] / 2, closed, g_sw), co = choose_colour(s, nplanes, 1, rb, g_sw);
        printf("smoother %dx%dx%d zy=%d rb=%d | ks family=%d nz=%d nt=%d grid=%u | pair family=%d | colour family=%d nz=%d d=%d mf=%d stream=%d grid=%u by=%u lds=%zu | reg=%d\n",
               h[0], h[1], h[2], zy, rb, ks.family, ks.nz, ks.nt, ks.grid, pr.family, co.family, co.nz, co.d, (int)co.mf, (int)co.stream, co.grid, co.by, co.lds,
               (int)choose_has_reg_kernel(s, g_sw));
      }
    }
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "names")) {
    char sym[4096];
    while (fgets(sym, sizeof sym, stdin)) {
      sym[strcspn(sym, "\n")] = 0;
      puts(demangled(sym).c_str());
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "fail")) g_fail = true;
  else if (argc > 1) { fprintf(stderr, "usage: %s [fail|names]\n", argv[0]); return 2; }
  held_calls();
  if (!g_fail) smoother_choices();
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
}
