// The C ABI of libmgx.so declared in include/mgx.h: instances, thin entry points over the host functions of mgx_cycle.cpp, mgx_comm.cpp
// and mgx_define.cpp (mgx_host.h), the run-time options, field access, timers and the namelist.  mgx_init / mgx_clean are in
// mgx_define.cpp, the mgx_p2p_* and mgx_rccl_* entry points in mgx_comm.cpp.
// There is no CPU compute path: every operator is a HIP kernel launch (mgx_wrappers.h).
#include "mgx_host.h"
#include "mgx_export.h"
#include "mgx_state_view.h"
#include "mgx_depth_view.h"

namespace mgx_host {

State S0;
std::vector<State *> g_instances = {&S0};
std::mutex g_instances_mu;
__thread State *Sp = &S0;
int live_instances() {
  std::lock_guard<std::mutex> lk(g_instances_mu);
  int n = 0;
  for (State *q : g_instances) if (q && q->inited) n++;
  return n;
}

int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  S.err = buf;
  if (S.verbose) fprintf(stderr, "mgx error: %s\n", buf);
  return 1;
}

// ---- run-time options: ONE table ---------------------------------------------------------------------------------
// Per option: its name, where its value lives in State (`at`) or how it is read when it is not a plain int member (`get`), the
// environment variable that presets it at mgx_init and what that variable means (its presence alone, or its value), who may touch
// it, and whether it outlives mgx_clean.  mgx_set_option, mgx_get_option, mgx_init (options_from_env) and mgx_clean
// (options_carried / options_restore) walk this table; the options with behaviour of their own are the explicit cases in front of
// the walk in mgx_set_option.  Precedence: the defaults in State, then the environment at mgx_init, then mgx_set_option.
// What mgx_clean carries is what it carried when the list was two hand-written lines: "rb_chain", "rbseq_rowcut" and "rbseq_d0_in_pass"
// go back to their defaults while "rbseq_window", "rbseq_fuse" and "rbseq_fuse_min" beside them stay -- kept as found.
// ("verbose" outlives mgx_clean too: by mgx_clean's own line, with the stream and the comm hooks, which are not options.)
enum { ENV_NONE, ENV_ZERO, ENV_ONE, ENV_ATOI };   // the variable's presence means 0, means 1, or its value is parsed
enum { RW, RO, WO };                              // RO: namelist members and counters; WO: test hooks
struct Opt { const char *name; int State::*at; int (*get)(const State &); const char *env; int env_rule; int access; bool carried; };
#define PAR(m) [](const State &s) { return (int)s.par.m; }
#define CNT(m) [](const State &s) { return (int)s.m; }
const Opt OPTIONS[] = {
  // the namelist members (the reference's drivers `use mg_namelist` and read e.g. `bmask` directly)
  {"bmask", nullptr, PAR(bmask), nullptr, ENV_NONE, RO, false},
  {"nsmall", nullptr, PAR(nsmall), nullptr, ENV_NONE, RO, false},
  {"solver_maxiter", nullptr, PAR(solver_maxiter), nullptr, ENV_NONE, RO, false},
  {"ns_coarsest", nullptr, PAR(ns_coarsest), nullptr, ENV_NONE, RO, false},
  {"ns_pre", nullptr, PAR(ns_pre), nullptr, ENV_NONE, RO, false},
  {"ns_post", nullptr, PAR(ns_post), nullptr, ENV_NONE, RO, false},
  {"netcdf_output", nullptr, PAR(netcdf_output), nullptr, ENV_NONE, RO, false},
  {"aggressive", nullptr, PAR(aggressive), nullptr, ENV_NONE, RO, false},
  // name                 value in State            read by        environment                rule      access carried
  {"warm_start",          &State::warm_start,       nullptr,       nullptr,                   ENV_NONE, RW, true},
  {"tictoc",              &State::tictoc,           nullptr,       "MGX_TICTOC",              ENV_ONE,  RW, true},
  {"exact_halos",         &State::exact_halos,      nullptr,       "MGX_EXACT_HALOS",         ENV_ONE,  RW, true},
  {"verbose",             &State::verbose,          nullptr,       nullptr,                   ENV_NONE, RW, false},
  {"rb_chain",            &State::rb_chain,         nullptr,       nullptr,                   ENV_NONE, RW, false},
  {"rb_exact",            &State::rb_exact,         nullptr,       "MGX_RB_EXACT",            ENV_ATOI, RW, true},
  {"rb_seq",              &State::rb_seq,           nullptr,       "MGX_RB_SEQ",              ENV_ATOI, RW, true},
  {"keep_r",              &State::keep_r,           nullptr,       nullptr,                   ENV_NONE, RW, true},
  {"c2f_skip",            &State::c2f_skip,         nullptr,       "MGX_C2F_NOSKIP",          ENV_ZERO, RW, true},
  {"fuse_closing",        &State::fuse_closing,     nullptr,       "MGX_NO_FUSE_CLOSING",     ENV_ZERO, RW, true},
  {"restrict_chain",      &State::use_chain,        nullptr,       "MGX_NO_RESTRICT_CHAIN",   ENV_ZERO, RW, true},
  {"rbseq_fuse",          &State::rbseq_fuse,       nullptr,       "MGX_NO_RBSEQ_FUSE",       ENV_ZERO, RW, true},
  {"rbseq_window",        &State::rbseq_window,     nullptr,       "MGX_NO_RBSEQ_WINDOW",     ENV_ZERO, RW, true},
  {"rbseq_rowcut",        &State::rbseq_rowcut,     nullptr,       nullptr,                   ENV_NONE, RW, false},
  {"rbseq_fuse_min",      &State::rbseq_fuse_min,   nullptr,       nullptr,                   ENV_NONE, RW, true},
  {"rbseq_d0_in_pass",    &State::rbseq_d0_in_pass, nullptr,       nullptr,                   ENV_NONE, RW, false},
  {"coarsest_direct",     &State::coarsest_direct,  nullptr,       "MGX_COARSEST_DIRECT",     ENV_ATOI, RW, true},
  {"overlap",             &State::overlap,          nullptr,       "MGX_OVERLAP",             ENV_ATOI, RW, true},
  {"async",               &State::async_ops,        nullptr,       nullptr,                   ENV_NONE, RW, true},
  {"fuse_tail",           &State::use_fuse,         nullptr,       nullptr,                   ENV_NONE, RW, true},
  {"cycle_precision",     &State::cycle_precision,  nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 32 / 64 only
  {"krylov",              &State::krylov,           nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0..8 only
  {"krylov_precision",    &State::krylov_precision, nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 32 / 64 only (no preset: the table's would pass any number by)
  {"mixed_tail",          &State::mixed_tail,       nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only
  {"mixed_ring",          &State::mixed_ring,       nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only
  {"mixed_direct",        &State::mixed_direct,     nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only
  {"small_any_nz",        &State::small_any_nz,     nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only
  {"periodic",            &State::periodic,         nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0..3 only, and not while initialised (read by mgx_init)
  {"hold_odd_nz",         &State::hold_odd_nz,      nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only, and not while initialised (read by mgx_init)
  {"hold_z_levels",       &State::hold_z_levels,    nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0..8 only, and not while initialised (read by mgx_init)
  {"hold_z_fuse",         &State::hold_z_fuse,      nullptr,       nullptr,                   ENV_NONE, RW, true},   // set: 0 / 1 only
  // reads as off while a time-out of this solver holds (ksp_down, which mgx_clean does not carry); set: see mgx_set_option
  {"ksp",                 &State::use_ksp,          [](const State &s) { return (s.use_ksp && !s.ksp_down) ? 1 : 0; }, "MGX_NO_KSP", ENV_ZERO, RW, true},
  {"p2p",                 nullptr,                  [](const State &s) { return s.p2p_on ? 1 : 0; }, nullptr, ENV_NONE, RW, false},   // set: see mgx_set_option
  {"ksp_test_stall",      &State::ksp_test_stall,   nullptr,       nullptr,                   ENV_NONE, WO, false},
  {"rbseq_test_stall",    &State::rbseq_test_stall, nullptr,       nullptr,                   ENV_NONE, WO, false},
  {"p2p_test_drop",       &State::p2p_test_drop,    nullptr,       nullptr,                   ENV_NONE, WO, false},
  // counters
  {"coarsest_direct_solves", nullptr, CNT(n_direct), nullptr, ENV_NONE, RO, false},
  {"rbseq_window_colours", nullptr, CNT(n_window), nullptr, ENV_NONE, RO, false},
  {"overlapped_passes", nullptr, CNT(n_overlap), nullptr, ENV_NONE, RO, false},
  {"tall_stored_passes", nullptr, CNT(n_tall_stored), nullptr, ENV_NONE, RO, false},
  {"mixed_iterations", nullptr, CNT(n_mixed), nullptr, ENV_NONE, RO, false},
  {"mixed_tail_launches", nullptr, CNT(n_mixed_tail), nullptr, ENV_NONE, RO, false},
  {"mixed_ring_passes", nullptr, CNT(n_mixed_ring), nullptr, ENV_NONE, RO, false},
  {"mixed_direct_solves", nullptr, CNT(n_mixed_direct), nullptr, ENV_NONE, RO, false},
  {"small_any_nz_calls", nullptr, CNT(n_small_any), nullptr, ENV_NONE, RO, false},
  {"krylov_restarts", nullptr, CNT(kr_restarts), nullptr, ENV_NONE, RO, false},
  {"krylov_mixed_iterations", nullptr, CNT(n_kr_mixed), nullptr, ENV_NONE, RO, false},
  {"p2p_failed", nullptr, CNT(p2p_failed), nullptr, ENV_NONE, RO, false},
  {"zeta_refreshes", nullptr, CNT(n_zeta_refresh), nullptr, ENV_NONE, RO, false},
  {"zeta_chain_launches", nullptr, CNT(n_zeta_chain), nullptr, ENV_NONE, RO, false},
  {"hold_z_fused", nullptr, CNT(n_hold_z_fused), nullptr, ENV_NONE, RO, false},
  {"depth_refreshes", nullptr, CNT(n_depth_refresh), nullptr, ENV_NONE, RO, false},
};
#undef PAR
#undef CNT
const Opt *find_option(const char *name) {
  for (const Opt &o : OPTIONS) if (streq(o.name, name)) return &o;
  return nullptr;
}

void options_from_env() {
  for (const Opt &o : OPTIONS) {
    const char *e = o.env ? getenv(o.env) : nullptr;
    if (e) S.*o.at = o.env_rule == ENV_ATOI ? atoi(e) : (o.env_rule == ENV_ONE ? 1 : 0);
  }
}
std::vector<int> options_carried() {
  std::vector<int> v;
  for (const Opt &o : OPTIONS) if (o.carried) v.push_back(S.*o.at);
  return v;
}
void options_restore(const std::vector<int> &v) {
  size_t q = 0;
  for (const Opt &o : OPTIONS) if (o.carried) S.*o.at = v[q++];
}
}  // namespace mgx_host
using namespace mgx_host;

// ====================================================================================================
extern "C" {

// ---- instances (see the comment at State S0) --------------------------------------------------------------------------------
int mgx_instance_create(void) {
  std::lock_guard<std::mutex> lk(g_instances_mu);
  for (size_t q = 1; q < g_instances.size(); q++) if (!g_instances[q]) { g_instances[q] = new State(); return (int)q; }
  g_instances.push_back(new State());
  return (int)g_instances.size() - 1;
}
int mgx_instance_select(int id) {
  std::lock_guard<std::mutex> lk(g_instances_mu);
  if (id < 0 || id >= (int)g_instances.size() || !g_instances[id]) return fail("mgx_instance_select: no instance %d", id);
  Sp = g_instances[id];
  return 0;
}
int mgx_instance_current(void) {
  std::lock_guard<std::mutex> lk(g_instances_mu);
  for (size_t q = 0; q < g_instances.size(); q++) if (g_instances[q] == Sp) return (int)q;
  return -1;
}
// the calling thread must have selected another instance (or 0) before; instance 0 cannot be destroyed
int mgx_instance_destroy(int id) {
  State *victim = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_instances_mu);
    if (id < 1 || id >= (int)g_instances.size() || !g_instances[id]) return fail("mgx_instance_destroy: no instance %d (instance 0 is permanent)", id);
    victim = g_instances[id];
    g_instances[id] = nullptr;
  }
  State *mine = Sp;
  Sp = victim;
  mgx_clean();
  Sp = (mine == victim) ? &S0 : mine;
  delete victim;
  return 0;
}

const char *mgx_last_error(void) { return S.err.c_str(); }
const char *mgx_version(void) { return "mgx 0.1 (gfx950)"; }
int mgx_set_verbose(int v) { S.verbose = v; return 0; }
int mgx_set_stream(void *st) { S.stream = (hipStream_t)st; return 0; }
int mgx_set_comm(mgx_exchange_fn ex, mgx_allreduce_fn ar, mgx_allgather_fn ag, void *ctx) { S.ex = ex; S.ar = ar; S.ag = ag; S.ctx = ctx; S.native_rccl = false; return 0; }

int mgx_params_default(mgx_params *p) {
  memset(p, 0, sizeof(*p));
  p->solver_prec = 1e-6; p->solver_maxiter = 50; p->nsmall = 8; p->ns_coarsest = 40; p->ns_pre = 3; p->ns_post = 2;
  strcpy(p->cmatrix, "real"); strcpy(p->relax_method, "RB"); strcpy(p->interp_type, "linear"); strcpy(p->restrict_type, "avg");
  return 0;
}

int mgx_read_namelist(const char *path, mgx_params *p) {
  FILE *f = fopen(path ? path : "nh_namelist", "r");
  if (!f) return 0;  // defaults stay (mg_namelist.f90:75-86)
  // Fortran namelist rules as far as /nhparam/ needs them (checked against read_nhnamelist of the reference compiled with flang,
  // tests/golden/ref_namelist.json): group and member names in any case; `!` starts a comment outside a string; assignments are
  // separated by commas, blanks or line ends; the group ends at `/`.
  std::string txt; char line[1024];
  while (fgets(line, sizeof(line), f)) {
    std::string s(line); char q = 0; size_t c = std::string::npos;
    for (size_t t = 0; t < s.size(); t++) {
      if (q) { if (s[t] == q) q = 0; }
      else if (s[t] == '\'' || s[t] == '"') q = s[t];
      else if (s[t] == '!') { c = t; break; }
    }
    if (c != std::string::npos) s = s.substr(0, c);
    txt += s + "\n";
  }
  fclose(f);
  std::string low = txt;
  for (auto &ch : low) ch = (char)tolower(ch);
  size_t a = low.find("&nhparam");
  if (a == std::string::npos) return fail("namelist group &nhparam not found in %s", path ? path : "nh_namelist");
  size_t pos = a + 8;
  const std::string ws = " \t\r\n,";
  for (;;) {
    pos = txt.find_first_not_of(ws, pos);
    if (pos == std::string::npos || txt[pos] == '/') break;
    size_t ke = pos;
    while (ke < txt.size() && (isalnum((unsigned char)txt[ke]) || txt[ke] == '_')) ke++;
    size_t eq = txt.find_first_not_of(" \t\r\n", ke);
    if (ke == pos || eq == std::string::npos || txt[eq] != '=') return fail("cannot parse namelist statement near '%s'", txt.substr(pos, 24).c_str());
    std::string key = low.substr(pos, ke - pos);
    size_t vb = txt.find_first_not_of(" \t\r\n", eq + 1), ve;
    if (vb == std::string::npos) return fail("namelist member '%s' has no value", key.c_str());
    std::string val, sv;
    if (txt[vb] == '\'' || txt[vb] == '"') {
      ve = txt.find(txt[vb], vb + 1);
      if (ve == std::string::npos) return fail("unterminated string for namelist member '%s'", key.c_str());
      sv = txt.substr(vb + 1, ve - vb - 1); val = sv; ve++;
    } else {
      ve = txt.find_first_of(" \t\r\n,/", vb);
      if (ve == std::string::npos) ve = txt.size();
      val = txt.substr(vb, ve - vb); sv = val;
    }
    pos = ve;
    auto num = [&](void) { std::string t = val; for (auto &ch : t) if (ch == 'd' || ch == 'D') ch = 'e'; return atof(t.c_str()); };
    auto lg = [&](void) { std::string t = val; for (auto &ch : t) ch = (char)tolower(ch); return (t.find(".t") == 0 || t.find("t") == 0) ? 1 : 0; };
    if (key == "solver_prec") p->solver_prec = num();
    else if (key == "solver_maxiter") p->solver_maxiter = (int)num();
    else if (key == "nsmall") p->nsmall = (int)num();
    else if (key == "ns_coarsest") p->ns_coarsest = (int)num();
    else if (key == "ns_pre") p->ns_pre = (int)num();
    else if (key == "ns_post") p->ns_post = (int)num();
    else if (key == "cmatrix") snprintf(p->cmatrix, 16, "%s", sv.c_str());
    else if (key == "relax_method") snprintf(p->relax_method, 16, "%s", sv.c_str());
    else if (key == "interp_type") snprintf(p->interp_type, 16, "%s", sv.c_str());
    else if (key == "restrict_type") snprintf(p->restrict_type, 16, "%s", sv.c_str());
    else if (key == "aggressive") p->aggressive = lg();
    else if (key == "netcdf_output") p->netcdf_output = lg();
    else if (key == "bmask") p->bmask = lg();
    else return fail("'%s' is not a member of namelist /nhparam/", key.c_str());  // a Fortran read would abort too
  }
  if (streq(p->interp_type, "linear") && streq(p->restrict_type, "linear")) return fail("linear interp + linear restrict is not permitted");
  return 0;
}

// nhydro_matrices from host (dev = false) or device (dev = true) arrays: the level-1 geometry, then define_matrices
static int matrices_from(const double *dx, const double *dy, const double *zeta, const double *h, const double *rmask, double hc,
                         double theta_b, double theta_s, bool dev) {
  NEED_INIT();
  if (S.par.bmask && !rmask) return fail("bmask=.true. needs rmask in mgx_matrices (nhydro.f90:52-55)");
  if (S.verbose && S.rank == 0) printf("  nhydro_matrices:\n");
  S.hlim = hc; S.theta_b = theta_b; S.theta_s = theta_s;
  Level &L = S.lev[0];
  const size_t n2 = (size_t)(L.ny + 2) * (L.nx + 2) * sizeof(double);
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(L.g.dx, dx, n2, kind, S.stream));
  HIPCHK(hipMemcpyAsync(L.g.dy, dy, n2, kind, S.stream));
  HIPCHK(hipMemcpyAsync(L.g.zeta, zeta, n2, kind, S.stream));
  HIPCHK(hipMemcpyAsync(L.g.h, h, n2, kind, S.stream));
  if (S.par.bmask) HIPCHK(hipMemcpyAsync(L.g.rmask, rmask, n2, kind, S.stream));  // grid(1)%rmask = rmask
  return define_matrices(DM_ALL, dev);
}

int mgx_matrices(const double *dx, const double *dy, const double *zeta, const double *h, const double *rmask, double hc,
                 double theta_b, double theta_s) {
  return matrices_from(dx, dy, zeta, h, rmask, hc, theta_b, theta_s, false);
}

int mgx_matrices_device(const double *dx_dev, const double *dy_dev, const double *zeta_dev, const double *h_dev, const double *rmask_dev,
                        double hc, double theta_b, double theta_s) {
  return matrices_from(dx_dev, dy_dev, zeta_dev, h_dev, rmask_dev, hc, theta_b, theta_s, true);
}

// the per-step call of a resident model with a moving free surface: a new level-1 zeta, everything that depends on it rebuilt
int mgx_update_zeta_device(const double *zeta_dev) {
  NEED_INIT();
  if (!S.have_geometry) return fail("mgx_update_zeta_device: no dx, dy, h to keep: call mgx_matrices or mgx_matrices_device first");
  if (!zeta_dev) return fail("mgx_update_zeta_device: zeta_dev is NULL");
  if (S.depths_user) return fail("mgx_update_zeta_device: the depths in use are the caller's (mgx_matrices_depths): there is no h and no stretching to apply a new zeta to; hand over the new depths with mgx_update_depths_device");
  Level &L = S.lev[0];
  HIPCHK(hipMemcpyAsync(L.g.zeta, zeta_dev, (size_t)(L.ny + 2) * (L.nx + 2) * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
  CHK(define_matrices(DM_ZETA, true));
  S.n_zeta_refresh++;
  return 0;
}

// the same refresh from the model's own zeta: i fastest, rows sj elements apart.  One transpose into the level-1 array, then as above.
int mgx_update_zeta_device_view(const double *zeta_dev, long long sj) {
  NEED_INIT();
  if (!S.have_geometry) return fail("mgx_update_zeta_device_view: no dx, dy, h to keep: call mgx_matrices or mgx_matrices_device first");
  if (!zeta_dev) return fail("mgx_update_zeta_device_view: zeta_dev is NULL");
  if (S.depths_user) return fail("mgx_update_zeta_device_view: the depths in use are the caller's (mgx_matrices_depths): there is no h and no stretching to apply a new zeta to; hand over the new depths with mgx_update_depths_device");
  Level &L = S.lev[0];
  long long last;
  if (sj < L.nx + 2) return fail("mgx_update_zeta_device_view: sj = %lld is below the row length of zeta, %d: rows would overlap", sj, L.nx + 2);
  if (__builtin_mul_overflow(sj, (long long)L.ny + 1, &last) || last > LLONG_MAX / 8 - (L.nx + 2))
    return fail("mgx_update_zeta_device_view: sj = %lld: the extent of zeta does not fit in 63 bits", sj);
  mgxs_zeta_view(S.stream, zeta_dev, sj, L.g.zeta, L.nx, L.ny); S.n_launch++;
  CHK(define_matrices(DM_ZETA, true));
  S.n_zeta_refresh++;
  return 0;
}

// ---- the matrices from the caller's own vertical grid (include/mgx.h: mgx_matrices_depths*) ----
// the caller's zr, zw into the interior of the level-1 arrays: host arrays (the dense layout only) by two pitched copies, device arrays by
// k_depths_copy (dense, s == nullptr) or k_depths_in (the model's i-fastest padded arrays)
static int depths_in(const double *zr, const double *zw, const mgx_depth_strides *s, bool dev, const char *who) {
  Level &L = S.lev[0];
  if (!zr || !zw) return fail("%s: zr or zw is NULL", who);
  if (s) {
    char why[256];
    if (depth_strides_refusal(L.nx, L.ny, L.nz, s, why, sizeof why)) return fail("%s: %s", who, why);
    mgxd_in(S.stream, zr, zw, s, &L.g); S.n_launch++;
  } else if (dev) {
    mgxd_copy(S.stream, zr, zw, &L.g); S.n_launch++;
  } else {  // per plane i the interior rows j = 1..ny are one run of ny columns
    const double *src[2] = {zr, zw}; double *dst[2] = {L.g.zr, L.g.zw};
    for (int q = 0; q < 2; q++) {
      const size_t nzz = (size_t)L.nz + q, pitch = (size_t)(L.ny + 4) * nzz * sizeof(double), first = ((size_t)2 * (L.ny + 4) + 2) * nzz;
      HIPCHK(hipMemcpy2DAsync(dst[q] + first, pitch, src[q] + first, pitch, (size_t)L.ny * nzz * sizeof(double), (size_t)L.nx, hipMemcpyHostToDevice, S.stream));
    }
  }
  return 0;
}

// a pair of levels halves an odd nz: define_matrices refuses such a hierarchy, and the entries ask before they touch level 1
static bool depths_unserved() {
  for (int l = 1; l < S.nlevs; l++)
    if (S.lev[l].nz != S.lev[l - 1].nz && (S.lev[l - 1].nz & 1)) return true;
  return false;
}

static int matrices_depths_from(const double *dx, const double *dy, const double *zr, const double *zw, const mgx_depth_strides *s, const double *rmask,
                                bool dev, const char *who) {
  NEED_INIT();
  if (!dx || !dy) return fail("%s: dx or dy is NULL", who);
  if (S.par.bmask && !rmask) return fail("bmask=.true. needs rmask in %s (nhydro.f90:52-55)", who);
  if (S.verbose && S.rank == 0) printf("  nhydro_matrices (depths):\n");
  Level &L = S.lev[0];
  const size_t n2 = (size_t)(L.ny + 2) * (L.nx + 2) * sizeof(double);
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // (refusals first: nothing of the level is touched by a call that is refused)
  if (!zr || !zw) return fail("%s: zr or zw is NULL", who);
  char why[256];
  if (s && depth_strides_refusal(L.nx, L.ny, L.nz, s, why, sizeof why)) return fail("%s: %s", who, why);
  if (depths_unserved()) return define_matrices(DM_DEPTHS_ALL, dev);   // its refusal, in its words
  HIPCHK(hipMemcpyAsync(L.g.dx, dx, n2, kind, S.stream));
  HIPCHK(hipMemcpyAsync(L.g.dy, dy, n2, kind, S.stream));
  if (S.par.bmask) HIPCHK(hipMemcpyAsync(L.g.rmask, rmask, n2, kind, S.stream));
  CHK(depths_in(zr, zw, s, dev, who));
  return define_matrices(DM_DEPTHS_ALL, dev);
}

int mgx_depth_strides_check(int nx, int ny, int nz, const mgx_depth_strides *s) {
  char why[256];
  return depth_strides_refusal(nx, ny, nz, s, why, sizeof why) ? fail("mgx_depth_strides_check: %s", why) : 0;
}
int mgx_matrices_depths(const double *dx, const double *dy, const double *zr, const double *zw, const double *rmask) {
  return matrices_depths_from(dx, dy, zr, zw, nullptr, rmask, false, "mgx_matrices_depths");
}
int mgx_matrices_depths_device(const double *dx_dev, const double *dy_dev, const double *zr_dev, const double *zw_dev, const mgx_depth_strides *s,
                               const double *rmask_dev) {
  return matrices_depths_from(dx_dev, dy_dev, zr_dev, zw_dev, s, rmask_dev, true, "mgx_matrices_depths_device");
}
// the per-step call of a resident model that owns its vertical grid: new depths under the dx, dy, rmask of the last set-up
int mgx_update_depths_device(const double *zr_dev, const double *zw_dev, const mgx_depth_strides *s) {
  NEED_INIT();
  if (!S.have_geometry) return fail("mgx_update_depths_device: no dx, dy to keep: call mgx_matrices_depths, mgx_matrices_depths_device or mgx_matrices first");
  if (depths_unserved()) return define_matrices(DM_DEPTHS, true);   // its refusal, in its words
  CHK(depths_in(zr_dev, zw_dev, s, true, "mgx_update_depths_device"));
  CHK(define_matrices(DM_DEPTHS, true));
  S.n_depth_refresh++;
  return 0;
}
// the launches of mgx_depths.hip for a level 1 of nx x ny x nz (mgx_choice_depths.h); pure host logic
int mgx_depths_launch(int nx, int ny, int nz, int *out) {
  if (!out) return fail("mgx_depths_launch: out is NULL");
  if (nx < 2 || ny < 2 || nz < 2 || (nx & 1) || (ny & 1)) return fail("mgx_depths_launch: %d x %d x %d is not a level-1 size", nx, ny, nz);
  mgxd_choice(nx, ny, nz, out);
  return 0;
}

// The model-facing entries, each once for both scalar types of the state (f32: u, v, w are floats; include/mgx.h: "the float state").
// `who` names the entry in its refusals.  The float entries refuse a NULL u, v or w; the fp64 ones keep taking what they are given.
#define NEED_STATE(who) do { if (f32 && !(u && v && w)) return fail("%s: u, v or w is NULL", who); } while (0)
// the view entries (str != nullptr; the dense entries pass by): the strides against the live level 1 (mgx_state_view.h), and no NULL array
static int view_refusal(const void *u, const void *v, const void *w, const mgx_state_strides *str, const char *who) {
  char why[256];
  const Level &L = S.lev[0];
  if (state_strides_refusal(L.nx, L.ny, L.nz, str, why, sizeof why)) return fail("%s: %s", who, why);
  if (!(u && v && w)) return fail("%s: u, v or w is NULL", who);
  return 0;
}
#define NEED_VIEW(who) do { if (str) CHK(view_refusal(u, v, w, str, who)); } while (0)

static int compute_rhs_host(const void *u, const void *v, const void *w, const double *rmask, bool f32, const char *who) {
  NEED_INIT();
  if (!S.have_matrix) return fail("mgx_matrices must be called before %s", who);
  NEED_STATE(who);
  CHK(set_call_mask(rmask, false));
  StateScope state(nullptr, nullptr, nullptr, f32);   // the staging buffers, as doubles or as floats
  CHK(upload_uvw(u, v, w, f32 ? sizeof(float) : sizeof(double)));
  CHK(compute_rhs_dev());
  CHK(sync_stream());
  return 0;
}

static int solve_host(void *u, void *v, void *w, const double *rmask, bool f32, const char *who) {
  NEED_INIT();
  if (!S.have_matrix) return fail("mgx_matrices must be called before %s", who);
  NEED_STATE(who);
  if (S.verbose && S.rank == 0) printf("  nhydro_solve:\n");
  CHK(set_call_mask(rmask, false));
  StateScope state(nullptr, nullptr, nullptr, f32);
  const size_t esz = f32 ? sizeof(float) : sizeof(double);
  CHK(upload_uvw(u, v, w, esz));
  CHK(compute_rhs_dev());
  CHK(solve_p_opt(S.par.solver_prec, S.par.solver_maxiter, nullptr, nullptr, nullptr));
  CHK(correct_uvw_dev());
  CHK(download_uvw(u, v, w, esz));
  CHK(sync_stream());
  return 0;
}

// Device-resident variant of nhydro_solve: u,v,w are DEVICE pointers in the model's (i,j,k) layout
// (e.g. torch tensors); nothing crosses PCIe.  The library's own staging copies are bypassed.
// str: u, v, w are the model's own padded arrays with these strides (the *_view entries), checked before anything else is looked at.
static int solve_device(void *u, void *v, void *w, const double *rmask, bool f32, const char *who, const mgx_state_strides *str = nullptr) {
  NEED_INIT();
  NEED_VIEW(who);
  if (!S.have_matrix) return fail("mgx_matrices must be called before %s", who);
  NEED_STATE(who);
  CHK(set_call_mask(rmask, true));
  StateScope state(u, v, w, f32, str);
  CHK(compute_rhs_dev());
  CHK(solve_p_opt(S.par.solver_prec, S.par.solver_maxiter, nullptr, nullptr, nullptr));
  CHK(correct_uvw_dev());
  CHK(sync_stream());
  return 0;
}

// nhydro_check_nondivergence on the model's own device arrays (the pattern of mgx_solve_device): the divergence into grid(1)%b
static int check_nondivergence_device(void *u, void *v, void *w, const double *rmask, bool f32, const char *who, const mgx_state_strides *str = nullptr) {
  NEED_INIT();
  NEED_VIEW(who);
  if (!S.have_matrix) return fail("mgx_matrices must be called before %s", who);
  NEED_STATE(who);
  if (S.verbose && S.rank == 0) printf(" - check non-divergence:\n");
  CHK(set_call_mask(rmask, true));
  StateScope state(u, v, w, f32, str);
  CHK(compute_rhs_dev());
  CHK(sync_stream());
  return 0;
}

int mgx_compute_rhs(const double *u, const double *v, const double *w, const double *rmask) { return compute_rhs_host(u, v, w, rmask, false, "compute_rhs"); }
int mgx_compute_rhs_f32(const float *u, const float *v, const float *w, const double *rmask) { return compute_rhs_host(u, v, w, rmask, true, "mgx_compute_rhs_f32"); }
int mgx_solve(double *u, double *v, double *w, const double *rmask) { return solve_host(u, v, w, rmask, false, "mgx_solve"); }
int mgx_solve_f32(float *u, float *v, float *w, const double *rmask) { return solve_host(u, v, w, rmask, true, "mgx_solve_f32"); }
int mgx_solve_device(double *u_dev, double *v_dev, double *w_dev, const double *rmask) { return solve_device(u_dev, v_dev, w_dev, rmask, false, "mgx_solve_device"); }
int mgx_solve_device_f32(float *u_dev, float *v_dev, float *w_dev, const double *rmask_dev) { return solve_device(u_dev, v_dev, w_dev, rmask_dev, true, "mgx_solve_device_f32"); }
int mgx_check_nondivergence(double *u, double *v, double *w, const double *rmask) {
  if (S.verbose && S.rank == 0) printf(" - check non-divergence:\n");
  return mgx_compute_rhs(u, v, w, rmask);
}
int mgx_check_nondivergence_f32(float *u, float *v, float *w, const double *rmask) {
  if (S.verbose && S.rank == 0) printf(" - check non-divergence:\n");
  return compute_rhs_host(u, v, w, rmask, true, "mgx_check_nondivergence_f32");
}
int mgx_check_nondivergence_device(double *u_dev, double *v_dev, double *w_dev, const double *rmask_dev) {
  return check_nondivergence_device(u_dev, v_dev, w_dev, rmask_dev, false, "mgx_check_nondivergence_device");
}
int mgx_check_nondivergence_device_f32(float *u_dev, float *v_dev, float *w_dev, const double *rmask_dev) {
  return check_nondivergence_device(u_dev, v_dev, w_dev, rmask_dev, true, "mgx_check_nondivergence_device_f32");
}

int mgx_state_strides_check(int nx, int ny, int nz, const mgx_state_strides *s) {
  char why[256];
  return state_strides_refusal(nx, ny, nz, s, why, sizeof why) ? fail("mgx_state_strides_check: %s", why) : 0;
}
int mgx_solve_device_view(void *u, void *v, void *w, const mgx_state_strides *s, int f32, const double *rmask_dev) {
  if (!s) return fail("mgx_solve_device_view: the strides are NULL");
  return solve_device(u, v, w, rmask_dev, f32 != 0, "mgx_solve_device_view", s);
}
int mgx_check_nondivergence_device_view(void *u, void *v, void *w, const mgx_state_strides *s, int f32, const double *rmask_dev) {
  if (!s) return fail("mgx_check_nondivergence_device_view: the strides are NULL");
  return check_nondivergence_device(u, v, w, rmask_dev, f32 != 0, "mgx_check_nondivergence_device_view", s);
}

int mgx_solve_p(double tol, int maxite, int *nite, double *res, double *hist) {
  NEED_INIT();
  if (!S.have_matrix) return fail("no matrix: call mgx_matrices (or mgx_set_field(lev, MGX_CA, ...)) first");
  return solve_p_opt(tol, maxite, nite, res, hist);
}
int mgx_fcycle(void) { NEED_INIT(); CHK(fcycle()); CHK(op_sync()); return 0; }
int mgx_vcycle(int lev) { NEED_LEV(lev); CHK(vcycle(lev)); CHK(op_sync()); return 0; }
int mgx_vcycle2(int lev1, int lev2) { NEED_LEV(lev1); NEED_LEV(lev2); if (lev2 < lev1) return fail("Vcycle2: lev2 < lev1"); CHK(vcycle2(lev1, lev2)); CHK(op_sync()); return 0; }
int mgx_relax(int lev, int nsweeps) { NEED_LEV(lev); CHK(relax(lev, nsweeps)); CHK(op_sync()); return 0; }
int mgx_residual(int lev, double *res) { NEED_LEV(lev); double r; CHK(residual(lev, &r)); if (res) *res = r; return 0; }
int mgx_fine2coarse(int lev) { NEED_LEV(lev); if (lev >= S.nlevs) return fail("fine2coarse(%d): no coarser level", lev); CHK(fine2coarse(lev)); CHK(op_sync()); return 0; }
int mgx_coarse2fine(int lev) { NEED_LEV(lev); if (lev >= S.nlevs) return fail("coarse2fine(%d): no coarser level", lev); CHK(coarse2fine(lev)); CHK(op_sync()); return 0; }
// the generic fill_halo(lev, field) of mg_mpi_exchange.f90:10-16: 3-D solver fields p, b, r (fill_halo_3D[_relax], nh = 1), the 2-D
// geometry dx, dy, zeta, h (fill_halo_2D), zr / zw (fill_halo_3D with nh = 2: extrapolation at physical sides, :956-964) and the
// 4-D cA (fill_halo_4D: neighbour exchange only).  Collective over the ranks.
int mgx_fill_halo(int lev, int field) {
  NEED_LEV(lev);
  Level &L = S.lev[lev - 1];
  switch (field) {
    case MGX_P: CHK(fill_halo_js(L, L.v.p)); break;
    case MGX_B: CHK(fill_halo_js(L, L.v.b)); L.b_halo_stale = false; break;
    case MGX_R: CHK(fill_halo_js(L, L.v.r)); L.r_halo_stale = false; break;
    case MGX_CA: for (int s = 0; s < 8; s++) CHK(fill_halo_js(L, L.v.cA[s], true, true)); break;
    case MGX_DX: CHK(rl_fill_halo(L, L.g.dx, 1, 1, 0)); break;
    case MGX_DY: CHK(rl_fill_halo(L, L.g.dy, 1, 1, 0)); break;
    case MGX_ZETA: CHK(rl_fill_halo(L, L.g.zeta, 1, 1, 0)); break;
    case MGX_H: CHK(rl_fill_halo(L, L.g.h, 1, 1, 0)); break;
    case MGX_ZR: CHK(rl_fill_halo(L, L.g.zr, L.nz, 2, 0)); break;
    case MGX_ZW: CHK(rl_fill_halo(L, L.g.zw, L.nz + 1, 2, 0)); break;
    default: return fail("fill_halo: field %d has no halo rule (p, b, r, cA, dx, dy, zeta, h, zr, zw)", field);
  }
  CHK(op_sync());  // option "async": enqueued only, like the cycles
  return 0;
}

// testgalerkin(lev) (mg_solvers.f90:203-288): energy of a coarse field under the coarse operator against the energy of its
// interpolation under the fine one.  The reference fills grid(lev)%p with random_number; here the caller provides it
// (mgx_set_field(lev, MGX_P, ...)), everything after that is the reference's sequence.  b of both levels is zeroed, as there.
int mgx_testgalerkin(int lev, double *norm_c, double *norm_f) {
  NEED_LEV(lev);
  if (lev < 2) return fail("testgalerkin(%d): needs a finer level lev-1", lev);
  if (!S.have_matrix) return fail("testgalerkin: no matrix");
  double nc = 0, nf = 0;
  for (int pass = 0; pass < 2; pass++) {
    Level &L = S.lev[pass == 0 ? lev - 1 : lev - 2];
    const int l = pass == 0 ? lev : lev - 1;
    if (pass == 0) CHK(fill_halo_js(L, L.v.p));                                   // call fill_halo(lev,grid(lev)%p)
    else {
      HIPCHK(hipMemsetAsync(L.v.p, 0, L.n3js * sizeof(double), S.stream));        // grid(lev-1)%p = 0
      CHK(coarse2fine(l));                                                         // interpolate p to r and add r to p
    }
    HIPCHK(hipMemsetAsync(L.v.b, 0, L.n3js * sizeof(double), S.stream));          // grid(.)%b = 0
    CHK(residual(l, nullptr));
    mgxk_dot(S.stream, &L.v, L.v.p, L.v.r, S.d_partial, S.d_scalar); S.n_launch += 2;  // norm(lev,p,r,...) -> global_sum
    double s; CHK(global_sum(L, &s));
    (pass == 0 ? nc : nf) = s;
  }
  if (S.verbose && S.rank == 0)
    printf(" ======== lev %12d ===========\n norm coarse = %24.16E\n norm fine   = %24.16E\n ratio       = %24.16E\n", lev, nc, nf / 4, nc / nf * 4);
  if (norm_c) *norm_c = nc;
  if (norm_f) *norm_f = nf;
  return 0;
}

// ---- the CSR export: A of a level, R and P of a pair of levels, as the kernels apply them (include/mgx.h) ----
// Probing, not a second spelling of the operator: the library's own residual / fine2coarse / coarse2fine is applied to sums of unit vectors
// that no row can confuse (the colours of mgx_export.h), and the entries are read off the result -- one times a coefficient and sums with
// zeros are exact, so every value is the number the kernels use, with the level's halo rule, the masks and the k = 1 diagonals of
// cmatrix = 'real' folded in by the kernels themselves.  Two sweeps over the colours: the first marks which colours each row answers to
// (its bit mask, whose population counts are scanned into rowptr), the second scatters the entries into their sorted slots.
namespace {
// What an export borrows and gives back bit for bit: whole JS arrays (halo and padding included), the deferred-halo flags, the timers' switch.
struct Borrowed {
  struct Field { double *at, *copy; size_t n; };
  std::vector<Field> fields;
  std::vector<std::pair<bool *, bool>> flags;
  std::vector<void *> scratch;
  int tictoc;
  Borrowed() : tictoc(S.tictoc) { S.tictoc = 0; }
  int field(double *a, size_t n) {
    double *c = nullptr;
    HIPCHK(hipMalloc((void **)&c, n * sizeof(double)));
    fields.push_back({a, c, n});
    HIPCHK(hipMemcpyAsync(c, a, n * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
    return 0;
  }
  void flag(bool *f) { flags.push_back({f, *f}); }
  int alloc(void **p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes));
    scratch.push_back(*p);
    return 0;
  }
  int give_back() {
    int rc = 0;
    for (const Field &f : fields)
      if (hipMemcpyAsync(f.at, f.copy, f.n * sizeof(double), hipMemcpyDeviceToDevice, S.stream) != hipSuccess) rc = fail("the export could not put a borrowed field back");
    const int rs = sync_stream();
    for (const Field &f : fields) (void)hipFree(f.copy);
    for (void *p : scratch) (void)hipFree(p);
    for (const auto &f : flags) *f.first = f.second;
    S.tictoc = tictoc;
    return rc ? rc : rs;
  }
};
}  // namespace

// which: -1 = A of level lev, 0 = R (lev -> lev + 1), 1 = P (lev + 1 -> lev).  rowptr == nullptr: count only (the *_size entries)
static int export_csr(const char *who, int lev, int which, long long *nrows, long long *ncols, long long *nnz, int *rowptr, int *col, double *val) {
  NEED_LEV(lev);
  const bool size_only = rowptr == nullptr && col == nullptr && val == nullptr;
  if (which < -1 || which > 1) return fail("%s: which = %d is neither 0 (the restriction) nor 1 (the prolongation)", who, which);
  if (which >= 0 && lev >= S.nlevs) return fail("%s(%d): no coarser level", who, lev);
  if (S.npx * S.npy > 1) return fail("%s: a process grid (%d x %d) is out of scope: the export numbers the unknowns of one rank", who, S.npx, S.npy);
  if (!S.have_matrix) return fail("%s: no matrix: call mgx_matrices (or mgx_set_field(lev, MGX_CA, ...)) first", who);
  if (!size_only && (!rowptr || !col || !val)) return fail("%s: rowptr, col and val must all be device pointers", who);
  Level &F = S.lev[lev - 1];
  Level &C = S.lev[which >= 0 ? lev : lev - 1];
  if (which >= 0 && (C.gather || F.nx != 2 * C.nx || F.ny != 2 * C.ny || (C.nz != F.nz && C.nz != F.nz / 2)))
    return fail("%s(%d): levels %d x %d x %d and %d x %d x %d are not a pair the export knows", who, lev, F.nx, F.ny, F.nz, C.nx, C.ny, C.nz);
  const int mode = which < 0 ? EX_A : (which == 0 ? EX_R : EX_P);
  Level &Lr = mode == EX_R ? C : F, &Lc = mode == EX_P ? C : F;   // rows, columns (A: both the level itself)
  const int *nb = Lc.neighb;
  if ((nb[0] < 0) != (nb[2] < 0) || (nb[1] < 0) != (nb[3] < 0)) return fail("%s(%d): a level closed on one side and open on the other has no halo rule the export knows", who, lev);
  const ExMap m = ex_map(mode, Lr.nx, Lr.ny, Lr.nz, Lc.nx, Lc.ny, Lc.nz, nb[0] < 0 ? EX_MIRROR : EX_WRAP, nb[1] < 0 ? EX_MIRROR : EX_WRAP);
  const int ncolours = ex_ncolours(m);
  if (ncolours > EX_MAX_COLOURS) return fail("%s(%d): a periodic level of %d x %d columns needs %d colours, the export has %d", who, lev, Lc.nx, Lc.ny, ncolours, EX_MAX_COLOURS);
  const long long nr = (long long)Lr.nx * Lr.ny * Lr.nz, nc = (long long)Lc.nx * Lc.ny * Lc.nz;
  if (ex_fits_int(nr, nc, 0)) return fail("%s(%d): %lld rows and %lld columns do not fit the int indices of rowptr and col", who, lev, nr, nc);
  if (!size_only && (S.ex_lev != lev || S.ex_which != which)) return fail("%s(%d): call %s_size for this matrix first: it says how large col and val must be", who, lev, who);

  Borrowed B;
  long long total = -1;
  const auto body = [&]() -> int {
    unsigned long long *mask = nullptr; long long *sums = nullptr;
    const int nsums = mgxe_csr_sums_len(nr);
    CHK(B.alloc((void **)&mask, (size_t)nr * sizeof(unsigned long long)));
    CHK(B.alloc((void **)&sums, (size_t)nsums * sizeof(long long)));
    B.flag(&F.r_halo_stale);
    if (mode == EX_A) { CHK(B.field(F.v.p, F.n3js)); CHK(B.field(F.v.b, F.n3js)); CHK(B.field(F.v.r, F.n3js)); }
    if (mode == EX_R) { CHK(B.field(F.v.r, F.n3js)); CHK(B.field(C.v.b, C.n3js)); CHK(B.field(C.v.p, C.n3js)); B.flag(&C.b_halo_stale); }
    if (mode == EX_P) { CHK(B.field(F.v.p, F.n3js)); CHK(B.field(F.v.r, F.n3js)); CHK(B.field(C.v.p, C.n3js)); }
    if (mode == EX_A) HIPCHK(hipMemsetAsync(F.v.b, 0, F.n3js * sizeof(double), S.stream));
    // the probe of one colour through the library's own operator; returns the field of the ROW level that holds the answer
    double *probe_in = mode == EX_A ? F.v.p : (mode == EX_R ? F.v.r : C.v.p);
    const double *answer = mode == EX_A ? F.v.r : (mode == EX_R ? C.v.b : F.v.p);
    const auto probe = [&](int colour) -> int {
      mgxe_probe_fill(S.stream, &Lc.v, probe_in, &m, colour); S.n_launch++;
      CHK(fill_halo_js(Lc, probe_in));
      if (mode == EX_A) return residual(lev, nullptr);
      if (mode == EX_R) return fine2coarse(lev);
      HIPCHK(hipMemsetAsync(F.v.p, 0, F.n3js * sizeof(double), S.stream));
      return coarse2fine(lev);
    };
    HIPCHK(hipMemsetAsync(mask, 0, (size_t)nr * sizeof(unsigned long long), S.stream));
    for (int c = 0; c < ncolours; c++) { CHK(probe(c)); mgxe_csr_mark(S.stream, &Lr.v, answer, &m, c, mask); S.n_launch++; }
    mgxe_csr_count(S.stream, mask, nr, sums); S.n_launch += 2;
    HIPCHK(hipMemcpyAsync(&total, sums + nsums - 1, sizeof total, hipMemcpyDeviceToHost, S.stream));
    CHK(sync_stream());
    if (ex_fits_int(nr, nc, total)) return fail("%s(%d): %lld entries do not fit the int indices of rowptr", who, lev, total);
    if (size_only) return 0;
    if (total != S.ex_nnz) return fail("%s(%d): the matrix has %lld entries, %s_size counted %lld: it changed in between, ask again", who, lev, total, who, S.ex_nnz);
    mgxe_csr_rowptr(S.stream, mask, nr, sums, rowptr); S.n_launch++;
    for (int c = 0; c < ncolours; c++) { CHK(probe(c)); mgxe_csr_scatter(S.stream, &Lr.v, answer, &m, c, mask, rowptr, col, val, mode == EX_A ? -1.0 : 1.0); S.n_launch++; }
    return 0;
  };
  const int rc = body(), rb = B.give_back();
  if (rc || rb) return rc ? rc : rb;
  if (size_only) { S.ex_lev = lev; S.ex_which = which; S.ex_nnz = total; }
  if (nrows) *nrows = nr;
  if (ncols) *ncols = nc;
  if (nnz) *nnz = total;
  return 0;
}
int mgx_operator_csr_size(int lev, long long *nrows, long long *nnz) { return export_csr("mgx_operator_csr", lev, -1, nrows, nullptr, nnz, nullptr, nullptr, nullptr); }
int mgx_operator_csr(int lev, int *rowptr_dev, int *col_dev, double *val_dev) {
  if (!rowptr_dev || !col_dev || !val_dev) return fail("mgx_operator_csr: rowptr, col and val must all be device pointers");
  return export_csr("mgx_operator_csr", lev, -1, nullptr, nullptr, nullptr, rowptr_dev, col_dev, val_dev);
}
int mgx_transfer_csr_size(int lev, int which, long long *nrows, long long *ncols, long long *nnz) {
  if (which != 0 && which != 1) return fail("mgx_transfer_csr: which = %d is neither 0 (the restriction) nor 1 (the prolongation)", which);
  return export_csr("mgx_transfer_csr", lev, which, nrows, ncols, nnz, nullptr, nullptr, nullptr);
}
int mgx_transfer_csr(int lev, int which, int *rowptr_dev, int *col_dev, double *val_dev) {
  if (which != 0 && which != 1) return fail("mgx_transfer_csr: which = %d is neither 0 (the restriction) nor 1 (the prolongation)", which);
  if (!rowptr_dev || !col_dev || !val_dev) return fail("mgx_transfer_csr: rowptr, col and val must all be device pointers");
  return export_csr("mgx_transfer_csr", lev, which, nullptr, nullptr, nullptr, rowptr_dev, col_dev, val_dev);
}

static int level_table(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int hold, int hold_z, int maxlev, int *out) {
  if (nx < 2 || ny < 2 || nz < 2 || npx < 1 || npy < 1 || rank < 0 || rank >= npx * npy || periodic < 0 || periodic > 3 || hold < 0 || hold > 1 || hold_z < 0 || hold_z > 8) return -1;
  const int nl = find_grid_levels(npx, npy, nx, ny, nz, hold, hold_z);
  if (nl < 1 || nl > maxlev) return -1;
  std::vector<Level> T(nl);
  T[0].nx = nx; T[0].ny = ny; T[0].nz = nz;
  rank_level_table(rank, T, npx, npy, nsmall, periodic, hold, hold_z);
  for (int l = 0; l < nl; l++) {
    const Level &L = T[l];
    const int v[12] = {L.nx, L.ny, L.nz, L.npx, L.npy, L.incx, L.incy, L.gather, L.ngx, L.ngy, L.key, L.color};
    memcpy(out + 20 * l, v, sizeof(v)); memcpy(out + 20 * l + 12, L.neighb, 8 * sizeof(int));
  }
  return nl;
}
int mgx_level_table(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int maxlev, int *out) {
  return level_table(nx, ny, nz, npx, npy, rank, nsmall, 0, 0, 0, maxlev, out);
}
int mgx_level_table_periodic(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int maxlev, int *out) {
  return level_table(nx, ny, nz, npx, npy, rank, nsmall, periodic, 0, 0, maxlev, out);
}
int mgx_level_table_hold(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int hold, int maxlev, int *out) {
  return level_table(nx, ny, nz, npx, npy, rank, nsmall, periodic, hold, 0, maxlev, out);
}
int mgx_level_table_semi(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int hold, int hold_z, int maxlev, int *out) {
  return level_table(nx, ny, nz, npx, npy, rank, nsmall, periodic, hold, hold_z, maxlev, out);
}
// the m of option "hold_z_levels" that squares the cells of a rank's block: the smallest m in 0..8 with 2^m min(dx, dy) >= max(h) / nz over the interior
int mgx_hold_z_hint(const double *dx, const double *dy, const double *h, int nx, int ny, int nz, int *m) {
  if (!dx || !dy || !h || !m) return fail("mgx_hold_z_hint: dx, dy, h or m is NULL");
  if (nx < 1 || ny < 1 || nz < 1) return fail("mgx_hold_z_hint: %d x %d x %d is not a level-1 size", nx, ny, nz);
  double dmin = 0.0, hmax = 0.0;
  for (int i = 1; i <= nx; i++)
    for (int j = 1; j <= ny; j++) {
      const size_t q = (size_t)i * (ny + 2) + j;   // (0:ny+1, 0:nx+1), j fastest
      const double d = dx[q] < dy[q] ? dx[q] : dy[q];
      if ((i == 1 && j == 1) || d < dmin) dmin = d;
      if ((i == 1 && j == 1) || h[q] > hmax) hmax = h[q];
    }
  if (!(dmin > 0.0) || !(hmax > 0.0) || !std::isfinite(dmin) || !std::isfinite(hmax)) return fail("mgx_hold_z_hint: dx, dy and h must be positive and finite over the interior (min(dx, dy) = %g, max(h) = %g)", dmin, hmax);
  int q = 0;
  while (q < 8 && ldexp(dmin, q) < hmax / nz) q++;
  *m = q;
  return 0;
}
// the first level of the tail of an fp32 cycle (option "mixed_tail") on a one-rank hierarchy, 0 = no level is small
int mgx_mixed_tail_first(int nx, int ny, int nz, int *first) {
  if (!first) return fail("mgx_mixed_tail_first: first is NULL");
  if (nx < 2 || ny < 2 || nz < 2) return fail("mgx_mixed_tail_first: %d x %d x %d is not a level-1 size", nx, ny, nz);
  const int nl = find_grid_levels(1, 1, nx, ny, nz);
  if (nl < 1) return fail("mgx_mixed_tail_first: %d x %d x %d has no hierarchy", nx, ny, nz);
  std::vector<Level> T(nl);
  T[0].nx = nx; T[0].ny = ny; T[0].nz = nz;
  rank_level_table(0, T, 1, 1, 8);
  *first = 0;
  for (int lev = nl; lev >= 1 && mixed_tail_small(T[lev - 1].nx, T[lev - 1].ny, T[lev - 1].nz); lev--) *first = lev;
  return 0;
}
// the levels whose fp32 colour passes option "mixed_ring" hands to k_relax32r on a one-rank hierarchy: bit lev-1 of *mask (choose_relax32)
int mgx_mixed_ring_levels(int nx, int ny, int nz, int *mask) {
  if (!mask) return fail("mgx_mixed_ring_levels: mask is NULL");
  if (nx < 2 || ny < 2 || nz < 2) return fail("mgx_mixed_ring_levels: %d x %d x %d is not a level-1 size", nx, ny, nz);
  const int nl = find_grid_levels(1, 1, nx, ny, nz);
  if (nl < 1 || nl > 31) return fail("mgx_mixed_ring_levels: %d x %d x %d has no hierarchy", nx, ny, nz);
  std::vector<Level> T(nl);
  T[0].nx = nx; T[0].ny = ny; T[0].nz = nz;
  rank_level_table(0, T, 1, 1, 8);
  *mask = 0;
  for (int lev = 1; lev <= nl; lev++) {
    int c[6];
    mgxx_ring_choice(T[lev - 1].nx, T[lev - 1].ny, T[lev - 1].nz, T[lev - 1].nx, c);
    if (c[0]) *mask |= 1 << (lev - 1);
  }
  return 0;
}
// the launch choose_relax32 names for a colour pass of nplanes planes of a level of nx x ny x nz under option "mixed_ring" = 1
int mgx_mixed_ring_choice(int nx, int ny, int nz, int nplanes, int *out) {
  if (!out) return fail("mgx_mixed_ring_choice: out is NULL");
  if (nx < 2 || ny < 2 || nz < 2 || nplanes < 1 || nplanes > nx) return fail("mgx_mixed_ring_choice: %d planes of %d x %d x %d is not a colour pass of a level", nplanes, nx, ny, nz);
  mgxx_ring_choice(nx, ny, nz, nplanes, out);
  return 0;
}
// cells of the coarsest level of a one-rank hierarchy where option "mixed_direct" serves its solve as a product, 0 = the sweeps (choose_mixed_direct_cells)
int mgx_mixed_direct_cells(int nx, int ny, int nz, int any_nz, int *cells) {
  if (!cells) return fail("mgx_mixed_direct_cells: cells is NULL");
  if (nx < 2 || ny < 2 || nz < 2) return fail("mgx_mixed_direct_cells: %d x %d x %d is not a level-1 size", nx, ny, nz);
  const int nl = find_grid_levels(1, 1, nx, ny, nz);
  if (nl < 1) return fail("mgx_mixed_direct_cells: %d x %d x %d has no hierarchy", nx, ny, nz);
  std::vector<Level> T(nl);
  T[0].nx = nx; T[0].ny = ny; T[0].nz = nz;
  rank_level_table(0, T, 1, 1, 8);
  *cells = mgxx_direct32_cells(T[nl - 1].nx, T[nl - 1].ny, T[nl - 1].nz, nl, any_nz ? 1 : 0);
  return 0;
}
int mgx_exchange_plan(const int *neighb, int rank, int *entries, int *self_mask) {
  if (!neighb || !entries) return -1;
  XEntry pl[8];
  const int n = exchange_plan(neighb, rank, pl, self_mask);
  for (int t = 0; t < n; t++) { entries[3 * t] = pl[t].peer; entries[3 * t + 1] = pl[t].sd; entries[3 * t + 2] = pl[t].rd; }
  return n;
}

int mgx_set_option(const char *name, int value) {
  // the options with behaviour of their own
  if (streq(name, "cycle_precision") && value != 32 && value != 64) return fail("cycle_precision must be 64 (fp64 cycles) or 32 (fp32 cycles under fp64 refinement), got %d", value);
  if (streq(name, "krylov_precision") && value != 32 && value != 64) return fail("krylov_precision must be 64 (fp64 cycles under the Krylov loop) or 32 (fp32 cycles under it), got %d", value);
  if (streq(name, "krylov") && (value < 0 || value > 8)) return fail("krylov must be 0 (off) or 1..8 (retained direction pairs of the truncated GCR), got %d", value);
  if (streq(name, "mixed_tail") && value != 0 && value != 1) return fail("mixed_tail must be 1 (the small levels of an fp32 cycle in one launch) or 0 (one launch per colour pass and transfer), got %d", value);
  if (streq(name, "mixed_ring") && value != 0 && value != 1) return fail("mixed_ring must be 1 (the fp32 colour passes of the levels that are not small by the pipelined kernel) or 0 (k_relax32 on every level), got %d", value);
  if (streq(name, "mixed_direct") && value != 0 && value != 1) return fail("mixed_direct must be 1 (the coarsest solve of an fp32 cycle as one matrix-vector product) or 0 (ns_coarsest sweeps), got %d", value);
  if (streq(name, "small_any_nz") && value != 0 && value != 1) return fail("small_any_nz must be 1 (closed levels of at most 1024 columns with nz = 3, 5, 6, 7 relax in one launch) or 0 (one launch per colour pass), got %d", value);
  if (streq(name, "periodic")) {
    if (value < 0 || value > 3) return fail("periodic must be 0 (closed), 1 (the i direction, east-west), 2 (the j direction, north-south) or 3 (both), got %d", value);
    if (S.inited && value != S.periodic)
      return fail("periodic = %d: the hierarchy in use was built with periodic = %d and the option takes effect at mgx_init: call mgx_clean, set it, then mgx_init", value, S.periodic);
  }
  if (streq(name, "hold_odd_nz")) {
    if (value != 0 && value != 1) return fail("hold_odd_nz must be 0 (every level halves nz, the reference's hierarchy) or 1 (an odd nz is held on the coarser levels), got %d", value);
    if (S.inited && value != S.hold_odd_nz)
      return fail("hold_odd_nz = %d: the hierarchy in use was built with hold_odd_nz = %d and the option takes effect at mgx_init: call mgx_clean, set it, then mgx_init", value, S.hold_odd_nz);
  }
  if (streq(name, "hold_z_fuse") && value != 0 && value != 1) return fail("hold_z_fuse must be 1 (the down leg of a held pair as one kernel) or 0 (compute_residual and the 2-D restriction as two launches), got %d", value);
  if (streq(name, "hold_z_levels")) {
    if (value < 0 || value > 8) return fail("hold_z_levels must be 0 (every coarsening halves nz, the reference's hierarchy) or m = 1..8 (the first m coarsenings keep nz), got %d", value);
    if (S.inited && value != S.hold_z_levels)
      return fail("hold_z_levels = %d: the hierarchy in use was built with hold_z_levels = %d and the option takes effect at mgx_init: call mgx_clean, set it, then mgx_init", value, S.hold_z_levels);
  }
  if (streq(name, "ksp")) { S.use_ksp = value; if (value) S.ksp_down = 0; return 0; }  // switching it on again also clears a time-out of this solver
  if (streq(name, "rbseq_timeout_ms")) { if (mgxk_set_rbseq_timeout((double)value)) return fail("rbseq_timeout_ms: could not set the device constant"); return 0; }
  if (streq(name, "ksp_timeout_ms")) { if (mgxk_set_ksp_timeout((double)value)) return fail("ksp_timeout_ms: could not set the device constant"); return 0; }
  if (streq(name, "p2p_timeout_ms")) { if (mgxk_set_p2p_timeout((double)value)) return fail("p2p_timeout_ms: could not set the device constant"); return 0; }
  if (streq(name, "p2p")) {  // collective: every rank switches together, between exchanges
    if (value && !S.p2p_ready) return fail("p2p: mgx_p2p_prepare / mgx_p2p_connect have not been called");
    S.p2p_on = value != 0;
    // the ranks decide this together (it is collective), so whatever a rank remembered about its own waits is settled here
    S.p2p_failed = 0;
    if (S.p2p_err) *S.p2p_err = 0;
    return 0;
  }
  const Opt *o = find_option(name);
  if (!o || o->access == RO) return fail("unknown option '%s'", name);
  S.*o->at = value;
  return 0;
}

// read back a namelist member (the reference's drivers `use mg_namelist` and read e.g. `bmask` directly) or an option
int mgx_get_option(const char *name, int *value) {
  if (!value) return fail("mgx_get_option: value is NULL");
  const Opt *o = find_option(name);
  if (!o || o->access == WO) return fail("unknown option '%s'", name);
  *value = o->get ? o->get(S) : S.*o->at;
  return 0;
}
// print_tictoc (mg_tictoc.f90:114-153): name, total and per-level seconds, then the call counts
int mgx_print_tictoc(const char *path) {
  tt_collect();
  FILE *f = fopen(path ? path : "fort.10", "w");
  if (!f) return fail("cannot open %s", path ? path : "fort.10");
  // the reference's formats (mg_tictoc.f90:128-150): t22 + A10, (x,I9) per level; per timer (x,A20), (x,E9.3) total and per level, then
  // the call counts under them -- byte for byte what flang writes (tests/golden/ref_tictoc.txt), E9.3 in Fortran's 0.dddE+ee form
  fprintf(f, "%21s%10s", "", "Total");
  for (int l = 1; l <= S.tt_nblev; l++) fprintf(f, " %9d", l);
  fprintf(f, "\n");
  for (size_t q = 0; q < S.tt_names.size(); q++) {
    double tot = 0; long long nc = 0;
    for (int l = 0; l < S.tt_nblev; l++) { tot += S.tt_time[l][q]; nc += S.tt_calls[l][q]; }
    fprintf(f, " %20s %s", S.tt_names[q].c_str(), fortran_e3(tot, 9).c_str());
    for (int l = 0; l < S.tt_nblev; l++) fprintf(f, " %s", fortran_e3(S.tt_time[l][q], 9).c_str());
    fprintf(f, "\n%21s %9lld", "", nc);
    for (int l = 0; l < S.tt_nblev; l++) fprintf(f, " %9lld", S.tt_calls[l][q]);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

int mgx_tic(int lev, const char *name) {
  if (lev < 1 || lev > 32 || !name) return fail("tic: level %d outside 1..32", lev);
  const int sub = tt_sub(name);
  if (sub >= 32) return fail("tic: more than 32 timer names (mg_tictoc.f90: submax)");
  S.tt_host.push_back(HostTic{lev, sub, std::chrono::steady_clock::now()});
  return 0;
}
int mgx_toc(int lev, const char *name) {
  if (lev < 1 || lev > 32 || !name) return fail("toc: level %d outside 1..32", lev);
  const int sub = tt_sub(name);
  for (int q = (int)S.tt_host.size() - 1; q >= 0; q--)
    if (S.tt_host[q].lev == lev && S.tt_host[q].sub == sub) {
      if (S.inited) (void)hipStreamSynchronize(S.stream);
      S.tt_time[lev - 1][sub] += std::chrono::duration<double>(std::chrono::steady_clock::now() - S.tt_host[q].t0).count();
      S.tt_calls[lev - 1][sub]++;
      if (lev > S.tt_nblev) S.tt_nblev = lev;
      S.tt_host.erase(S.tt_host.begin() + q);
      return 0;
    }
  return fail("toc(%d,'%s') without a matching tic", lev, name);  // the reference prints "Error: tictoc" and goes on (mg_tictoc.f90:104-108)
}

// wait for everything enqueued on the solver's stream and report device-side errors (time-outs, rejected launches); the counterpart of option "async"
int mgx_synchronize(void) { NEED_INIT(); return sync_stream(); }
int mgx_nlevs(void) { return S.inited ? S.nlevs : 0; }
int mgx_level_dims(int lev, int *nx, int *ny, int *nz) { NEED_LEV(lev); const Level &L = S.lev[lev - 1]; *nx = L.nx; *ny = L.ny; *nz = L.nz; return 0; }
int mgx_rbseq_window_info(int lev, double *rho, int *planes) { NEED_LEV(lev); const Level &L = S.lev[lev - 1]; *rho = L.rbs_rho; *planes = L.rbs_m; return 0; }
int mgx_rbseq_window_rows(int lev, int *rows) { NEED_LEV(lev); *rows = S.lev[lev - 1].rbs_rows; return 0; }
int mgx_level_info(int lev, int *out) {
  NEED_LEV(lev);
  const Level &L = S.lev[lev - 1];
  const int v[10] = {L.npx, L.npy, L.incx, L.incy, L.gather, L.ngx, L.ngy, L.key, L.color, S.periodic};   // [9]: option "periodic" (a periodic side's neighbour is the rank itself)
  memcpy(out, v, sizeof(v)); memcpy(out + 10, L.neighb, 8 * sizeof(int));
  return 0;
}

static int field_ptr(Level &L, int field, double **a, size_t *n) {
  const size_t n2 = (size_t)(L.ny + 2) * (L.nx + 2);
  switch (field) {
    case MGX_DX: *a = L.g.dx; *n = n2; return 0;
    case MGX_DY: *a = L.g.dy; *n = n2; return 0;
    case MGX_ZETA: *a = L.g.zeta; *n = n2; return 0;
    case MGX_H: *a = L.g.h; *n = n2; return 0;
    case MGX_ZR: *a = L.g.zr; *n = (size_t)(L.ny + 4) * (L.nx + 4) * L.nz; return 0;
    case MGX_ZW: *a = L.g.zw; *n = (size_t)(L.ny + 4) * (L.nx + 4) * (L.nz + 1); return 0;
    case MGX_CW: *a = L.g.cw; *n = n2 * (L.nz + 1); return 0;
    case MGX_RMASK: *a = L.g.rmask; *n = n2; return 0;
  }
  return 1;
}

int mgx_get_field(int lev, int field, double *host) {
  NEED_LEV(lev);
  Level &L = S.lev[lev - 1];
  const size_t n3 = (size_t)L.nz * (L.ny + 2) * (L.nx + 2);
  double *a; size_t n;
  if (field == MGX_P || field == MGX_B || field == MGX_R) {
    double *js = field == MGX_P ? L.v.p : (field == MGX_B ? L.v.b : L.v.r);
    if (field == MGX_R && L.r_halo_stale) { CHK(fill_halo_js(L, L.v.r, true)); L.r_halo_stale = false; }
    if (field == MGX_B && L.b_halo_stale) { CHK(fill_halo_js(L, L.v.b, true)); L.b_halo_stale = false; }
    mgxk_convert(S.stream, &L.v, js, S.ref_scratch, 1, 0, 1);
    HIPCHK(hipMemcpyAsync(host, S.ref_scratch, n3 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else if (field == MGX_CA) {
    for (int s = 0; s < 8; s++) mgxk_convert(S.stream, &L.v, L.v.cA[s], S.ref_scratch, 8, s, 1);
    HIPCHK(hipMemcpyAsync(host, S.ref_scratch, 8 * n3 * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else if (!field_ptr(L, field, &a, &n)) {
    HIPCHK(hipMemcpyAsync(host, a, n * sizeof(double), hipMemcpyDeviceToHost, S.stream));
  } else return fail("get_field: unknown field id %d", field);
  CHK(sync_stream());
  return 0;
}

int mgx_set_field(int lev, int field, const double *host) {
  NEED_LEV(lev);
  Level &L = S.lev[lev - 1];
  const size_t n3 = (size_t)L.nz * (L.ny + 2) * (L.nx + 2);
  double *a; size_t n;
  if (field == MGX_P || field == MGX_B || field == MGX_R) {
    double *js = field == MGX_P ? L.v.p : (field == MGX_B ? L.v.b : L.v.r);
    HIPCHK(hipMemcpyAsync(S.ref_scratch, host, n3 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    mgxk_convert(S.stream, &L.v, js, S.ref_scratch, 1, 0, 0);
  } else if (field == MGX_CA) {
    HIPCHK(hipMemcpyAsync(S.ref_scratch, host, 8 * n3 * sizeof(double), hipMemcpyHostToDevice, S.stream));
    for (int s = 0; s < 8; s++) mgxk_convert(S.stream, &L.v, L.v.cA[s], S.ref_scratch, 8, s, 0);
    mgxs_pivots(S.stream, &L.v);
    if (L.v.gk) mgxk_rbseq_setup(S.stream, &L.v);
    if (L.v.gk && S.rho_dev && lev <= 32) {
      HIPCHK(hipMemsetAsync(S.rho_dev + lev - 1, 0, sizeof(double), S.stream));
      mgxk_rbseq_rho(S.stream, &L.v, S.rho_dev + lev - 1);
      if (L.gdec) {
        HIPCHK(hipMemsetAsync(L.gdec, 0, (size_t)L.nz * sizeof(double), S.stream));
        mgxk_rbseq_gdecay(S.stream, &L.v, L.gdec);
        HIPCHK(hipMemcpyAsync(L.gdec_h.data(), L.gdec, (size_t)L.nz * sizeof(double), hipMemcpyDeviceToHost, S.stream));
      }
      HIPCHK(hipMemcpyAsync(S.rho_host, S.rho_dev, sizeof S.rho_host, hipMemcpyDeviceToHost, S.stream));
      CHK(sync_stream());
      set_window_planes();
    }
    L.v.zy = L.v.zx = nullptr;  // a user-supplied matrix is used as stored
    L.v.m4 = nullptr;
    S.cd_valid = 0;
    S.coef_gen++;
    S.have_matrix = true;
  } else if (!field_ptr(L, field, &a, &n)) {
    HIPCHK(hipMemcpyAsync(a, host, n * sizeof(double), hipMemcpyHostToDevice, S.stream));
  } else return fail("set_field: unknown field id %d", field);
  CHK(sync_stream());
  return 0;
}

static int time_op(int lev, int reps, float *ms, int which) {
  NEED_LEV(lev);
  if (reps < 1) return fail("reps must be >= 1");
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, S.stream));
  for (int q = 0; q < reps; q++) { if (which == 0) CHK(relax(lev, 1)); else CHK(residual(lev, nullptr)); }
  HIPCHK(hipEventRecord(e1, S.stream));
  HIPCHK(hipEventSynchronize(e1));
  float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *ms = t / reps;
  return 0;
}
// a[i] / b[i] by the hardware division sequence against the refined-reciprocal quotient the colour pass uses for its per-column
// divisors (DIVC, mgx_device.h): *nbad = number of pairs whose bits differ.  Needs no mgx_init.
int mgx_selftest_divc(const double *a, const double *b, int n, long long *nbad) {
  if (n < 1) return fail("mgx_selftest_divc: n must be >= 1");
  double *da = nullptr, *db = nullptr; unsigned long long *dbad = nullptr, h = 0;
  HIPCHK(hipMalloc((void **)&da, (size_t)n * sizeof(double))); HIPCHK(hipMalloc((void **)&db, (size_t)n * sizeof(double))); HIPCHK(hipMalloc((void **)&dbad, sizeof h));
  HIPCHK(hipMemcpy(da, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(db, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dbad, 0, sizeof h));
  mgxk_divc_selftest(nullptr, da, db, n, dbad);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&h, dbad, sizeof h, hipMemcpyDeviceToHost));
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dbad);
  *nbad = (long long)h;
  return 0;
}
int mgx_time_relax(int lev, int reps, float *ms) { return time_op(lev, reps, ms, 0); }
int mgx_time_residual(int lev, int reps, float *ms) { return time_op(lev, reps, ms, 1); }
// test hook of the fp32 cycle: one fp32 operator on the shadow of level lev, inputs converted from the level's fp64 fields, results
// converted back into them -- so each fp32 kernel can be checked against the fp64 operator of the same name on the same input
int mgx_mixed_op(const char *op, int lev, int n) {
  NEED_LEV(lev);
  if (!S.have_matrix) return fail("mgx_mixed_op: no matrix: call mgx_matrices first");
  if (!op) return fail("mgx_mixed_op: op is NULL");
  CHK(mixed_check());
  CHK(mixed_prepare());
  Level &L = S.lev[lev - 1];
  const bool two = streq(op, "fine2coarse") || streq(op, "coarse2fine") || streq(op, "resrest");
  if (two && lev >= S.nlevs) return fail("mgx_mixed_op(%s, %d): no coarser level", op, lev);
  if (streq(op, "relax")) {
    if (n < 0) return fail("mgx_mixed_op(relax): n = %d sweeps", n);
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0); mgxx_to32(S.stream, &L.v, &L.v32, L.v.b, L.v32.f, 1.0);
    CHK(relax32(lev, n));
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.e, L.v.p, 1.0, 0);
  } else if (streq(op, "vcycle")) {   // Vcycle(lev) on the shadow from grid(lev)%p, %b; grid(lev..nlevs)%p = the e it leaves on every level
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0); mgxx_to32(S.stream, &L.v, &L.v32, L.v.b, L.v32.f, 1.0);
    CHK(vcycle32(lev, false));
    for (int q = lev; q <= S.nlevs; q++) { Level &Q = S.lev[q - 1]; mgxx_to64(S.stream, &Q.v, &Q.v32, Q.v32.e, Q.v.p, 1.0, 0); }
  } else if (streq(op, "coarsest")) {   // the coarsest solve of a cycle: b of the coarsest level -> p, from e = 0 (the product under option "mixed_direct", else the sweeps)
    if (lev != S.nlevs) return fail("mgx_mixed_op(coarsest, %d): the coarsest level is %d", lev, S.nlevs);
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.b, L.v32.f, 1.0);
    HIPCHK(hipMemsetAsync(L.v32.e, 0, L.n3js32 * sizeof(float), S.stream));
    CHK(coarsest_solve32(true));
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.e, L.v.p, 1.0, 0);
  } else if (streq(op, "residual")) {
    mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0); mgxx_to32(S.stream, &L.v, &L.v32, L.v.b, L.v32.f, 1.0);
    mgxx_residual(S.stream, &L.v32, S.real);
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.r, L.v.r, 1.0, 0);
    L.r_halo_stale = false;   // the kernel stored the physical images, and a single rank has no others
  } else if (streq(op, "fine2coarse") || streq(op, "resrest")) {
    Level &C = S.lev[lev];
    if (streq(op, "fine2coarse")) {   // grid(lev+1)%b = restriction of grid(lev)%r, grid(lev+1)%p = 0
      mgxx_to32(S.stream, &L.v, &L.v32, L.v.r, L.v32.r, 1.0);
      mgxx_restrict(S.stream, &L.v32, &C.v32, L.v32.r);
    } else {                          // the down leg of a V-cycle: restriction of b - A p of level lev
      mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0); mgxx_to32(S.stream, &L.v, &L.v32, L.v.b, L.v32.f, 1.0);
      mgxx_resrest(S.stream, &L.v32, &C.v32, S.real);
    }
    mgxx_to64(S.stream, &C.v, &C.v32, C.v32.f, C.v.b, 1.0, 0);
    mgxx_to64(S.stream, &C.v, &C.v32, C.v32.e, C.v.p, 1.0, 0);
    C.b_halo_stale = false;
  } else if (streq(op, "coarse2fine")) {   // grid(lev)%p += interpolation of grid(lev+1)%p
    Level &C = S.lev[lev];
    mgxx_to32(S.stream, &C.v, &C.v32, C.v.p, C.v32.e, 1.0); mgxx_to32(S.stream, &L.v, &L.v32, L.v.p, L.v32.e, 1.0);
    coarse2fine32(lev);
    mgxx_to64(S.stream, &L.v, &L.v32, L.v32.e, L.v.p, 1.0, 0);
  } else return fail("mgx_mixed_op: unknown operator '%s' (relax, vcycle, coarsest, residual, fine2coarse, coarse2fine, resrest)", op);
  return sync_stream();
}

// test hook of the three passes of option "krylov": one pass on level 1 through the wrapper and on the buffers solve_p_krylov uses (mgx_cycle.cpp: krylov_op)
int mgx_krylov_op(const char *op, int nd, double *const *fields, const int *slot, const double *sin, double *sout, int *path) {
  NEED_INIT();
  if (S.nranks > 1) return fail("mgx_krylov_op needs a single rank (process grid %d x %d)", S.npx, S.npy);
  if (!S.have_matrix) return fail("mgx_krylov_op: no matrix: call mgx_matrices first");
  return krylov_op(op, nd, fields, slot, sin, sout, path);
}

int mgx_counters(long long *out) { out[0] = S.n_launch; out[1] = S.n_halo; out[2] = S.n_exch; out[3] = S.n_allred; return 0; }

}  // extern "C"

#ifdef MGX_RBSEQ_TRACE
extern "C" int mgx_debug_rbs(int lev, unsigned long long *out8) {
  auto &L = S.lev[lev - 1];
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(out8, L.rbs_flag + (L.nx / 8 + 2) * 16, 64, hipMemcpyDeviceToHost);
  (void)hipMemset(L.rbs_flag + (L.nx / 8 + 2) * 16, 0, 64);
  return 0;
}
#endif
