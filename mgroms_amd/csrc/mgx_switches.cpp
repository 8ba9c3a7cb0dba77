// The A/B switches: ONE table.  Per switch: the environment variable, its member of Switches, how the variable is read, the value
// without it, and what the alternative is -- with "same bits" where the alternative computes what the default computes, bit for bit.
// mgx_switches() walks the table once per process, on first use.  A variable that is present but empty counts as present.
//
// Not here, and read where they are used:
//   MGX_NO_SMALL, MGX_NO_MF, MGX_P2P_TIMEOUT_MS  mgx_init (mgx_define.cpp) reads them at every mgx_init, not once per process: one process can
//                                                initialise with and without them (the tests do)
//   MGX_P2P_TEST_FAIL_CONNECT                    mgx_p2p_connect (mgx_comm.cpp): a test hook that names one rank, read at every connect
// and the variables that preset a run-time option at mgx_init (OPTIONS[] in mgx_api.cpp: mgx_set_option overrides them).
#include "mgx_switches.h"
#include <cstdlib>

namespace {

enum Rule { SET_TRUE, SET_FALSE, ATOI, ATOLL };   // the variable's presence means true, means false, or its value is parsed
struct Row {
  const char *env; bool Switches::*flag; int Switches::*num; long long Switches::*wide; Rule rule; long long dflt; const char *what;
  Row(const char *e, bool Switches::*m, Rule r, long long d, const char *w) : env(e), flag(m), num(nullptr), wide(nullptr), rule(r), dflt(d), what(w) {}
  Row(const char *e, int Switches::*m, Rule r, long long d, const char *w) : env(e), flag(nullptr), num(m), wide(nullptr), rule(r), dflt(d), what(w) {}
  Row(const char *e, long long Switches::*m, Rule r, long long d, const char *w) : env(e), flag(nullptr), num(nullptr), wide(m), rule(r), dflt(d), what(w) {}
};
const Row TABLE[] = {
  // variable                    member                            rule       default           the alternative
  {"MGX_NO_XCD",                 &Switches::no_xcd,                SET_TRUE,  0,                "plain block order instead of the per-XCD block map of the colour passes (relax, tall, k-split); same bits"},
  {"MGX_NO_REG",                 &Switches::no_reg,                SET_TRUE,  0,                "small closed levels without the one-thread-per-column kernel (k_relax_reg): the LDS-resident or the generic one; same bits"},
  {"MGX_NO_TINY",                &Switches::no_tiny,               SET_TRUE,  0,                "small closed levels without the all-in-LDS kernel (k_relax_tiny); same bits"},
  {"MGX_NO_WAVE",                &Switches::no_wave,               SET_TRUE,  0,                "the two coarsest levels without the wave kernels (k_relax_wave, four and eight waves included): the older one-workgroup kernels; same bits, except red-black with cmatrix = 'real' in the sequential order at speed: the plane loop's bits instead of the walk's, both within 1e-12 of the reference's loop"},
  {"MGX_NO_WAVE_FUSE",           &Switches::no_wave_fuse,          SET_TRUE,  0,                "coarse2fine / residual + fine2coarse as launches of their own around the coarse relax instead of folded into it; same bits"},
  {"MGX_NO_TALL",                &Switches::no_tall,               SET_TRUE,  0,                "generic colour pass at nz = 80, 96, 128 instead of the tall-column pass (and no chained snapshots there); same bits"},
  {"MGX_NO_KS",                  &Switches::no_ks,                 SET_TRUE,  0,                "row-by-row colour passes on the mid levels instead of every k-split kernel (pass, colour pair, persistent relax); same bits"},
  {"MGX_NO_KS8",                 &Switches::ks8,                   SET_FALSE, 1,                "nz = 8 levels: row-by-row instead of the k-split colour pass; same bits"},
  {"MGX_NO_KS64",                &Switches::ks64,                  SET_FALSE, 1,                "nz = 64 levels that fit the caches: row-by-row instead of the k-split colour pass; same bits"},
  {"MGX_NO_KS2",                 &Switches::no_ks2,                SET_TRUE,  0,                "four colours on the closed mid levels: one launch per colour instead of per colour pair (and no persistent relax); same bits"},
  {"MGX_NO_KSP",                 &Switches::no_ksp,                SET_TRUE,  0,                "one launch per colour pair instead of the persistent relax; also presets option \"ksp\", which cannot turn it back on; same bits"},
  {"MGX_KSP_SC1",                &Switches::ksp_fence,             SET_FALSE, 1,                "the persistent relax hands planes over with sc1 accesses instead of release / acquire fences (measured on gfx950 only); same bits"},
  {"MGX_KS_NW",                  &Switches::ks_nw,                 ATOI,      0,                "= 4: four waves per workgroup instead of eight in the k-split colour pass; same bits"},
  {"MGX_RBSEQ_D0_KERNEL",        &Switches::rbseq_d0_kernel,       SET_TRUE,  0,                "sequential-order red-black: the walk reads d0 on every level, written by the colour pass or by k_rbseq_d0, instead of forming it on narrow half-rows; same bits"},
  {"MGX_RBSEQ_NO_D0_MID",        &Switches::rbseq_d0_mid,          SET_FALSE, 1,                "half-rows of 65..128 columns: the walk forms d0 itself instead of reading what the colour pass left; same bits"},
  {"MGX_NO_RBSEQ_WALK_APPLY",    &Switches::no_rbseq_walk_apply,   SET_TRUE,  0,                "small levels: walk and correction by the scan kernels instead of k_rbseq_walk_apply; same bits"},
  {"MGX_RBSEQ_WINDOW_NO_XMAP",   &Switches::rbseq_window_no_xmap,  SET_TRUE,  0,                "plain block order instead of the per-XCD block map of the windowed walk; same bits"},
  {"MGX_RBW_PRIO",               &Switches::rbw_prio,              ATOI,      1,                "= 0: the walking wave of the windowed walk at normal priority instead of s_setprio 3; same bits"},
  {"MGX_C2F_KC",                 &Switches::c2f_kc,                ATOI,      0,                "> 0: that many coarse levels per lane in the prolongation instead of 16 (before the cut for small levels); same bits"},
  {"MGX_C2F_NT",                 &Switches::c2f_nt,                ATOI,      -1,               ">= 0: the prolongation's streaming hints forced on (1) or off (0) instead of chosen by the level's size; same bits"},
  {"MGX_NO_RESREST",             &Switches::no_resrest,            SET_TRUE,  0,                "residual and restriction as two kernels instead of the fused one; same bits"},
  {"MGX_RESREST_MIN",            &Switches::resrest_min,           ATOLL,     0,                "the fused residual + restriction only from that many fine cells on, two kernels below; same bits"},
  {"MGX_RESREST_FLAT_MAX",       &Switches::resrest_flat_max,      ATOLL,     256LL * 256 * 64, "fine cells up to which the fused residual + restriction takes its flat form (no walk up the column); same bits"},
  {"MGX_RESREST_FLAT_S",         &Switches::resrest_flat_s,        ATOI,      0,                ">= 4: four fine rows per wave in the flat form instead of two; same bits"},
  {"MGX_RESREST_AHEAD",          &Switches::resrest_ahead,         ATOI,      11,               "10 * AW + AR, the look-ahead of the walking form: 12 and 21 are instantiated beside 11; same bits"},
  {"MGX_RESREST_NO_ZW",          &Switches::resrest_no_zw,         SET_TRUE,  0,                "the walking form of a cycle's down leg streams slots 4 and 7 instead of generating their interior rows from the depth formula (look-ahead 11, no norm: the others always stream); same bits"},
  {"MGX_P2P_MAXBLK",             &Switches::p2p_maxblk,            ATOI,      128,              "block cap of the halo push kernel (its grid must stay resident beside a neighbour's smoother); same bits"},
  {"MGX_P2P_IPT",                &Switches::p2p_ipt,               ATOI,      1,                "test hook: at least that many items per thread in the halo push kernel; same bits"},
  {"MGX_MODEL_KR",               &Switches::model_kr,              ATOI,      0,                "> 0 (A/B and test hook): runs of exactly that many rows in the flux kernels and correct_uvw; same bits"},
};

}  // namespace

const Switches &mgx_switches() {
  static const Switches sw = [] {
    Switches s = {};
    for (const Row &r : TABLE) {
      const char *e = getenv(r.env);
      if (r.flag) s.*r.flag = e ? r.rule == SET_TRUE : r.dflt != 0;
      else if (r.num) s.*r.num = e ? atoi(e) : (int)r.dflt;
      else s.*r.wide = e ? atoll(e) : r.dflt;
    }
    return s;
  }();
  return sw;
}
