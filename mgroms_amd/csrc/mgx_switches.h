// The A/B switches of libmgx.so: environment variables that make a kernel wrapper take its measured alternative.  They are read once per
// process, on first use, by the one table of mgx_switches.cpp; every wrapper reads mgx_switches().x.  Unlike the run-time options of
// mgx_api.cpp (OPTIONS[]) they cannot be changed after the first launch, which is why a test of one of them runs in a process of its own.
#pragma once

struct Switches {
  // block order of the colour passes
  bool no_xcd;
  // one-workgroup kernels of the small levels (mgx_relax.hip, mgx_relax_coarse.hip)
  bool no_reg, no_tiny, no_wave, no_wave_fuse;
  // tall columns (mgx_relax_tall.hip)
  bool no_tall;
  // k-split colour passes of the mid levels (mgx_relax_ks.hip)
  bool no_ks, ks8, ks64, no_ks2, no_ksp, ksp_fence;
  int ks_nw;
  // sequential-order red-black (mgx_rbseq.hip)
  bool rbseq_d0_kernel, rbseq_d0_mid, no_rbseq_walk_apply, rbseq_window_no_xmap;
  int rbw_prio;
  // transfer kernels (mgx_transfer.hip, mgx_resrest.hip)
  int c2f_kc, c2f_nt;
  bool no_resrest, resrest_no_zw;
  long long resrest_min, resrest_flat_max;
  int resrest_flat_s, resrest_ahead;
  // halo pushes (mgx_halo.hip) and the model coupling (mgx_model.hip)
  int p2p_maxblk, p2p_ipt, model_kr;
};

const Switches &mgx_switches();
