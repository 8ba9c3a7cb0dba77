"""The case table of tests/test_gpu_switches.py: for every A/B switch of mgx_switches.cpp (and MGX_NO_SMALL, which mgx_init reads) the
environment of the arm that takes the alternative, the probes it runs, where the arm may differ from the default arm in the last bits,
and the evidence that the alternative ran.  Importable without a GPU and without torch: tests/test_switch_coverage_host.py keeps this
table, the table of mgx_switches.cpp and the rest of the suite together.

A probe is small and fully seeded (tests/_gpu_switch_worker.py runs it, with the CPU oracle beside it):
  relax   on every level random p and b, fill_halo, relax(lev, 3): per level p, the launches of the call, the error against the oracle
  cycle   compute_rhs from random u, v, w, two Vcycle(1) with the launches of each, every level's p and b, solve_p(1e-30, 2)
The probes of a case are one of the lists of PROBE_SETS, so that the cases of a list share one default arm.

Evidence, exactly one kind per case:
  launches  [(probe, "lev<n>" or "vcycle", launches of the default arm or None, launches of the variant arm or None, difference or None)]
            with the derivation from mgx_cycle.cpp beside it
  kernel    regular expressions (blanks removed from the kernel names first) that match a kernel of the variant arm's rocprofv3 kernel
            trace and none of the default arm's ("present"), and the reverse ("absent")
  shape     [(probe, level, predicate(nx, ny, nz, method))]: the switch changes a run-time argument or the grid only, and the predicate
            is the precondition, read from the gating line quoted beside it, under which the two arms launch something different"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT_VARIABLES = ("MGX_NO_SMALL", "MGX_NO_MF", "MGX_P2P_TIMEOUT_MS")   # read by mgx_init (mgx_define.cpp), not by the table
EVIDENCE_KINDS = ("launches", "kernel", "shape")


def table_variables():
    """the variables of TABLE in mgx_switches.cpp, in its order"""
    text = open(os.path.join(ROOT, "mgroms_amd", "csrc", "mgx_switches.cpp")).read()
    return re.findall(r'^\s*\{"(MGX_\w+)",\s*&Switches::\w+,', text, re.M)


def relax(dims, method, cmatrix, **options):
    return {"kind": "relax", "dims": tuple(dims), "method": method, "cmatrix": cmatrix, "options": dict(options)}


def cycle(dims, method, cmatrix):
    return {"kind": "cycle", "dims": tuple(dims), "method": method, "cmatrix": cmatrix, "options": {}}


def probe_id(p):
    opts = "".join(f":{k}={v}" for k, v in sorted(p["options"].items()))
    return f"{p['kind']}:{'x'.join(str(d) for d in p['dims'])}:{p['method']}:{p['cmatrix']}{opts}"


def probe_mode(p):
    """'exact': the fields equal the oracle's bit for bit (four colours; red-black without the k = 1 diagonals; red-black in the
    reference's order plane by plane, option rb_exact).  'rb_seq': red-black with cmatrix = 'real' in the sequential order at speed,
    the tolerances of the header of tests/test_gpu_parity.py."""
    if p["method"] == "FC" or p["cmatrix"] == "simple" or p["options"].get("rb_exact"):
        return "exact"
    return "rb_seq"


MODES = [("FC", "real", {}), ("FC", "simple", {}), ("RB", "simple", {}), ("RB", "real", {}), ("RB", "real", {"rb_exact": 1})]
WINDOW_ROUTES = [{"rbseq_window": 1}, {"rbseq_window": 0, "rbseq_fuse": 1}, {"rbseq_window": 0, "rbseq_fuse": 0}]

PROBE_SETS = {
    # levels (nsmall = 8, one rank): 16x16x8 > 8x8x4 > 4x4x2;  32x32x8 > 16x16x4 > 8x8x2;  64x64x8 > 32x32x4 > 16x16x2;
    # 128x128x8 > 64x64x4 > 32x32x2 (k_relax_reg<2, ., 1024> with all its 1024 threads);  256x128x8 > 128x64x4 > 64x32x2
    "ladder": [relax(d, m, c, **o) for d in ((16, 16, 8), (32, 32, 8), (64, 64, 8), (128, 128, 8), (256, 128, 8)) for m, c, o in MODES],
    # 32x32x8: level 1 has nz = 8 and 256 columns per colour;  32x32x64 > 16x16x32 > 8x8x16 > 4x4x8
    "ks": [relax(d, m, c) for d in ((32, 32, 8), (32, 32, 64)) for m, c in (("FC", "real"), ("FC", "simple"), ("RB", "real"))]
          + [cycle((32, 32, 8), "FC", "real")],
    # 32x160x16: ragged half-rows of 80 columns in two j-chunks;  16x160x80: the tall pass
    "xcd": [relax(d, m, "real") for d in ((32, 160, 16), (16, 160, 80)) for m in ("FC", "RB")],
    # half-rows of 128 columns (16x256x8), ragged ones of 80 (16x160x16), of 16 (32x32x8), each by the window, by walk + correction in
    # one launch where an instance exists, and by the walk and the correction as launches of their own
    "rbseq": [relax(d, "RB", "real", **o) for d in ((16, 256, 8), (16, 160, 16), (32, 32, 8)) for o in WINDOW_ROUTES],
    # 32x32x8 > 16x16x4 > 8x8x2;  64x96x32 > 32x48x16 > 16x24x8 > 8x12x4 > 4x6x2
    "transfer": [cycle(d, m, c) for d in ((32, 32, 8), (64, 96, 32)) for m, c in (("FC", "real"), ("RB", "simple"), ("RB", "real"))],
}
# the level shapes the cases below rely on, asserted by the test through mg.grid(lev) of both arms
LEVELS = {
    (16, 16, 8): [(16, 16, 8), (8, 8, 4), (4, 4, 2)],
    (32, 32, 8): [(32, 32, 8), (16, 16, 4), (8, 8, 2)],
    (64, 64, 8): [(64, 64, 8), (32, 32, 4), (16, 16, 2)],
    (128, 128, 8): [(128, 128, 8), (64, 64, 4), (32, 32, 2)],
    (256, 128, 8): [(256, 128, 8), (128, 64, 4), (64, 32, 2)],
    (32, 32, 64): [(32, 32, 64), (16, 16, 32), (8, 8, 16), (4, 4, 8)],
    (32, 160, 16): [(32, 160, 16), (16, 80, 8), (8, 40, 4), (4, 20, 2)],
    (16, 160, 80): [(16, 160, 80), (8, 80, 40), (4, 40, 20)],
    (16, 256, 8): [(16, 256, 8), (8, 128, 4), (4, 64, 2)],
    (16, 160, 16): [(16, 160, 16), (8, 80, 8), (4, 40, 4)],
    (64, 96, 32): [(64, 96, 32), (32, 48, 16), (16, 24, 8), (8, 12, 4), (4, 6, 2)],
}

B = r"(?:true|false)"       # a bool template argument, either value
WALK = ("k_relax_wave runs the sequential order by its walk (within 1e-12 of the reference's loop), the kernels behind it run the "
        "plane loop itself (its bits): the two arms differ in the last bits on the levels the wave kernel serves")


def _ids(name, **like):
    return [probe_id(p) for p in PROBE_SETS[name] if all(p[k] == v for k, v in like.items())]


def _case(env, probes, evidence, not_same_bits=None, one_launch=()):
    """not_same_bits: {probe id: (levels, one-line reason)} -- p of each of these levels must DIFFER from the default arm's (an exemption
    that is not needed has to go); every other level of the probe, and every other probe of the case, must equal it bit for bit.
    one_launch: [(probe id, level)] whose relax call must be ONE launch in both arms (the persistent relax ran to its end)."""
    return {"env": dict(env), "probes": probes, "evidence": evidence, "not_same_bits": dict(not_same_bits or {}), "one_launch": list(one_launch)}


def _rb_seq_ids(name):
    return [probe_id(p) for p in PROBE_SETS[name] if probe_mode(p) == "rb_seq"]


def _wave_walk_levels(dims):
    """the levels of a hierarchy that k_relax_wave serves in the sequential order by its walk.  relax_wave_launch (mgx_relax_coarse.hip):
    "(L->nz != 2 && L->nz != 4 && !nz3)" declines, "if (seq && L->ny / 2 > WAVE) return 0;", "nblk > (L->nz == 2 ? 8 : 4) * WAVE" declines
    with nblk = (nx / 2) * (ny / 2), and the walk's LDS, (2 nz + 5) nx ny + 4 + 64 * 18 doubles, must fit 160 KB"""
    return tuple(lev for lev, (nx, ny, nz) in enumerate(LEVELS[dims], 1)
                 if nz in (2, 4) and ny // 2 <= 64 and (nx // 2) * (ny // 2) <= (8 if nz == 2 else 4) * 64
                 and ((2 * nz + 5) * nx * ny + 4 + 64 * 18) * 8 <= 160 * 1024)


def _no_wave_exempt():
    return {probe_id(p): (_wave_walk_levels(p["dims"]), WALK) for p in PROBE_SETS["ladder"] if probe_mode(p) == "rb_seq"}


# MGX_NO_SMALL: the levels on which the colour pass with the walk of mgx_rbseq.hip came out with other last bits than the one-workgroup
# kernel of the default arm (k_relax_small's plane loop at 16x16x8, the walk of k_relax_wave on the others).  Measured, not derived: on
# the smaller levels (8x8x4, 4x4x2, 16x16x4, 8x8x2, 16x16x2) the two walks give the same bits, and those levels keep the duty.
NO_SMALL_LEVELS = {(16, 16, 8): (1,), (64, 64, 8): (2,), (128, 128, 8): (3,), (256, 128, 8): (3,)}
NO_SMALL_WHY = ("without the one-workgroup kernels a small level takes the colour pass and the walk of mgx_rbseq.hip, the default arm the walk "
                "of k_relax_wave or the plane loop of k_relax_small: each within 1e-12 of the reference's loop, not the same bits")


def _nplanes(nx, method):
    return nx // 2 if method == "FC" else nx


def _xcd_differs(nx, ny, nz, method):
    # XCD_BLOCK_MAP (mgx_relax_common.h): "if (gx < 0) { plain } else if ((nunit & 7) == 0) { per-XCD } else { plain }" over a grid of
    # gx * nunit blocks, gx = ceil(ny / 2 / 64) j-chunks and nunit = the planes of the colour (one plane per workgroup below 2048
    # workgroups): the two maps differ once there are more than 8 blocks
    gx, n = (ny // 2 + 63) // 64, _nplanes(nx, method)
    return nz in (8, 16, 32, 64, 80, 96, 128) and n % 8 == 0 and gx * n > 8 and gx * n < 2048


def _xmap_differs(nx, ny, nz, method):
    # mgxk_rbseq_window: "const int xmap = !mgx_switches().rbseq_window_no_xmap && L->nx % 8 == 0 && (long long)nch * L->nx * nkz < (1LL << 31);"
    return nx % 8 == 0 and nz % 4 == 0


def _always(nx, ny, nz, method):
    # mgxk_rbseq_window: "const int prio = mgx_switches().rbw_prio;" is handed to every launch of the window (the test also asserts
    # that the window served the level: 6 window colours in 3 sweeps)
    return nz % 4 == 0


def _nt_differs(nx, ny, nz, method):
    # mgxk_coarse2fine: "const int nt = mgx_switches().c2f_nt >= 0 ? mgx_switches().c2f_nt : level_streams(F);" with
    # level_streams = nx * ny * nz * 72.0 > 256e6 (mgx_device.h): a forced 1 differs wherever the level is smaller than that
    return not nx * ny * nz * 72.0 > 256e6


FC8, FS8, RB8 = (probe_id(relax((32, 32, 8), m, c)) for m, c in (("FC", "real"), ("FC", "simple"), ("RB", "real")))
FC64 = probe_id(relax((32, 32, 64), "FC", "real"))
CY_FC_S, CY_FC_L = probe_id(cycle((32, 32, 8), "FC", "real")), probe_id(cycle((64, 96, 32), "FC", "real"))
W0F1_32 = probe_id(relax((32, 32, 8), "RB", "real", rbseq_window=0, rbseq_fuse=1))
KSP_ONE = [(FC8, 1), (FS8, 1), (FC64, 3)]

CASES = {
    # ---- the small-level ladder: mgxk_relax_small (mgx_relax.hip) and relax_wave_launch (mgx_relax_coarse.hip) ----
    "no_wave": _case(
        {"MGX_NO_WAVE": "1"}, "ladder",
        # 16x16x4 and 8x8x4 go to k_relax_reg<4, ., 256>, the nz = 2 levels of up to 1024 columns to k_relax_reg<2, ., 1024>, 64x32x2 to
        # k_relax_small<2, ., 1024> (the default arm has the REAL = true instances of these from its rb_exact probes, which the wave declines)
        {"kind": "kernel", "present": [r"k_relax_reg<4,false,256>", r"k_relax_reg<2,false,1024>", r"k_relax_small<2,false,1024>"],
         "absent": [r"k_relax_wave<"]},
        not_same_bits=_no_wave_exempt()),
    "no_wave_no_reg": _case(
        {"MGX_NO_WAVE": "1", "MGX_NO_REG": "1"}, "ladder",
        # k_relax_tiny where 11 arrays of the level fit 64 KB of LDS (8x8x4; 4x4x2, 8x8x2, 16x16x2), k_relax_small<4> at 16x16x4 and 32x32x4
        {"kind": "kernel", "present": [r"k_relax_tiny<2,", r"k_relax_tiny<4,", r"k_relax_small<4,false,256>"],
         "absent": [r"k_relax_wave<", r"k_relax_reg<"]},
        not_same_bits=_no_wave_exempt()),
    "no_wave_no_reg_no_tiny": _case(
        {"MGX_NO_WAVE": "1", "MGX_NO_REG": "1", "MGX_NO_TINY": "1"}, "ladder",
        {"kind": "kernel", "present": [r"k_relax_small<2,false,256>", r"k_relax_small<2,true,256>", r"k_relax_small<4,false,256>"],
         "absent": [r"k_relax_wave<", r"k_relax_reg<"]},
        not_same_bits=_no_wave_exempt()),
    "no_reg_rb_exact": _case(
        {"MGX_NO_REG": "1"}, "ladder",
        # the wave declines mode 1 (rb_exact) and k_relax_tiny has no plane loop: k_relax_small in its exact form
        {"kind": "kernel", "present": [r"k_relax_small<4,true,256>", r"k_relax_small<2,true,256>"], "absent": [r"k_relax_reg<"]}),
    "no_small": _case(
        {"MGX_NO_SMALL": "1"}, "ladder",
        # relax(): "if (S.use_small && nsweeps > 0) {...one launch...}" is skipped.  8x8x2 has no k-split kernel (nz = 2; a closed nz = 4
        # level has the persistent relax with four colours), so relax_fc launches mgxk_relax_colour once per colour, 4 x 3 sweeps;
        # k_relax_nz<2|4> stores the mirrors, so fill_halo_js launches nothing.  relax_rb without the k = 1 diagonals takes no snapshot:
        # 2 x 3 sweeps.
        {"kind": "launches", "checks": [(probe_id(relax((32, 32, 8), "FC", "real")), "lev3", 1, 12, None),
                                        (probe_id(relax((32, 32, 8), "FC", "simple")), "lev3", 1, 12, None),
                                        (probe_id(relax((32, 32, 8), "RB", "simple")), "lev2", 1, 6, None),
                                        (probe_id(relax((32, 32, 8), "RB", "simple")), "lev3", 1, 6, None),
                                        (probe_id(relax((256, 128, 8), "RB", "simple")), "lev3", 1, 6, None)]},
        not_same_bits={probe_id(p): (NO_SMALL_LEVELS[p["dims"]], NO_SMALL_WHY) for p in PROBE_SETS["ladder"]
                       if probe_mode(p) == "rb_seq" and p["dims"] in NO_SMALL_LEVELS}),
    # ---- the k-split mid levels: mgx_relax_ks.hip ----
    "no_ks": _case(
        {"MGX_NO_KS": "1"}, "ks",
        {"kind": "kernel", "present": [r"k_relax_nz<8,", r"k_relax_nz<16,", r"k_relax_nz<32,", rf"k_relax_nz<64,{B},false,"],
         "absent": [r"k_relax_ks<", r"k_relax_ksp<"]}),
    "no_ks8": _case(
        {"MGX_NO_KS8": "1"}, "ks",
        # (the persistent relax of a closed four-colour level does not ask ks8: the red-black probe shows the row-by-row pass)
        {"kind": "kernel", "present": [r"k_relax_nz<8,"], "absent": [r"k_relax_ks<8,"]}),
    "no_ks64": _case(
        {"MGX_NO_KS64": "1"}, "ks",
        # (red-black with the snapshot is row by row at nz = 64 in both arms: "L->nz == 64 && sw.ks64 && !snap")
        {"kind": "kernel", "present": [rf"k_relax_nz<64,{B},false,"], "absent": [r"k_relax_ks<64,"]}),
    "no_ks2": _case(
        {"MGX_NO_KS2": "1"}, "ks",
        # relax(): mgxk_relax_ks_persist and, in relax_fc, mgxk_relax_ks_pair both return 0 under no_ks2: one mgxk_relax_colour per colour,
        # 4 x 3 sweeps (k_relax_ks stores the mirrors: no halo launch)
        {"kind": "launches", "checks": [(FC8, "lev1", 1, 12, None), (FS8, "lev1", 1, 12, None), (FC64, "lev3", 1, 12, None)]}),
    "no_ksp": _case(
        {"MGX_NO_KSP": "1"}, "ks",
        # relax(): mgxk_relax_ks_persist returns 0; relax_fc: "if (closed && mgxk_relax_ks_pair(...)) { S.n_launch++; continue; }" per
        # colour pair, 2 x 3 sweeps
        {"kind": "launches", "checks": [(FC8, "lev1", 1, 6, None), (FS8, "lev1", 1, 6, None), (FC64, "lev3", 1, 6, None)]}),
    "ksp_sc1": _case(
        {"MGX_KSP_SC1": "1"}, "ks",
        {"kind": "kernel", "present": [r"k_relax_ksp<8,8,true,false>", r"k_relax_ksp<8,8,false,false>", r"k_relax_ksp<16,4,true,false>"],
         "absent": [rf"k_relax_ksp<\d+,\d,{B},true>"]},
        one_launch=KSP_ONE),
    "ks_nw4": _case(
        {"MGX_KS_NW": "4"}, "ks",
        {"kind": "kernel", "present": [r"k_relax_ks<8,4,", r"k_relax_ks<16,4,", r"k_relax_ks<32,4,"],
         "absent": [r"k_relax_ks<8,8,", r"k_relax_ks<16,8,", r"k_relax_ks<32,8,"]},
        one_launch=KSP_ONE),
    "no_xcd": _case(
        {"MGX_NO_XCD": "1"}, "xcd",
        {"kind": "shape", "checks": [(i, 1, _xcd_differs) for i in _ids("xcd")]}),
    # ---- sequential-order red-black: mgx_rbseq.hip, rbseq_correct (mgx_cycle.cpp) ----
    "rbseq_d0_kernel": _case(
        {"MGX_RBSEQ_D0_KERNEL": "1"}, "rbseq",
        # half-rows of at most 64 columns, window and fuse off: the walk reads d0 (D0IN = false) where the default forms it (true)
        {"kind": "kernel", "present": [rf"k_rbseq_scan<1,\d+,[01],{B},1,false,0>"], "absent": [rf"k_rbseq_scan<\d+,\d+,[01],{B},\d,true,0>"]}),
    "rbseq_no_d0_mid": _case(
        {"MGX_RBSEQ_NO_D0_MID": "1"}, "rbseq",
        # half-rows of 65..128 columns (128 and 80 here), window off: the walk forms d0 (D0IN = true) where the default reads it (false)
        {"kind": "kernel", "present": [rf"k_rbseq_scan<2,\d+,[01],{B},1,true,0>"], "absent": [rf"k_rbseq_scan<2,\d+,[01],{B},1,false,0>"]}),
    "no_rbseq_walk_apply": _case(
        {"MGX_NO_RBSEQ_WALK_APPLY": "1"}, "rbseq",
        # rbseq_correct with the window off: "if (have_d0 && S.rbseq_fuse && mgxk_rbseq_walk_apply(...)) { S.n_launch++; ...return 0; }" is one
        # launch per colour; without it mgxk_rbseq_scan_apply returns 1 (no fused instance for half-rows of 16 columns): the walk, then
        # "if (ran == 1) { mgxk_rbseq_apply(...); S.n_launch++; }  S.n_launch += 2 - have_d0;" -- two.  Per call: the snapshot, then 6 colours
        # of pass + 1 against pass + 2
        {"kind": "launches", "checks": [(W0F1_32, "lev1", 13, 19, None)]}),
    "rbseq_window_no_xmap": _case(
        {"MGX_RBSEQ_WINDOW_NO_XMAP": "1"}, "rbseq",
        {"kind": "shape", "window": True, "checks": [(i, 1, _xmap_differs) for i in _ids("rbseq") if "rbseq_window=1" in i]}),
    "rbw_prio0": _case(
        {"MGX_RBW_PRIO": "0"}, "rbseq",
        {"kind": "shape", "window": True, "checks": [(i, 1, _always) for i in _ids("rbseq") if "rbseq_window=1" in i]}),
    # ---- transfers ----
    "no_wave_fuse": _case(
        {"MGX_NO_WAVE_FUSE": "1"}, "transfer",
        # vcycle(): on the level below the coarsest one (16x16x4 above 8x8x2, 8x12x4 above 4x6x2) relax_fused(lev, ns_pre, 2) is ONE launch for
        # relax + residual + fine2coarse and relax_fused(lev, ns_post, 1) ONE for coarse2fine + relax; without them relax (1) + the fused
        # residual + restriction (1) and coarse2fine (1, its fill_halo_js finds the images stored) + relax (1): two more per V-cycle
        {"kind": "launches", "checks": [(CY_FC_S, "vcycle", None, None, 2), (CY_FC_L, "vcycle", None, None, 2)]}),
    "c2f_nt1": _case(
        {"MGX_C2F_NT": "1"}, "transfer",
        # (MGX_C2F_NT=0 has no case: at these sizes level_streams picks 0 itself and the two arms would launch the same thing)
        {"kind": "shape", "checks": [(i, 1, _nt_differs) for i in _ids("transfer")]}),
    "resrest_min_above": _case(
        {"MGX_RESREST_MIN": "10000000"}, "transfer",
        # fine2coarse(): "if (mgxk_residual_restrict(...)) { S.n_launch++; return 1; }  return residual(lev, nullptr) ? -1 : 0;" and then
        # restrict(): one launch becomes two on every down leg that is not folded into the coarse relax -- level 1 of 32x32x8, levels 1-3 of 64x96x32
        {"kind": "launches", "checks": [(CY_FC_S, "vcycle", None, None, 1), (CY_FC_L, "vcycle", None, None, 3)]}),
    "resrest_min_between": _case(
        {"MGX_RESREST_MIN": "8192"}, "transfer",
        # "if ((long long)F->nx * F->ny * F->nz < sw.resrest_min) return 0;": 32x32x8 = 8192 cells keeps the fused kernel (its level 2 is folded
        # into the coarse relax); of 64x96x32 levels 1 and 2 (196608, 24576 cells) keep it and level 3 (3072) takes the two kernels
        {"kind": "launches", "checks": [(CY_FC_S, "vcycle", None, None, 0), (CY_FC_L, "vcycle", None, None, 1)]}),
}

# switches that another file of the suite pins: variable -> "tests/file.py::test"
# (MGX_P2P_TIMEOUT_MS is no A/B switch and has no alternative to show: the test named for it sets the bound the library has anyway, so
# only the read in mgx_init and the store of the device constant are exercised.  What a shorter bound does is the subject of
# test_p2p_timeout_is_agreed_collectively, which sets it through option "p2p_timeout_ms", the same mgxk_set_p2p_timeout.)
COVERED_ELSEWHERE = {
    "MGX_NO_TALL": "tests/test_gpu_tall_stored.py::test_two_wave_blocks_and_streaming_same_words_as_generic_column",
    "MGX_C2F_KC": "tests/test_gpu_parity.py::test_transfer_kernel_variants_same_bits",
    "MGX_NO_RESREST": "tests/test_gpu_resrest_zw.py::test_generated_slots_same_fields",
    "MGX_RESREST_FLAT_MAX": "tests/test_gpu_parity.py::test_transfer_kernel_variants_same_bits",
    "MGX_RESREST_FLAT_S": "tests/test_gpu_parity.py::test_transfer_kernel_variants_same_bits",
    "MGX_RESREST_AHEAD": "tests/test_gpu_parity.py::test_transfer_kernel_variants_same_bits",
    "MGX_RESREST_NO_ZW": "tests/test_gpu_resrest_zw.py::test_generated_slots_same_fields",
    "MGX_P2P_MAXBLK": "tests/test_gpu_multirank.py::test_multirank_one_block_per_direction",
    "MGX_P2P_IPT": "tests/test_gpu_multirank.py::test_multirank_long_edge_path",
    "MGX_MODEL_KR": "tests/test_gpu_model_coupling.py::test_forced_run_lengths_against_the_oracle",
    "MGX_NO_MF": "tests/test_gpu_configs.py::test_in_kernel_coefficients_match_stored_slots_on_stretched_grids",
    "MGX_P2P_TIMEOUT_MS": "tests/test_gpu_multirank.py::test_multirank_one_block_per_direction",
}
