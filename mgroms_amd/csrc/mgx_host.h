// Host side of libmgx.so, shared by its host translation units (mgx_api.cpp, mgx_comm.cpp, mgx_cycle.cpp, mgx_define.cpp): solver state,
// level hierarchy, the small helpers every file uses and the prototypes of the host functions that cross files.  Host only: the HIP
// translation units see mgx_internal.h / mgx_device.h.  Mirrors the reference's module structure:
//   mg_grids.f90 (levels, neighbours, gather groups)      -> rank_level_table(), mgx_init()   (mgx_define.cpp)
//   mg_define_matrix.f90 (define_matrices_topo)           -> define_matrices()                (mgx_define.cpp)
//   mg_mpi_exchange.f90 (fill_halo_*, global_sum)         -> fill_halo_js(), rl_fill_halo(), global_sum()   (mgx_comm.cpp)
//   mg_gather.f90 (gather, split)                         -> inside fine2coarse()/coarse2fine()   (mgx_cycle.cpp)
//   mg_relax.f90 / mg_intergrids.f90 / mg_solvers.f90     -> relax(), residual(), fine2coarse(), ...   (mgx_cycle.cpp)
// There is no CPU compute path: every operator is a HIP kernel launch (mgx_residual.hip, mgx_transfer.hip, mgx_halo.hip, mgx_setup.hip, ...).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mgx.h"
#include "mgx_internal.h"

// Everything the host files share lives in this namespace: libmgx.so exports the C ABI of include/mgx.h and the kernel wrappers
// (mgx_wrappers.h) under their plain names, and nothing else without this prefix.
namespace mgx_host {

enum { M_GS = 0, M_RB = 1, M_FC = 2 };
inline bool all_physical(const Sides &s) { return s.S && s.E && s.N && s.W; }
inline bool any_physical(const Sides &s) { return s.S || s.E || s.N || s.W; }

struct Level {
  int nx, ny, nz, npx, npy, incx, incy, gather, ngx, ngy, key, color;
  int neighb[8];
  LevView v;    // solver fields (JS)
  LevView vs;   // pre-gather / split block (gathered levels): vs.b = restricted block, vs.p = split block
  GeoView g;    // set-up arrays (reference layout)
  double *tmp2[4];  // pre-gather coarse dx,dy,zeta,h
  double *blk, *gbuf;  // all-gather send / receive (reference layout blocks incl. halo)
  double *dblk = nullptr, *dgbuf = nullptr;  // the same for the interior block of zw, nz + 1 rows (the depths of mgx_matrices_depths*: blk, gbuf carry zr)
  bool pass_stored = false;  // the depths are the caller's and the level's colour pass would generate from the sigma fields it no longer has (depths_pass_stored, mgx_choice_depths.h): the pass takes the stored coefficients
  int group[4], ngroup;
  size_t n3js;  // doubles in one JS array
  bool r_halo_stale = false, b_halo_stale = false;  // deferred neighbour exchanges (multi-rank)
  size_t p2p_off[8][2];         // doubles into the receive slab: direction x parity
  unsigned long long p2p_seq = 0;  // exchanges done on this level through the peer-to-peer transport
  size_t p2p_goff[2];           // gathered levels: ngroup blocks of the peer-to-peer gather, by parity
  unsigned long long p2p_gseq = 0;
  unsigned int *ksp_done = nullptr; unsigned int ksp_seq = 0;  // per-plane progress counters of the persistent mid-level relax (k_relax_ksp) and their common value
  unsigned int *rbs_flag = nullptr; unsigned int rbs_seq = 0;  // progress word of the sequential-order red-black walk and the number of its launches (mgx_rbseq.hip: k_rbseq_scan, FUSE)
  double *gdec = nullptr; std::vector<double> gdec_h; int rbs_rows = 0;  // per row the largest |g(k) / g(1)| of the level (k_rbseq_gdecay) and the rows the correction reaches (mgxk_rbseq_window_rows)
  double rbs_rho = -1.0; int rbs_m = 0;  // sequential-order red-black, windowed walk (k_rbseq_window): rho = max |ag5| + |ag8| of the level, found at set-up, and the planes of warm-up it asks for (0 = none: the walk over the whole level)
  double *p1b = nullptr;        // second k=1 snapshot buffer (red-black on closed levels: one snapshot launch per relax call)
  double *zy_store, *zx_store;  // slope arrays; v.zy/v.zx point here while the matrix is the one define_matrices built
  double *f2d_store[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, *tab_store[2] = {nullptr, nullptr};  // m4,d4,m7,d7,h2,hi2,ze2 and cffw,csw (LevView)
  double *zg_store[4] = {nullptr, nullptr, nullptr, nullptr};  // dx2,dy2,cffr,csr (LevView)
  LevView32 v32 = {};           // fp32 shadow of the mixed-precision solve_p (allocated at the first mixed solve)
  size_t n3js32 = 0;            // floats in one of its JS arrays
};
inline bool held_pair(const Level &F, const Level &C) { return F.nz == C.nz; }   // options "hold_odd_nz", "hold_z_levels": the pair coarsens in x and y only
inline Sides sides_of(const Level &L) { return {L.neighb[0] < 0, L.neighb[1] < 0, L.neighb[2] < 0, L.neighb[3] < 0}; }

struct TicRec { int lev, sub; hipEvent_t e0, e1; };
struct HostTic { int lev, sub; std::chrono::steady_clock::time_point t0; };  // a section the caller opened with mgx_tic

struct State {
  bool inited = false, have_matrix = false;
  bool have_geometry = false;   // define_matrices has run: level 1 holds dx, dy, h, rmask and S the hc, theta_b, theta_s a zeta refresh keeps
  long long n_zeta_refresh = 0, n_zeta_chain = 0;   // read-only options "zeta_refreshes", "zeta_chain_launches"
  // the depths of every level are the caller's (mgx_matrices_depths*, mgx_update_depths_device): there is no h and no stretching to apply a new
  // zeta to, and no level carries the nine sigma fields; the next mgx_matrices / mgx_matrices_device clears it
  bool depths_user = false;
  long long n_depth_refresh = 0;   // read-only option "depth_refreshes"
  mgx_params par;
  int method = M_RB, real = 1, linear = 1;
  int nlevs = 0, npx = 1, npy = 1, nranks = 1, rank = 0, pi = 0, pj = 0;
  std::vector<Level> lev;
  double hlim = 0, theta_b = 0, theta_s = 0;
  hipStream_t stream = nullptr;
  mgx_exchange_fn ex = nullptr; mgx_allreduce_fn ar = nullptr; mgx_allgather_fn ag = nullptr; void *ctx = nullptr;
  bool native_rccl = false;  // the hooks are the library's own RCCL transport (mgx_rccl_connect)
  double *d_partial = nullptr; int npartial = 0;
  double *d_scalar = nullptr; double *h_scalar = nullptr;
  double *ref_scratch = nullptr; size_t ref_scratch_n = 0;  // reference-layout staging (8 x level-1 field)
  double *slope_scratch = nullptr;                          // zy, zx of the level in work (2 x level-1 field), mgx_setup.hip
  double *xbuf[16]; size_t xbuf_n = 0;                       // 8 send + 8 receive halo buffers
  // peer-to-peer halo transport (mgx_p2p_prepare / mgx_p2p_connect): receive slab + flags in fine-grained device memory,
  // the same slab and flags of every other rank opened through hipIpc
  bool p2p_ready = false, p2p_on = false, p2p_borrowed = false;  // borrowed: peers are plain pointers (mgx_p2p_connect_pointers)
  double *p2p_slab = nullptr; size_t p2p_slab_n = 0;
  unsigned long long *p2p_flags = nullptr;
  std::vector<double *> peer_slab; std::vector<unsigned long long *> peer_flags;
  unsigned int *p2p_counter = nullptr;
  int *p2p_err = nullptr;   // host-mapped
  int *kerr = nullptr;      // host-mapped error word of the persistent relax kernel (a plane's neighbour never showed up)
  long long n_p2p = 0;
  int p2p_failed = 0;       // a wait of this rank timed out since the ranks last agreed (global_sum): reported collectively there
  int p2p_test_drop = 0;    // test hook (option "p2p_test_drop" = n): the n-th halo exchange from now does not raise its flags
  int state_f32 = 0;    // d_u, d_v, d_w of the running call hold floats (the mgx_*_f32 entries; StateScope sets and resets it)
  int state_view = 0; mgx_state_strides state_str = {};   // d_u, d_v, d_w of the running call are the model's own padded arrays with these strides (the *_view entries; StateScope likewise)
  double *d_u = nullptr, *d_v = nullptr, *d_w = nullptr, *d_fx = nullptr, *d_fy = nullptr, *d_fz = nullptr, *d_bm = nullptr;  // model-layout scratch: the three fluxes of compute_rhs, divergence / pressure
  // the mask handed to nhydro_solve / nhydro_check_nondivergence on THIS call (nhydro.f90:72,82,98): staging copy in the
  // caller's layout and the i-fastest copy the model-space kernels read; call_mask = a mask came with the current call
  double *d_rmask_ref = nullptr, *d_rmask_m = nullptr; bool call_mask = false;
  std::vector<void *> allocs;
  int verbose = 1;
  int warm_start = 0;   // keep p between solves instead of the reference's cold start (mg_solvers.f90:35)
  int tictoc = 0;       // per-(level,name) GPU timers in the shape of mg_tictoc.f90
  int rb_chain = 1;     // red-black: chained k=1 snapshots on closed levels (0 = one snapshot launch per colour pass, for A/B tests)
  int keep_r = 0;       // cycles also store the interpolated correction in the fine r (dead state of the reference's coarse2fine)
  int rb_seq = 1;       // red-black with cmatrix='real' in the reference's sequential order by the parallel pass + a scan over the planes of the k=1 couplings + a rank-one correction per column (mgx_rbseq.hip): within a few ulp of mg_relax.f90:170-186, the DEFAULT; 0 = the plain parallel pass (old same-colour diagonals everywhere, 1e-4 per sweep away)
  int rb_exact = 0;     // red-black with cmatrix='real' in the reference's SEQUENTIAL order (plane after plane): bit-identical to mg_relax.f90:170-186, slow
  int exact_halos = 0;  // MGX_EXACT_HALOS=1: exchange r and b halos eagerly like the reference
  int no_mf = 0;      // MGX_NO_MF=1: always use the stored slots 3,5,6,8 (A/B tests)
  int use_small = 1;  // one-launch relax on small levels (MGX_NO_SMALL=1 disables, for A/B tests)
  int ksp_test_stall = 0;  // test hook (option "ksp_test_stall" = i): in the next persistent relax the workgroup of plane i returns at once
  int use_fuse = 1;   // option "fuse_tail" / MGX_NO_WAVE_FUSE=1: coarse2fine / residual+restriction folded into the one-workgroup relax of the level below the coarsest (A/B)
  int async_ops = 0;  // option "async": mgx_vcycle / mgx_fcycle / mgx_relax / mgx_fine2coarse / mgx_coarse2fine return without waiting for the stream
  int use_ksp = 1;    // option "ksp" / MGX_NO_KSP=1: one launch per colour pair instead of the persistent relax kernel (A/B)
  int ksp_down = 0;   // the persistent relax kernel timed out in this solver (its workgroups were not all resident): off until the next mgx_init
  // halo exchange beside the interior sweep (relax(), four colours on a level with neighbours, pushes on): a second stream carries the
  // boundary part of a colour pass and the exchange behind it while the solver's stream sweeps the interior
  hipStream_t stream2 = nullptr; hipEvent_t ev_a = nullptr, ev_s = nullptr, ev_x = nullptr;
  // OFF by default.  Measured (profiles/r04_overlap_2ranks.txt: two ranks of 512x512x64 sharing the one GPU of a test box): 8.4 ms per V-cycle with
  // it, 4.7 ms without.  A colour pass of such a block is ONE 512-register wave per SIMD for its whole duration: an exchange wave (or the boundary
  // part's) on a SIMD keeps the interior part's wave off it, and the boundary part alone takes as long as a whole pass (every wave runs the full
  // ~50 us), so the chain exchange -> boundary part -> exchange is no shorter than the serial one; the two cross-stream waits per colour come on top.
  int overlap = 0;       // option "overlap" / MGX_OVERLAP=1 (the same bits either way)
  long long n_overlap = 0;  // colour passes run that way
  int rbseq_fuse_min = 4 << 20;  // option "rbseq_fuse_min": cells of a colour (nx * ny/2 * nz) from which on the fused launch is used (below, the hand-off costs more than the correction's own launch: 256x256x32 0.111 ms per sweep fused, 0.099 separate)
  int rbseq_d0_in_pass = 1;  // option "rbseq_d0_in_pass" (A/B): 0 = k_rbseq_d0 as a launch of its own
  int rbseq_test_stall = 0;  // test hook: the walk of the fused launch never reports its progress (the bounded waits must end the launch)
  // option "coarsest_direct": the coarsest-level solve of a cycle (ns_coarsest sweeps from p = 0: a fixed linear map of b) as one matrix-vector product with the
  // operator the level's own relax kernel builds from the unit vectors when the matrix changes (mgx_relax_coarse.hip: k_coarse_direct).  The same map in
  // another association (1e-15 of max|p|), so: 1 (default) = only where the iteration is tolerance-based anyway (red-black in the sequential order at speed),
  // 2 = every method (four colours then lose their bit parity with the reference's loop), 0 = never
  int coarsest_direct = 1;
  double *cd_pb = nullptr, *cd_M = nullptr, *cd_part = nullptr; unsigned int *cd_cnt = nullptr;
  int cd_n = 0, cd_valid = 0, cd_method = -1, cd_mode = -1, cd_nsweeps = -1, cd_any = -1;   // cd_n: -1 = the level has no instance
  long long n_direct = 0;   // coarsest solves done that way
  // option "small_any_nz" (0 default, 1): relax calls on closed levels of at most 1024 columns with nz = 3, 5, 6, 7 (the coarse ends of the nz = 24,
  // 48, 96 hierarchies, and of nz = 20, 28, 40, 80 under "hold_odd_nz") run in one workgroup and one launch like their nz = 2, 4 neighbours
  // (mgxk_relax_small), and a coarsest level of nz = 3 takes the direct solve.  The same rows as the colour passes: the same bits for four colours,
  // 'simple', the parallel pass and rb_exact.  Off by default because it changes the launch counts of those levels.  May be set at any time.
  int small_any_nz = 0;
  long long n_small_any = 0;   // read-only option "small_any_nz_calls": relax calls and direct coarsest solves served by those instances since mgx_init
  int rbseq_rowcut = 1;  // option "rbseq_rowcut" (A/B): the windowed walk's correction stops at the last row it reaches to 2^-64 (Level::rbs_rows); 0 = every row
  int rbseq_window = 1;  // option "rbseq_window" / MGX_NO_RBSEQ_WINDOW=1: walk and correction of a colour by the windowed walk (k_rbseq_window: no hand-off, no walk over the whole level) on the levels whose contraction bound allows it (Level::rbs_m)
  long long n_window = 0;  // colours done that way
  long long n_tall_stored = 0;  // option "tall_stored_passes": colour passes the stored-coefficient tall-column kernel served (mgx_relax_tall.hip)
  double *rho_dev = nullptr, rho_host[32];  // the levels' rho (k_rbseq_rho) on the device and after the set-up's copy
  int rbseq_fuse = 1;    // option "rbseq_fuse" / MGX_NO_RBSEQ_FUSE=1: the correction of the sequential-order red-black inside the walk's launch (k_rbseq_scan, FUSE) instead of a launch behind it (A/B)
  int use_chain = 1;     // option "restrict_chain" / MGX_NO_RESTRICT_CHAIN=1: Fcycle's first-leg restrictions below level 1 as one launch (A/B)
  int fuse_closing = 1;  // option "fuse_closing" / MGX_NO_FUSE_CLOSING=1: the closing compute_residual(1) of a solve_p iteration also restricts its r for the next Fcycle, one kernel, no r written (A/B)
  // option "cycle_precision" (64 default, 32): solve_p keeps its fp64 iterate, residual, norm and stopping test and runs the F-cycle in
  // correction form on fp32 shadows of every level (solve_p_mixed, mgx_mixed.hip).  The shadows are allocated at the first mixed solve and
  // their coefficients converted again whenever the fp64 coefficients changed (coef_gen: define_matrices, mgx_set_field of cA)
  int cycle_precision = 64;
  // option "krylov" (0 default, 1..8): solve_p as truncated GCR / Orthomin(m) with one F-cycle from p = 0 as right preconditioner (solve_p_krylov,
  // mgx_krylov.hip); m = retained direction pairs.  kr_z / kr_q: m + 1 level-1 fields each (the retained pairs and the one in work), allocated at
  // the first solve with the option on (kr_n = pairs allocated); kr_sc: the scalars the kernels hand to each other, [0..7] (q, q_i), [8] s, [9] t,
  // [16..24] (q_i, q_i) by slot
  int krylov = 0;
  int kr_restarts = 0;            // read-only option "krylov_restarts": times the last solve fell back to the true residual
  int kr_n = 0;
  // option "krylov_precision" (64 default, 32; acts while krylov > 0): the preconditioner is the fp32 F-cycle of "cycle_precision" = 32 on the
  // shadows, A e = sigma r from e = 0.  The two conversions live in passes the loop runs anyway (k_kr_update32 leaves f = (float)(sigma r),
  // k_kr_apply32[_mf] reads z = e / sigma straight from the shadow): no conversion launch in steady state.
  int krylov_precision = 64;
  long long n_kr_mixed = 0;       // read-only option "krylov_mixed_iterations": Krylov iterations run with an fp32 cycle since mgx_init
  double *kr_z[9] = {}, *kr_q[9] = {}, *kr_sc = nullptr, *kr_partial = nullptr;
  long long n_mixed = 0;          // read-only option "mixed_iterations": solve_p iterations run with fp32 cycles since mgx_init
  bool mx_ready = false;
  // option "mixed_tail" (0 default, 1): the fp32 cycles run their tail -- the coarsest levels that are all small (mixed_tail_small,
  // mgx_internal.h) -- inside one workgroup, one launch per relax call, V-cycle tail or F-cycle tail (k_tail32, mgx_mixed.hip), the same
  // device text as the per-launch kernels and the same bits; 0 = one launch per colour pass and transfer on every level.  Off by default
  // because it changes what mgx_counters reports for an fp32 cycle, which callers (and tests/test_gpu_krylov_mixed.py) count by hand.
  int mixed_tail = 0;
  int mx_tail_first = 0;          // first level of that tail, 0 = no level is small (mixed_prepare)
  long long n_mixed_tail = 0;     // read-only option "mixed_tail_launches": launches of the tail kernel since mgx_init
  // option "mixed_ring" (0 default, 1): the colour passes of the fp32 cycles on the levels that are not small and whose nz has an instance
  // (choose_relax32, mgx_choice.h; mgx_mixed_ring_levels) run k_relax32r, the software-pipelined pass of mgx_mixed.hip, instead of k_relax32:
  // one launch per colour pass either way, other roundings within the same bound against the fp64 pass.  0 = every launch and bit as before.
  int mixed_ring = 0;
  long long n_mixed_ring = 0;     // read-only option "mixed_ring_passes": colour passes served by k_relax32r since mgx_init
  // option "mixed_direct" (0 default, 1): the coarsest solve of an fp32 cycle -- ns_coarsest sweeps from e = 0, a fixed linear map of f -- as one
  // product with B32, the operator of the fp64 level (mgxk_coarse_direct_build, parallel colour order) rounded once to fp32: k_coarse_direct32, or
  // a phase of the tail kernel (mgx_mixed.hip).  Served where the fp64 direct solve is (choose_mixed_direct_cells, mgx_choice.h); apart from
  // that solve's state (cd_*), of which only the scratch cd_pb is borrowed.  0 = every launch and bit as before.
  int mixed_direct = 0;
  float *md_M = nullptr; double *md_M64 = nullptr, *md_pb = nullptr;   // B32, the builder's fp64 matrix, its scratch where cd_pb does not exist
  int md_n = 0, md_valid = 0, md_any = -1;      // cells allocated for; the operator is built (0 with md_gen current: the builder declined)
  unsigned long long md_gen = ~0ULL;            // the coefficients it was built from (coef_gen)
  long long n_mixed_direct = 0;   // read-only option "mixed_direct_solves": coarsest solves of fp32 cycles served by the product since mgx_init
  unsigned long long coef_gen = 0, mx_gen = ~0ULL;
  // option "periodic" (0 default; bit 1 = the i direction, east-west; bit 2 = the j direction, north-south): read by mgx_init, which makes the rank
  // its own neighbour on the periodic sides of every level (rank_level_table).  Such a side is an open side like a rank seam: every kernel
  // reads what the last halo fill left there.  Where the level has one rank along the direction the neighbour is the rank itself and the fill a local
  // wrap (fill_halo_js: k_halo_wrap, or the direct copies of k_halo_exchange / k_halo_pack_all on a level that also has other ranks as neighbours;
  // exchange(): device copies); where it has more, the neighbour is the rank at the other end of the row or column and the fill the exchange of a
  // rank seam.  One rank is then the neighbour on several sides at once: exchange_plan() orders the entries of such a peer.
  int periodic = 0;
  // option "hold_odd_nz" (0 default, 1): read by mgx_init.  A level with an odd nz hands its nz on to the next level, which then coarsens in x and
  // y only (a "held pair": F.nz == C.nz), down to the horizontal bound of the hierarchy, instead of the reference's nz / 2 that drops the top row
  // and diverges.  The transfers of a held pair are the reference's 2-D operators row by row (mgx_hold.hip); every fast path that
  // assumes nz_c = nz_f / 2 declines such a pair.  0: the reference's table, word for word.
  int hold_odd_nz = 0;
  // option "hold_z_levels" (0 default, m = 1..8): read by mgx_init.  Semi-coarsening at the FINE end: the first m coarsenings (levels 1 -> 2 ...
  // m -> m + 1) keep nz and halve nx, ny -- held pairs like those of "hold_odd_nz", served by the same transfers -- and from level m + 1 on the
  // rule without the option applies.  For cells taller than wide, where the z-line smoother leaves the horizontally oscillatory error alone
  // (mgx_hold_z_hint names m).  The down leg of such a pair is one kernel that never writes r where the level has its slopes
  // (k_residual_restrict*<HELD>, mgx_resrest.hip).  0: every table, kernel, launch count and bit as without the option.
  int hold_z_levels = 0;
  int hold_z_fuse = 1;   // option "hold_z_fuse" (A/B): 0 = the down leg of every held pair and the closing residual on one stay two launches; same bits
  long long n_hold_z_fused = 0;   // read-only option "hold_z_fused": down legs and closing residuals of held pairs served by the fused kernel since mgx_init
  // the CSR export (mgx_operator_csr, mgx_transfer_csr): what the last *_csr_size call counted and for which matrix (which: -1 = A, 0 = R,
  // 1 = P) -- the *_csr call that follows fills buffers of that size and refuses any other count
  int ex_lev = 0, ex_which = -2; long long ex_nnz = -1;
  int c2f_skip = 1;   // the cycles' prolongation leaves the columns alone that the first colour of the following four-colour relax overwrites unread (option "c2f_skip", MGX_C2F_NOSKIP=1)
  long long n_launch = 0, n_halo = 0, n_exch = 0, n_allred = 0;
  std::string err, transport_name;
  // mg_tictoc.f90's module variables (subname, time, calls, nblev) + the HIP events still in flight
  std::vector<std::string> tt_names;
  std::vector<TicRec> tt_open, tt_done;
  std::vector<HostTic> tt_host;
  double tt_time[32][32] = {};
  long long tt_calls[32][32] = {};
  int tt_nblev = 0;
};

// Instances.  The reference keeps ONE solver per process in module-global state (grid(:), mg_grids.f90:113-117), and so does every
// caller that never asks for more: instance 0 exists from the start and every thread acts on it.  A thread may select another
// instance (mgx_instance_create / mgx_instance_select): all mgx_* calls of THAT thread then act on it.  Used to couple several
// domains from one process and to run several ranks of one job as threads of one process (tests: BASELINE config 5's 4x2 grid on
// the one GPU of a test box, which admits fewer processes than that).
extern State S0;
extern std::vector<State *> g_instances;
extern std::mutex g_instances_mu;
extern __thread State *Sp;   // (__thread, not thread_local: a plain pointer with a constant initialiser, so no call of an initialisation wrapper per access)
#define S (*Sp)
// solvers that hold device state right now: the persistent relax kernel needs all its workgroups resident together, which nothing
// guarantees once several instances (thread-ranks, coupled domains) put kernels on the same device
int live_instances();

// The order of a red-black relax of level L (relax, relax_fused and coarsest_solve must agree on it, or the fused and the unfused path of a
// cycle smooth in different orders): the parallel colour passes, the reference's plane loop bit for bit (option "rb_exact"), or the same
// order by the walk of mgx_rbseq.hip (option "rb_seq", where the level has its gk).  The values are the `mode` the kernels take.
enum { RB_PLAIN = 0, RB_EXACT = 1, RB_SEQ = 2 };
inline int rb_mode(const Level &L) {
  if (S.method != M_RB || !S.real) return RB_PLAIN;
  if (S.rb_exact) return RB_EXACT;
  return (S.rb_seq && L.v.gk != nullptr) ? RB_SEQ : RB_PLAIN;
}

int fail(const char *fmt, ...);
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define CHK(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)
#define NEED_INIT() do { if (!S.inited) return fail("mgx_init has not been called"); } while (0)
#define NEED_LEV(l) do { NEED_INIT(); if ((l) < 1 || (l) > S.nlevs) return fail("level %d out of range 1..%d", (l), S.nlevs); } while (0)
inline bool streq(const char *a, const char *b) { return strcmp(a, b) == 0; }

// ---- mgx_api.cpp: the option table ----
void options_from_env();                    // mgx_init: the environment variables that preset an option
std::vector<int> options_carried();         // mgx_clean: the values of the options that outlive it, in table order ...
void options_restore(const std::vector<int> &);   // ... and back into the fresh State

// ---- mgx_define.cpp ----
int dmalloc(double **p, size_t n);
int roundup(int a, int m);
void make_view(LevView &v, int nx, int ny, int nz);
int find_grid_levels(int npxg, int npyg, int nx, int ny, int nz, int hold = 0, int hold_z = 0);
void rank_level_table(int rank, std::vector<Level> &T, int npx0, int npy0, int nsmall, int periodic = 0, int hold = 0, int hold_z = 0);
void set_window_planes(bool known = true);
enum { DM_ALL = 0, DM_ZETA = 1, DM_DEPTHS_ALL = 2, DM_DEPTHS = 3 };
int define_matrices(int what = DM_ALL, bool may_return_early = false);
int set_call_mask(const double *rmask, bool dev);
int compute_rhs_dev();
int correct_uvw_dev();
int upload_uvw(const void *u, const void *v, const void *w, size_t esz);
int download_uvw(void *u, void *v, void *w, size_t esz);
// the state compute_rhs_dev / correct_uvw_dev work on while the scope lives: u, v, w device arrays of doubles or (f32) of floats, or,
// with u = nullptr, the staging buffers S.d_u, S.d_v, S.d_w themselves under that type; str: u, v, w are padded arrays with these strides
// (checked by the caller: mgx_state_view.h), nullptr: densely packed
struct StateScope {
  double *su, *sv, *sw; int sf, sview; mgx_state_strides sstr;
  StateScope(void *u, void *v, void *w, bool f32, const mgx_state_strides *str = nullptr);
  ~StateScope();
};

// ---- mgx_comm.cpp ----
struct XEntry { int peer, sd, rd; };   // one message pair of an exchange: what was packed for direction sd goes to peer, what peer sends lands in the halo of direction rd
int exchange_plan(const int *neighb, int rank, XEntry *out, int *self_mask);
int exchange(int n, const int *peer, double *const *sb, double *const *rb, const int *cnt, const int *dir = nullptr);
int fill_halo_js(Level &L, double *a, bool phys_done = false, bool xonly = false);
void rect(double *a, double *buf, int op, int nzz, int nh, int ny, int j0, int j1, int i0, int i1, int mj = 0, int cj = 0, int mi = 0,
          int ci = 0, int mj2 = 0, int cj2 = 0, int mi2 = 0, int ci2 = 0);
int rl_fill_halo(Level &L, double *a, int nzz, int nh, char c, bool xonly = false);
int global_sum(const Level &L, double *out);
void p2p_release();
int sync_stream();
int op_sync();

// ---- mgx_cycle.cpp ----
int tt_sub(const char *name);
void tic(int lev, const char *name);
void toc(int lev, const char *name);
void tt_collect();
struct TicScope { int lev; const char *name; TicScope(int l, const char *n) : lev(l), name(n) { tic(l, n); } ~TicScope() { toc(lev, name); } };
int relax(int lev, int nsweeps);
int residual(int lev, double *res);
int fine2coarse(int lev, bool dup_r = false, bool with_residual = false);
int coarse2fine(int lev, bool keep_r = true, bool skip1 = false);
int vcycle(int lev1, bool lead_c2f = false);
int vcycle2(int lev1, int lev2);
int fcycle(int have_r2 = 0);
std::string fortran_e3(double v, int width);
int solve_p_opt(double tol, int maxite, int *nite_out, double *res_out, double *hist);
int krylov_op(const char *op, int nd, double *const *f, const int *slot, const double *sin, double *sout, int *path);
int mixed_check();
int mixed_prepare();
int relax32(int lev, int nsweeps);
int coarsest_solve32(bool e_zero);
void coarse2fine32(int lev);
int vcycle32(int lev1, bool lead_c2f);

}  // namespace mgx_host
