/*
 * mgx.h -- C ABI of the MI355X-native multigrid pressure solver (libmgx.so).
 *
 * Drop-in boundary for the hot path of CESR-lab/mgroms: every entry point below
 * replaces one Fortran module procedure of the reference (file:line relative to
 * the reference's src/).  The reference has no C interop; a Fortran module
 * `nhydro` with the reference's five signatures forwards to these through
 * ISO_C_BINDING (fortran/nhydro.f90).  Like the reference
 * (module-global `grid(:)`, mg_grids.f90:113-117) the library holds ONE solver
 * instance per process unless the caller asks for more (mgx_instance_*, below);
 * one process drives one GPU.
 *
 * Conventions
 *  - all arrays are host pointers to double (real(kind=8)); the library owns
 *    every device array until mgx_clean().
 *  - 2-D geometry arrays are (0:ny+1, 0:nx+1), j fastest (mg_define_matrix.f90:71-76).
 *  - 3-D solver fields are (nz, 0:ny+1, 0:nx+1), k fastest (mg_grids.f90:207-209);
 *    cA is (8, nz, 0:ny+1, 0:nx+1) (mg_grids.f90:221).
 *  - model velocities are (i,j,k)-ordered, i fastest (nhydro.f90:57-59):
 *    u(1:nx+1,0:ny+1,1:nz)  v(0:nx+1,1:ny+1,1:nz)  w(0:nx+1,0:ny+1,0:nz).
 *  - every function returns 0 on success; on failure a non-zero code, and
 *    mgx_last_error() describes it (the reference would `stop -1`).
 */
#ifndef MGX_API_H_INCLUDED
#define MGX_API_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

/* The 13 members of namelist /nhparam/ (mg_namelist.f90:37-50), defaults :11-35 */
typedef struct mgx_params {
  double solver_prec;     /* 1e-6 */
  int solver_maxiter;     /* 50 */
  int nsmall;             /* 8 */
  int ns_coarsest;        /* 40 */
  int ns_pre;             /* 3 */
  int ns_post;            /* 2 */
  char cmatrix[16];       /* 'real' | 'simple' */
  char relax_method[16];  /* 'Gauss-Seidel','GS' | 'Red-Black','RB' | 'Four-Color','FC' */
  char interp_type[16];   /* 'linear' | 'nearest' */
  char restrict_type[16]; /* 'avg' (never read by the reference outside the namelist) */
  int aggressive;         /* .false. ; .true. is rejected (unimplemented in the reference, mg_intergrids.f90:243) */
  int netcdf_output;      /* .false. ; ignored (debug I/O, out of scope) */
  int bmask;              /* .false. ; .true. = masked coefficients, needs rmask in mgx_matrices */
} mgx_params;

/* field ids for mgx_get_field / mgx_set_field / mgx_fill_halo */
enum { MGX_P = 0, MGX_B = 1, MGX_R = 2, MGX_CA = 3, MGX_DX = 4, MGX_DY = 5, MGX_ZETA = 6, MGX_H = 7,
       MGX_ZR = 8, MGX_ZW = 9, MGX_CW = 10, MGX_RMASK = 14 };

/* fills *p with the defaults of mg_namelist.f90:11-35 */
int mgx_params_default(mgx_params *p);
/* read_nhnamelist (mg_namelist.f90:55-127): parse &nhparam from `path` (NULL = "nh_namelist");
 * a missing file keeps *p unchanged; linear+linear is rejected (:95-98). */
int mgx_read_namelist(const char *path, mgx_params *p);

/* nhydro_init(nx,ny,nz,npxg,npyg) (nhydro.f90:18-33).  nx,ny,nz: local block; npx,npy: process grid;
 * rank: this process's rank, placed at pi=mod(rank,npx), pj=rank/npx (mg_grids.f90:593-594).
 * par == NULL: read ./nh_namelist if present, else defaults (what the reference does).
 * nx, ny, nz must be even; nz need not be a power of two.  Coarser levels halve nz as the reference does (an odd level drops its
 * top row on restriction, mg_intergrids.f90:149-160), unless option "hold_odd_nz" holds an odd nz or option "hold_z_levels" = m holds nz on
 * the first m coarsenings (both read here, both off by default).  Level-1 colour pass: a register-resident kernel for nz in {2, 4, 8, 12, 16,
 * 20, 24, 32, 40, 48, 64}; a tall-column kernel for nz in {80, 96, 128}, in its matrix-free form when the matrix came from
 * define_matrices without bmask and on the stored coefficients otherwise (bmask, mgx_set_field(cA), MGX_NO_MF; the read-only option
 * "tall_stored_passes" counts the colour passes served that way since mgx_init); every other nz runs the generic kernel plus a
 * physical-halo launch per colour.
 * relax_method = 'GS' accepts any nz (register-resident columns for the powers of two up to 64, the generic column otherwise). */
int mgx_init(int nx, int ny, int nz, int npx, int npy, int rank, const mgx_params *par);
/* nhydro_matrices(dx,dy,zeta,h,rmask,hc,theta_b,theta_s) (nhydro.f90:36-50) -> define_matrices
 * (mg_define_matrix.f90:28-208).  rmask may be NULL (= all ones; only read when bmask). */
int mgx_matrices(const double *dx, const double *dy, const double *zeta, const double *h, const double *rmask,
                 double hc, double theta_b, double theta_s);
/* nhydro_solve(nx,ny,nz,rmask,u,v,w) (nhydro.f90:53-102): compute_rhs, solve_p, correct_uvw; u,v,w updated in place.
 * rmask = the mask of THIS call (rmaska, nhydro.f90:56,72): the same memory layout as in mgx_matrices, (0:ny+1,0:nx+1)
 * with j fastest -- what the reference's drivers allocate (mg_testseamount.f90:97) and what compute_rhs / correct_uvw
 * index as rmask(j,i) (mg_compute_rhs.f90:61,110; the explicit-shape dummy of nhydro_solve declares it (0:nx+1,0:ny+1),
 * which is the same memory for the square blocks the reference is run on; on a non-square block with a non-trivial mask the
 * reference's own indexing reads element j+(nx+2)*i of an array its drivers fill at j+(ny+2)*i -- the library keeps the
 * drivers' layout, deliberately).  As in the reference it multiplies the w
 * cross terms of compute_rhs whatever bmask says, and yields umask / vmask when bmask (mg_compute_rhs.f90:56-72,
 * mg_correct_uvw.f90:51-68).  NULL = the level-1 mask of mgx_matrices when bmask, else all ones. */
int mgx_solve(double *u, double *v, double *w, const double *rmask);
/* nhydro_solve with the model state already on the GPU: u,v,w (and rmask, when not NULL) are DEVICE pointers (same layouts); no PCIe traffic.
 * This is what a GPU-resident ocean model calls every time step. */
int mgx_solve_device(double *u_dev, double *v_dev, double *w_dev, const double *rmask);
/* nhydro_check_nondivergence (nhydro.f90:105-134): recompute the divergence into grid(1)%b */
int mgx_check_nondivergence(double *u, double *v, double *w, const double *rmask);
/* nhydro_clean (nhydro.f90:137-141) */
void mgx_clean(void);

/* ---- the set-up half of a device-resident time step (no Fortran counterpart: the reference's model is on the host) ----
 * mgx_matrices with DEVICE pointers: same layouts ((0:ny+1, 0:nx+1), j fastest), same refusals in the same words, the five copies
 * device-to-device on the solver's stream.  rmask_dev may be NULL unless bmask.  The arrays are read in stream order: keep them
 * unchanged until the call has returned (option "async" = 0) or until the next mgx_synchronize ("async" = 1). */
int mgx_matrices_device(const double *dx_dev, const double *dy_dev, const double *zeta_dev, const double *h_dev,
                        const double *rmask_dev, double hc, double theta_b, double theta_s);
/* The per-step call of a model with a moving free surface: a new level-1 zeta (device pointer, layout as above) under the dx, dy, h,
 * rmask, hc, theta_b, theta_s of the last mgx_matrices / mgx_matrices_device.  Refused before the first of those.
 * Rebuilt, by the kernels of mgx_matrices in their order, hence bit for bit what mgx_matrices(dx, dy, zeta_new, h, rmask, ...) leaves:
 * zeta, zr, zw, cw and cA of every level (both layouts), the pivots, the slopes, the red-black extras (g, rho, the decay figures:
 * mgx_rbseq_window_info / _rows), the 2-D zeta of the matrix-free passes and the model-space copies of zw, dzw, cw, zxdy, zydx.
 * Kept, and not recomputed: dx, dy, h of every level and their halos, the coarse masks, the sigma tables, the 2-D metric factors, the
 * model-space copies of dx, dy, rmask.  Invalidated as mgx_matrices does: the direct coarsest operator ("coarsest_direct": rebuilt at
 * the next cycle) and the fp32 copies of "cycle_precision" / "krylov_precision" = 32 (converted again at the next such solve).
 * A matrix installed with mgx_set_field(lev, MGX_CA, ...) is OVERWRITTEN, as mgx_matrices would overwrite it; dx, dy, h, rmask changed
 * through mgx_set_field on level 1 are taken as they are, on coarser levels they are kept as set.
 * On a hierarchy whose levels are all closed and un-gathered (a single rank) zeta reaches every level, halos included, in one launch
 * (mgx_setup.hip: k_zeta_chain; a second one from 7 levels on); levels with neighbours or a gather take one coarsening, one all-gather
 * where the level gathers and one halo fill each -- the call is then collective.
 * Waiting: with option "async" = 0 both calls return when the device has finished, like mgx_matrices.  With "async" = 1 they only enqueue,
 * and errors surface at mgx_synchronize -- unless relax_method = 'RB' with cmatrix = 'real' runs in the sequential order ("rb_seq" = 1), whose
 * windowed walk is sized on the host from rho and the decay figures of the new coefficients: then the read-back and its wait stay.  (Red-black
 * with "rb_seq" = 0 under "async" = 1 skips the read-back: mgx_rbseq_window_info then reports no window until the next waiting set-up.)
 * Read-only options: "zeta_refreshes" (default 0; calls of mgx_update_zeta_device served since mgx_init) and "zeta_chain_launches"
 * (default 0; how many of them took the one-launch path for the 2-D part). */
int mgx_update_zeta_device(const double *zeta_dev);
/* nhydro_check_nondivergence with the model state on the GPU (the pattern of mgx_solve_device): u, v, w and rmask (may be NULL) are DEVICE
 * pointers and are only read; the divergence is left in grid(1)%b.  Waits for the device. */
int mgx_check_nondivergence_device(double *u_dev, double *v_dev, double *w_dev, const double *rmask_dev);

/* ---- the float state: the model keeps u, v, w in single precision (no Fortran counterpart in the reference) ----
 * The contract, for float arrays u32, v32, w32 in the layouts of mgx_solve:
 *   mgx_solve_device_f32(u32, v32, w32, rmask) leaves in every element exactly (float) x, where x is what mgx_solve_device leaves in that
 *   element when called on (double) u32, (double) v32, (double) w32 under the same options.
 * The conversion rounds to nearest, ties to even; subnormal float results are kept; the sign of zero is kept; elements that correct_uvw
 * does not write come back with unchanged bits.  What follows from it:
 * - grid(1)%b, the residual history, *nite and p are bit-identical to the fp64 call on the promoted input: promotion is exact, and b is
 *   formed in fp64 by the same expressions (one text of every formula serves both state types, mgx_model.hip).
 * - each element of u, v, w is rounded once, at its store: correct_uvw computes in fp64, and one thread reads and writes each element once.
 * - rmask stays const double *, as in every other entry: it is 2-D, and mgx_matrices takes it as double anyway.
 * - every option composes and is served as in the fp64 call (relax_method, "krylov", "cycle_precision" = 32, "warm_start", bmask, the
 *   per-call mask, "periodic", "hold_odd_nz", process grids: the flux faces neighbours exchange are fp64 either way).
 * - no conversion pass and no 3-D allocation: each entry issues the kernel launches of its fp64 twin (mgx_counters), on the model's own
 *   float arrays (the device entries) or on the first half of the library's staging buffers (the host entries).
 * Rows of u hold nx + 1 floats, rows of v and w nx + 2: the arrays need the alignment of a float, no more.
 * A NULL u, v or w is refused with the entry's name in mgx_last_error().
 * mgx_solve_device_f32 / mgx_check_nondivergence_device_f32: DEVICE pointers, the twins of mgx_solve_device / mgx_check_nondivergence_device. */
int mgx_solve_device_f32(float *u_dev, float *v_dev, float *w_dev, const double *rmask_dev);
int mgx_check_nondivergence_device_f32(float *u_dev, float *v_dev, float *w_dev, const double *rmask_dev);
/* ... and on host arrays: the twins of mgx_solve, mgx_compute_rhs and mgx_check_nondivergence (floats cross PCIe, half the bytes) */
int mgx_solve_f32(float *u, float *v, float *w, const double *rmask);
int mgx_compute_rhs_f32(const float *u, const float *v, const float *w, const double *rmask);
int mgx_check_nondivergence_f32(float *u, float *v, float *w, const double *rmask);

/* ---- the state in the model's own padded arrays (no Fortran counterpart: there the compiler copies an array section in and out) ----
 * A model keeps u, v, w in arrays with ghost cells and padding (CROCO's GLOBAL_2D_ARRAY: i fastest, two or three ghost cells per side).
 * The *_view entries work on those arrays in place: no gather before the call, no scatter after it, no second copy of the state.
 * Addressing.  Each pointer names the FIRST LOGICAL ELEMENT of its array, u(1,0,1), v(0,1,1), w(0,0,0); the strides are in elements of
 * the state's type: sj from row j to row j + 1, sk from level k to level k + 1; the i stride is 1.  So
 *     u(i,j,k) = u[(i-1) + j sj + (k-1) sk],   v(i,j,k) = v[i + (j-1) sj + (k-1) sk],   w(i,j,k) = w[i + j sj + k sk]
 * over the shapes of mgx_solve: u(1:nx+1,0:ny+1,1:nz), v(0:nx+1,1:ny+1,1:nz), w(0:nx+1,0:ny+1,0:nz).  Only these elements are read, and
 * only the ones correct_uvw writes are written: the padding between rows and between levels is neither read nor written.
 * The densely packed arrays of mgx_solve_device are the strides sj = nx+1 (u) or nx+2 (v, w), sk = sj (ny+2) (u, w) or sj (ny+1) (v):
 * with them a view entry leaves the bits of the dense entry and issues its launches (mgx_counters).  One text and one instance of every
 * model kernel serves both (mgx_model.hip); the results never depend on the strides.
 * f32 = 0: u, v, w point to doubles; f32 = 1: to floats, under the contract of the float state above.
 * mgx_state_strides_check: host only, needs neither a GPU nor mgx_init.  Returns 1, with the array, the field and the offending value in
 * mgx_last_error(), for a stride that is not positive, an sj below the row length, an sk below sj x rows, or an extent whose last element
 * lies more than 63 bits' worth (in bytes of a double) from the first.  The view entries call it first and refuse in its words, then
 * behave as mgx_solve_device / mgx_check_nondivergence_device do, under every option ("async", "warm_start", "krylov", "hold_z_levels",
 * "periodic", process grids, every relax_method): they are those entries with other addresses.  A NULL u, v, w or s is refused.
 * rmask_dev stays in the library's dense layout ((0:ny+1, 0:nx+1), j fastest; may be NULL): a mask is set-up data, not per-step traffic.
 * mgx_update_zeta_device_view: the refresh of mgx_update_zeta_device from the model's own zeta, i FASTEST: zeta(i,j) = zeta_dev[i + j sj],
 * i = 0..nx+1, j = 0..ny+1, row pitch sj >= nx+2 (the pointer names zeta(0,0)).  One LDS-tiled transpose launch brings it into the level-1
 * array; from there the call is mgx_update_zeta_device and leaves bit for bit what that leaves for the transposed dense array, waits or
 * enqueues as that does, and counts in "zeta_refreshes".
 * Out of scope: the host-array entries (mgx_solve, mgx_solve_f32) and the Fortran module, which binds host arrays only; a pitched dx, dy,
 * h or rmask (set-up data); strides other than 1 along i. */
typedef struct { long long u_sj, u_sk, v_sj, v_sk, w_sj, w_sk; } mgx_state_strides;   /* in elements of the state's type */
int mgx_state_strides_check(int nx, int ny, int nz, const mgx_state_strides *s);
int mgx_solve_device_view(void *u, void *v, void *w, const mgx_state_strides *s, int f32, const double *rmask_dev);
int mgx_check_nondivergence_device_view(void *u, void *v, void *w, const mgx_state_strides *s, int f32, const double *rmask_dev);
int mgx_update_zeta_device_view(const double *zeta_dev, long long sj);

/* ---- the matrices from the model's own vertical grid: z_r, z_w instead of h, zeta and a stretching (no Fortran counterpart in the
 * reference, whose nhydro_matrices evaluates setup_zr_zw_croco / new_s_coord on every level) ----
 * For a model whose depths the library's one stretching does not produce -- the old S-coordinate, a stretching function of its own, ALE or
 * z-tilde variants: the caller hands over the depths of its rho points, zr(k), k = 1..nz, and of its interfaces, zw(k), k = 1..nz+1
 * (the model's z_w(0..N)), of level 1, and the library builds every level's operator from depths alone.
 * Coarser levels.  With (J, I) a coarse column, fj = 2J-1, fi = 2I-1 its four fine columns and
 *     avg(x) = 0.25 * (x(fj,fi) + x(fj+1,fi) + x(fj,fi+1) + x(fj+1,fi+1))     (in that order)
 * a pair of levels that halves nz (nz_F even) takes zw_C(kc) = avg(zw_F(2kc-1)), kc = 1..nz_C+1, and zr_C(kc) = avg(zw_F(2kc)), kc = 1..nz_C:
 * a coarse rho point is a fine interface; a held pair ("hold_z_levels", "hold_odd_nz": nz_C = nz_F) takes zw_C(k) = avg(zw_F(k)),
 * zr_C(k) = avg(zr_F(k)).  For a constant h and zeta this is the sigma hierarchy of mgx_matrices bit for bit; elsewhere it is a hierarchy
 * of its own (on a seamount 5e-6 ... 5e-4 of the depth away), which no reference pins.  A hierarchy that halves an ODD nz is refused, with
 * the level named: the rule has no top interface there; option "hold_odd_nz" = 1 is the way out.
 * Layouts.  s == NULL: the library's dense layout, what mgx_get_field(1, MGX_ZR / MGX_ZW, ...) returns -- zr(nz, -1:ny+2, -1:nx+2),
 * zw(nz+1, -1:ny+2, -1:nx+2), k fastest, two halo cells per side; the host entry takes only this one.  With s the pointers name
 * z_r(1,1,1) and z_w(1,1,0) of the model's own arrays, i fastest:
 *     zr(i,j,k) = zr_dev[(i-1) + (j-1) zr_sj + (k-1) zr_sk],   zw(i,j,k) = zw_dev[(i-1) + (j-1) zw_sj + (k-1) zw_sk],   k from 1
 * In EVERY layout only i = 1..nx, j = 1..ny are read: halos and padding are neither read nor written.  The library fills its own halos by
 * its own rules (the fill_halo of zr, zw with two cells: extrapolation at a closed side, the neighbour's columns at a rank seam or a
 * periodic side); h and zeta of every level are then set to -zw(1) and zw(nz+1), so that grid(lev)%h, %zeta stay what they mean.
 * dx, dy, rmask: as in mgx_matrices / mgx_matrices_device, dense; rmask may be NULL unless bmask.
 * Monotone depths are the caller's duty: zw strictly increasing in k and zw(k) < zr(k) < zw(k+1) in every column.  It is not checked.
 * mgx_depth_strides_check: host only, needs neither a GPU nor mgx_init; the refusals of mgx_state_strides_check in its words, for the
 * arrays zr (nx x ny x nz) and zw (nx x ny x (nz+1)): a stride that is not positive, an sj below the row length nx, an sk below sj x ny, an
 * extent beyond 63 bits.  The device entries call it first and refuse in its words.
 * mgx_update_depths_device: the per-step call -- new depths under the dx, dy, rmask of the last set-up; rebuilt, by the kernels of
 * mgx_matrices_depths_device in their order and hence bit for bit what it leaves: zr, zw, h, zeta, cw, cA of every level, the pivots, the
 * slopes, the red-black extras and the model-space copies.  Waits or, under option "async" = 1, only enqueues, exactly as
 * mgx_update_zeta_device does (the read-back of sequential-order red-black included).  Counted by the read-only option "depth_refreshes".
 * While the depths are the caller's:
 * - mgx_update_zeta_device and mgx_update_zeta_device_view are refused: there is no h and no stretching to apply a new zeta to;
 * - the levels keep their slopes (the operator, the transfers and the colour passes below nz = 32 stay matrix-free) and lose the nine
 *   fields from which the fastest kernels generate slots 4 / 7 and zw: those kernels' stored-slot instances run instead, and the colour
 *   pass of a level with nz >= 32 -- which has no instance between the two -- takes the stored coefficients.  The same bits either way.
 * - everything else is served as after mgx_matrices_device: every relax_method, "krylov", bmask, "periodic", "hold_odd_nz",
 *   "hold_z_levels", process grids with gathered levels (the calls are then collective), the _f32 and _view state entries,
 *   "coarsest_direct", "small_any_nz", the CSR export, and the fp32 cycles, whose coefficients are conversions of the stored fp64 ones.
 * A later mgx_matrices / mgx_matrices_device restores the library's own grid and its generated fields; so does mgx_clean.
 * mgx_depths_launch: the launches of the kernels above for a level 1 of nx x ny x nz, pure host logic (mgx_choice_depths.h): out[0..7] =
 * the transpose of the strided layout (i tiles, k tiles of zr, of zw, grid.x, grid.y, block.x, block.y, LDS bytes), out[8..9] = the dense
 * copy (grid, block), out[10..11] = the coarsening onto level 2 (grid, block), out[12..15] = the h, zeta pass (grid.x, grid.y, block.x,
 * block.y), out[16] = 1 where the level's colour pass takes the stored coefficients. */
typedef struct { long long zr_sj, zr_sk, zw_sj, zw_sk; } mgx_depth_strides;   /* in elements; the i stride is 1 */
int mgx_depth_strides_check(int nx, int ny, int nz, const mgx_depth_strides *s);
int mgx_matrices_depths(const double *dx, const double *dy, const double *zr, const double *zw, const double *rmask);
int mgx_matrices_depths_device(const double *dx_dev, const double *dy_dev, const double *zr_dev, const double *zw_dev,
                               const mgx_depth_strides *s, const double *rmask_dev);
int mgx_update_depths_device(const double *zr_dev, const double *zw_dev, const mgx_depth_strides *s);
int mgx_depths_launch(int nx, int ny, int nz, int *out);

/* mg_solvers.f90:17-101 solve_p(tol,maxite).  *nite = iterations done, *res = last ||r||/||b||,
 * hist (may be NULL, else >= maxite+1 doubles) = normalised residual after each iteration, hist[0] = initial. */
int mgx_solve_p(double tol, int maxite, int *nite, double *res, double *hist);
/* mg_solvers.f90:104-126.  Fcycle restricts grid(1)%r on its way down: call mgx_residual for level 1 first, as solve_p does
 * (:50); the r a previous cycle's coarse2fine would have left there is not kept unless option "keep_r" is set. */
int mgx_fcycle(void);
int mgx_vcycle(int lev);                  /* mg_solvers.f90:129-151 */
int mgx_vcycle2(int lev1, int lev2);      /* mg_solvers.f90:155-177 partial V-cycle down to lev2 */
int mgx_relax(int lev, int nsweeps);      /* mg_relax.f90:16-47   */
int mgx_residual(int lev, double *res);   /* mg_relax.f90:337-383: r = b - A p, halo fill of r, *res = global ||r||_2 */
int mgx_fine2coarse(int lev);             /* mg_intergrids.f90:16-72  */
int mgx_coarse2fine(int lev);             /* mg_intergrids.f90:167-228 */
int mgx_fill_halo(int lev, int field);    /* generic fill_halo (mg_mpi_exchange.f90:10-16): p,b,r (:396-745); dx,dy,zeta,h (2D :23-352); zr,zw (nh=2 :750-1242); cA (4D :1247-1534); collective */
/* testgalerkin(lev) (mg_solvers.f90:203-288): *norm_c = <p,A p> on level lev, *norm_f = <I p, A I p> on level lev-1 (the reference
 * prints norm_c, norm_f/4 and norm_c/norm_f*4).  The coarse field is grid(lev)%p as the caller set it (the reference draws
 * it with random_number); b of both levels is zeroed. */
int mgx_testgalerkin(int lev, double *norm_c, double *norm_f);
/* ---- the level operators and transfers as CSR matrices on the device (no Fortran counterpart; single rank) ----
 * Index convention: the unknown of interior cell (k, j, i) of a level of nx x ny x nz has index ((i-1)*ny + (j-1))*nz + (k-1) -- the
 * reference's k-fastest order, 0-based.  Halo cells are not unknowns.
 * mgx_operator_csr: A of level lev with the sign of compute_residual, r = b - A p.  The level's halo rule is folded in: the image of a
 *   closed side adds its coefficient to the entry of its interior source, a "periodic" wrap points at the cell one period away.  It is whatever
 *   mgx_residual(lev) applies today: matrix-free or stored, bmask, a matrix set by mgx_set_field(lev, MGX_CA, ...), either cmatrix.
 * mgx_transfer_csr, which = 0: R, nrows = the unknowns of lev + 1, ncols = those of lev -- what mgx_fine2coarse(lev) does to grid(lev)%r to
 *   produce grid(lev+1)%b.  which = 1: P, nrows = the unknowns of lev, ncols = those of lev + 1 -- what mgx_coarse2fine(lev) adds to grid(lev)%p
 *   from grid(lev+1)%p whose halo holds what mgx_fill_halo(lev + 1, MGX_P) puts there (as inside a cycle), under the live interp_type.  The held
 *   pairs of "hold_odd_nz" / "hold_z_levels" are served.
 * How: the library's own residual / fine2coarse / coarse2fine is applied to sums of unit vectors that no row can confuse (mgx_export.h) and the
 *   entries are read off the result: every value is bit for bit the number the kernels use.  An export costs some dozens of operator
 *   applications, three level-sized scratch fields and 8 bytes per row; nothing of it is kept.
 * Output: rowptr (nrows + 1 ints), col and val (nnz each) are DEVICE pointers.  Rows are sorted by column, no column twice; entries whose
 *   value is +-0 are dropped (a land row may be empty).  The *_size call reports the exact counts; the *_csr call must follow a *_size call for
 *   the same matrix and refuses when the count has changed since.
 * State: p, b, r of the level (for a transfer: of both levels), their halos and the deferred-halo state are left bit for bit as found;
 *   mgx_counters may grow; nothing else is visible afterwards.  Both calls wait for the device.
 * Refused: before mgx_matrices (or a mgx_set_field of cA); lev out of range, or no coarser level for a transfer; a process grid larger than
 *   1 x 1 (a distributed CSR needs a global numbering); a level whose rows or entries do not fit an int. */
int mgx_operator_csr_size(int lev, long long *nrows, long long *nnz);
int mgx_operator_csr(int lev, int *rowptr_dev, int *col_dev, double *val_dev);
int mgx_transfer_csr_size(int lev, int which, long long *nrows, long long *ncols, long long *nnz);
int mgx_transfer_csr(int lev, int which, int *rowptr_dev, int *col_dev, double *val_dev);
/* compute_rhs / correct_uvw on the device-resident model state (mg_compute_rhs.f90:14, mg_correct_uvw.f90:15) */
int mgx_compute_rhs(const double *u, const double *v, const double *w, const double *rmask);

/* grid(lev)%<field> accessors (mg_grids.f90:24-65), host layout as described above */
int mgx_nlevs(void);
int mgx_level_dims(int lev, int *nx, int *ny, int *nz);
/* sequential-order red-black, windowed walk (option "rbseq_window"): the level's contraction bound rho = max |ag5| + |ag8| (-1: not a red-black
 * solver with cmatrix='real') and the planes of warm-up chosen from it (0 = the walk over the whole level stays).  No Fortran counterpart. */
int mgx_rbseq_window_info(int lev, double *rho, int *planes);
/* ... and the rows (from the bottom) its correction reaches: above the last row where max over the columns of |g(k) / g(1)| exceeds 2^-64 nothing is
 * read or written (option "rbseq_rowcut"); nz = every row. */
int mgx_rbseq_window_rows(int lev, int *rows);
/* out[0..9] = npx,npy,incx,incy,gather,ngx,ngy,key,color,0 ; out[10..17] = neighbours S,E,N,W,SW,SE,NE,NW (-1 = none) */
int mgx_level_info(int lev, int *out);
/* Pure host logic of find_grid_levels / define_grid_dims / define_neighbours / define_gather_informations
 * (mg_grids.f90:468-738) for any rank, usable before mgx_init and without a GPU.  out: 20 ints per level =
 * nx,ny,nz,npx,npy,incx,incy,gather,ngx,ngy,key,color, neighbours S,E,N,W,SW,SE,NE,NW.  Returns nlevs, or -1. */
int mgx_level_table(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int maxlev, int *out);
/* The same with option "periodic" (0..3) as an argument: the neighbours of any rank of a periodic process grid, as mgx_init will build them.
 * periodic = 0 is mgx_level_table.  Host only. */
int mgx_level_table_periodic(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int maxlev, int *out);
/* The same with options "periodic" (0..3) and "hold_odd_nz" (0, 1) as arguments: the table mgx_init will build under them.  hold = 1: level
 * l + 1 exists iff l < nl1 (the horizontal bound of find_grid_levels) and nz_l != 2, with nz_{l+1} = nz_l / 2 for an even nz_l and nz_l for an odd
 * one; nx, ny and the gathers are those of hold = 0.  hold = 0 is mgx_level_table_periodic.  Host only. */
int mgx_level_table_hold(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int hold, int maxlev, int *out);
/* The same with option "hold_z_levels" (hold_z = m, 0..8) as an argument too.  The first m coarsenings (levels 1 -> 2 ... m -> m + 1) keep nz and
 * halve nx, ny; from level m + 1 on the rule of `hold` applies unchanged.  nx, ny and the gathers are those of the reference's table.  With
 * hold = 0 the table has min(nl1, m + nl2) levels (nl1, nl2: the horizontal and the vertical bound of find_grid_levels); an m above nl1 - 1
 * holds every pair.  hold_z = 0 is mgx_level_table_hold.  Host only. */
int mgx_level_table_semi(int nx, int ny, int nz, int npx, int npy, int rank, int nsmall, int periodic, int hold, int hold_z, int maxlev, int *out);
/* A value for option "hold_z_levels" from the geometry of a rank's block: *m = the smallest m in 0..8 with
 * 2^m * min(dx, dy) >= max(h) / nz, both extrema over the interior (i = 1..nx, j = 1..ny) -- the coarsenings in x and y after which the cells
 * are no longer taller than wide.  dx, dy, h: HOST arrays in the layout of mgx_matrices, (0:ny+1, 0:nx+1) with j fastest.  Pure host logic,
 * usable before mgx_init and without a GPU.  On a process grid every rank must build the same hierarchy: the caller takes the MAXIMUM of *m
 * over the ranks and sets that.  Returns 0, or non-zero (mgx_last_error) for NULL arguments and a geometry that is not positive and finite.
 * A model that hands over its own depths (mgx_matrices_depths*) has no h array of this kind: h = -zw(1), the depth of the bottom interface. */
int mgx_hold_z_hint(const double *dx, const double *dy, const double *h, int nx, int ny, int nz, int *m);
/* The first level of the tail of an fp32 cycle (option "mixed_tail") on the one-rank hierarchy of nx x ny x nz: *first = the finest level from
 * which every level down to the coarsest has at most 32768 cells and nz <= 32, 0 = no level is that small.  Pure host logic, usable before
 * mgx_init and without a GPU.  Returns 0, or non-zero (mgx_last_error) for sizes that make no hierarchy. */
int mgx_mixed_tail_first(int nx, int ny, int nz, int *first);
/* The levels whose fp32 colour passes option "mixed_ring" hands to the software-pipelined kernel, on the one-rank hierarchy of nx x ny x nz:
 * bit lev-1 of *mask is set where level lev is served -- nz one of 16, 20, 24, 32, 40, 48, 64 and the level not small in the sense of
 * mgx_mixed_tail_first (more than 32768 cells, or nz > 32).  Pure host logic, usable before mgx_init and without a GPU.  Returns 0, or
 * non-zero (mgx_last_error) for sizes that make no hierarchy. */
int mgx_mixed_ring_levels(int nx, int ny, int nz, int *mask);
/* The launch that option "mixed_ring" = 1 makes for one colour pass of nplanes planes (nx / 2 with four colours, nx red-black) of a level of
 * nx x ny x nz: out[0] = 1 where the pipelined kernel serves the level (0: the row-by-row kernel, and out[1..3] = 0), out[1] = rows of look-ahead,
 * out[2] = planes per workgroup, out[3] = 1 for the non-temporal instance, out[4] = workgroups, out[5] = the NZ of the instance.  Pure host
 * logic (the answer of the function the launch is made by), usable before mgx_init and without a GPU.  Returns 0, or non-zero (mgx_last_error). */
int mgx_mixed_ring_choice(int nx, int ny, int nz, int nplanes, int *out);
/* Where option "mixed_direct" serves the coarsest solve of an fp32 cycle as one matrix-vector product, on the one-rank hierarchy of
 * nx x ny x nz: *cells = the cells of the coarsest level when the product serves it, 0 when the sweeps run.  any_nz = the value of option
 * "small_any_nz".  Served: a coarsest level with nz = 2 or 4 (or 3 with any_nz), even nx and ny and at most 2048 cells (inclusive), in a
 * hierarchy of at least two levels -- the rule of the direct solve of "coarsest_direct".  Pure host logic (the answer of the function the launch
 * is made by), usable before mgx_init and without a GPU; the option's value does not move it.  Returns 0, or non-zero (mgx_last_error) for
 * sizes that make no hierarchy. */
int mgx_mixed_direct_cells(int nx, int ny, int nz, int any_nz, int *cells);
/* The entry list of one halo exchange of `rank` whose neighbours are neighb[0..7] (S,E,N,W,SW,SE,NE,NW; -1 = none), as the library hands it to
 * the exchange hook: entries[3t..3t+2] = peer, send direction, receive direction of entry t -- sendbuf[t] holds what was packed for the send
 * direction, recvbuf[t] is unpacked into the halo of the receive direction; both are of one kind (S/N edge, E/W edge, corner).  For each peer
 * the sends go in ascending direction and the receive slots in ascending order of the SENDER's direction (the opposite of the slot's).
 * Directions whose neighbour is the rank itself are not entries: their bits are set in *self_mask (may be NULL).  Returns the number of
 * entries (<= 8), -1 for a table no decomposition produces.  Pure host logic, usable without a GPU. */
int mgx_exchange_plan(const int *neighb, int rank, int *entries, int *self_mask);
/* In a multi-rank run mgx_get_field(lev, MGX_R | MGX_B, ...) is COLLECTIVE when the neighbour part of that field's halo is still
 * pending (the cycle defers the exchanges nothing reads): every rank must ask, as with mgx_fill_halo. */
int mgx_get_field(int lev, int field, double *host);
int mgx_set_field(int lev, int field, const double *host);

/* ---- multi-rank plumbing (replaces MPI in mg_mpi_exchange.f90 / mg_gather.f90) ----
 * The data path stays on the GPU: the library packs edges into device buffers and asks the host layer
 * (torch.distributed over RCCL) to move them.  All pointers handed to the callbacks are DEVICE pointers.
 *  exchange : for q in 0..n-1 send sendbuf[q] (count[q] doubles) to peer[q] and receive recvbuf[q]
 *             (count[q] doubles) from the same peer                           (fill_halo_*, :504-718)
 *  allreduce: in-place sum of n doubles over all ranks                          (global_sum, :1555-1571)
 *  allgather: gather `count` doubles from each of the `ng` ranks in `group` (ordered as the reference's
 *             localcomm, mg_grids.f90:702-718) into recvbuf                     (gather_3D, mg_gather.f90:126)
 * Each returns 0 on success.  Work must be enqueued on / ordered with the stream given to mgx_set_stream.
 * CONTRACT of exchange: entries that name ONE peer are matched in list order -- the k-th send to a peer is the message that peer's k-th receive
 * from this rank takes, on both sides.  With option "periodic" on a process grid one rank is the neighbour on several sides at once (east and
 * west with two ranks along a periodic direction; S, SW and SE with one), the counts are equal, and any other matching is a silent swap of
 * halos.  The library orders its lists for this rule (mgx_exchange_plan).  Kept by: torch.distributed batch_isend_irecv, MPI point-to-point
 * with one tag (non-overtaking), the thread-rank queues, the grouped ncclSend / ncclRecv of the native transport.  The rank itself is never a
 * peer of the list. */
typedef int (*mgx_exchange_fn)(void *ctx, int n, const int *peer, double *const *sendbuf, double *const *recvbuf,
                               const int *count);
typedef int (*mgx_allreduce_fn)(void *ctx, double *devbuf, int n);
typedef int (*mgx_allgather_fn)(void *ctx, const int *group, int ng, const double *sendbuf, double *recvbuf, int count);
int mgx_set_comm(mgx_exchange_fn ex, mgx_allreduce_fn ar, mgx_allgather_fn ag, void *ctx);

/* ---- native RCCL transport: the same three operations served inside libmgx.so by RCCL calls on the solver's stream
 * (ncclGroupStart / ncclRecv / ncclSend / ncclGroupEnd per halo fill, a one-double ncclAllReduce, grouped send/recv inside
 * the gather groups), replacing the MPI calls of mg_mpi_exchange.f90:504-718,1555-1571 and mg_gather.f90:126 with no host
 * language in the loop.  librccl is bound at run time (the copy already in the process, else librccl.so.1).
 * Bootstrap (collective, one rank per GPU, device selected by the caller): rank 0 obtains the id, the caller broadcasts its
 * mgx_rccl_unique_id_bytes() bytes (MPI_Bcast, torch.distributed, ...), every rank connects; connecting installs the
 * hooks (as mgx_set_comm would).  mgx_rccl_selftest (after mgx_init, collective): rank-coded exchange + all-reduce. */
int mgx_rccl_unique_id_bytes(void);
int mgx_rccl_get_unique_id(void *id_out);
int mgx_rccl_connect(const void *id, int nranks, int rank);
int mgx_rccl_disconnect(void);
int mgx_rccl_selftest(void);
/* human-readable name of the transport that carries the halos right now */
const char *mgx_transport(void);

/* HIP stream (hipStream_t) every kernel is launched on; NULL = the default stream */
int mgx_set_stream(void *hip_stream);
/* 0 = silent, 1 = the reference's rank-0 prints (parameter block, level table, "ite = ..: res = .. / conv = ..") */
int mgx_set_verbose(int level);

/* Options (0/1): "warm_start" keep p between solves instead of the cold start of mg_solvers.f90:35;
 * "tictoc" per-(level,name) timers like mg_tictoc.f90 (HIP events); "exact_halos" exchange the never-read r/b halos
 * eagerly as the reference does; "keep_r" (default 0) the cycles' coarse2fine also leaves the interpolated correction in the
 * fine level's r as mg_intergrids.f90:218-226 does (dead state: compute_residual rewrites r before anything reads it; the
 * mgx_coarse2fine operator always stores it, and so do the cycles under "exact_halos"); "verbose"; "p2p" (see below); "rb_chain" (default 1) red-black with cmatrix='real' on a
 * single-rank level: the colour passes write the next sweep's k=1 snapshot themselves, 0 = one snapshot launch per pass;
 * "c2f_skip" (default 1; MGX_C2F_NOSKIP=1 = 0): inside a cycle the prolongation before a four-colour relax does not update the
 * (i odd, j odd) columns, which that relax's first colour overwrites without reading them (mg_relax.f90:212-216) -- the coupling is
 * asserted by tests/test_gpu_parity.py::test_c2f_skip_is_invisible; 0 updates every column as the reference does;
 * Red-black with cmatrix='real' (the reference default) depends on the reference's SEQUENTIAL loop order (mg_relax.f90:170-186: a column
 * reads the same-colour k=1 diagonals of plane i-1 already updated, :271-276).  Three modes:
 * "rb_seq" (default 1; environment MGX_RB_SEQ): that order at speed -- parallel colour pass, a walk over the planes for the k=1 couplings,
 *   a rank-one correction per column (mgx_rbseq.hip): the reference's iterates up to the association of one sum per column (tests: 1e-12
 *   per relax call, histories within 1e-10), including the decomposition dependence on several ranks;
 * "rb_exact" (default 0; MGX_RB_EXACT): the same order bit for bit, one launch per i-plane (a parity mode, ~90 times slower);
 * both 0: the plain parallel sweep, same-colour diagonals as they were before the pass (the reference's own results differ by 2.5e-6
 *   between decompositions for the same reason; 5e-5 on the history).
 * "fuse_closing" (default 1; MGX_NO_FUSE_CLOSING): inside solve_p the closing compute_residual(1) of an iteration also restricts its r
 *   for the next Fcycle in the same pass (into grid(2)%r; grid(1)%r is materialised once, after the loop); 0 = the two operators.
 *   The fused kernel sums the norm in another order than compute_residual: between 1 and 0 the printed norms and hist agree to
 *   rounding (the tests compare them at 1e-13 relative), not bit for bit.
 * "restrict_chain" (default 1; MGX_NO_RESTRICT_CHAIN): Fcycle's first-leg restrictions below level 1 on closed levels as one launch
 *   (mgx_transfer.hip: k_restrict_chain), 0 = one launch per level; the same bits.
 * "rbseq_fuse" (default 1; MGX_NO_RBSEQ_FUSE): with "rb_seq", walk and per-column correction of a colour in ONE launch -- on large levels
 *   the correction chases the walk across the XCDs (mgx_rbseq.hip: k_rbseq_scan, FUSE), on small levels (half-rows of at most 64 columns,
 *   at most 128 planes) every workgroup redoes the walk for its own planes (k_rbseq_walk_apply); 0 = the correction in a launch of its
 *   own behind the walk; the same bits.  A lost hand-off inside the large-level launch (its waits are bounded) makes the next
 *   synchronising call fail and switches the option off (read it back).
 * "rbseq_window" (default 1; MGX_NO_RBSEQ_WINDOW): with "rb_seq", walk and correction of a colour in one launch WITHOUT a walk over the whole
 *   level (mgx_rbseq.hip: k_rbseq_window).  The walk's recurrence contracts by rho = max |ag5| + |ag8| per plane (a property of the matrix, found
 *   when the coefficients are built: mgx_rbseq_window_info); a walk started from zero m planes before a plane has forgotten its start to
 *   rho^m, and m is chosen so that rho^m <= 2^-64 (half an ulp of the largest increment).  Every workgroup walks the m planes in front of
 *   its own over its chunk of columns +- 32; nothing is handed from one workgroup to another.  Used on every level where m <= 48 (rho <~ 0.39:
 *   0.03-0.04 on the seamount problem); otherwise, and with 0, the walk over the whole level ("rbseq_fuse").  Not the same bits as that
 *   walk (a truncation of 2^-64 of the largest increment), inside the same tolerances (tests: 1e-12 per relax call against "rb_exact").
 *   Read-only: "rbseq_window_colours" (colours done that way since mgx_init).
 * "rbseq_rowcut" (default 1): the correction p = y + g s of the windowed walk stops at the last row it reaches -- g = T^-1 e1 decays away from the bottom
 *   row, and above the last row where max over the columns of |g(k) / g(1)| exceeds 2^-64 (found with the coefficients: mgx_rbseq_window_rows) the
 *   correction is below 2^-63 of the largest increment: those rows are neither read nor written (55 of 64 rows on level 1 of 512x512x64, 56 of 128 at
 *   nz = 128); 0 = every row (A/B).
 * "coarsest_direct" (default 1; MGX_COARSEST_DIRECT=n): inside a cycle the coarsest level is entered with p = 0 and left after relax(nlevs, ns_coarsest)
 *   (mg_solvers.f90:117,144): a fixed linear map of b.  Its matrix is built with the level's own relax kernel from the unit vectors whenever the
 *   coefficients change (lazily, at the first cycle after) and the solve becomes one matrix-vector product (mgx_relax_coarse.hip: k_coarse_direct; closed,
 *   un-gathered coarsest levels of at most 2048 cells).  The same map in another association -- not the same bits as the sweeps (1e-15 of max|p|) -- so:
 *   1 = only where the iteration is tolerance-based anyway (relax_method='RB', cmatrix='real' in the sequential order at speed, "rb_seq"), 2 = every method
 *   (four colours then lose their bit parity with the reference's loop), 0 = never.  relax(nlevs, n) called as an operator always sweeps.
 *   Read-only: "coarsest_direct_solves".
 * "rbseq_fuse_min" (default 4194304): cells of a colour (nx * ny/2 * nz) from which on a level counts as large for "rbseq_fuse".
 * "rbseq_timeout_ms" (default 2000; write-only): bound of the waits inside that launch.
 * "rbseq_d0_in_pass" (default 1): the colour pass also writes the walk's d0 (0 = a launch of its own; the same bits).
 * "overlap" (default 0; MGX_OVERLAP=1): four colours on a level with neighbours, halos by the pushes: the boundary part of a colour pass and
 *   the exchange on a second stream beside the interior part.  Same bits; slower where it could be measured.
 * "ksp" (default 1): the persistent relax of the closed mid levels; read back 0 after it timed out (then off until mgx_init or "ksp" = 1).
 * "cycle_precision" (64 default, or 32; any other value is refused; survives mgx_clean / mgx_init): 32 = mixed-precision solve_p.  The iterate,
 *   r = b - A p, its norm, the history, the stopping test and the prints stay fp64 as in solve_p; each iteration runs the F-cycle in correction
 *   form on fp32 copies of every level (A e = r / ||r|| from e = 0, same nsmall hierarchy, interp_type and relax_method; red-black as the parallel
 *   pass of rb_seq = 0) and adds the correction to p (iterative refinement, mgx_mixed.hip).  Applies to mgx_solve_p and through it to
 *   mgx_solve / mgx_solve_device.  The operator entry points (mgx_fcycle, mgx_vcycle, mgx_vcycle2, mgx_relax, mgx_residual, mgx_fine2coarse,
 *   mgx_coarse2fine) stay the reference's fp64 operators on grid(lev) fields whatever the option says.  Refused at the first mixed solve:
 *   a process grid larger than 1 x 1, relax_method = 'GS', option "rb_exact".  The fp32 copies (~48 B per cell) are allocated at the first
 *   mixed solve and their coefficients converted again after every mgx_matrices / mgx_set_field of cA.
 *   Read-only: "mixed_iterations" (solve_p iterations run with fp32 cycles since mgx_init).
 * "krylov" (default 0 = off, or m = 1..8; any other value is refused; survives mgx_clean / mgx_init): solve_p as right-preconditioned truncated GCR
 *   (Orthomin(m)) with one F-cycle from p = 0 as preconditioner and m retained direction pairs (mgx_krylov.hip).  Same contract as solve_p:
 *   tol is on ||b - A p|| / ||b||, maxite counts F-cycles, *nite, *res, hist, the printed lines and fort.100 keep their meaning; "warm_start"
 *   works; every relax_method, bmask, the per-call mask, any process grid.  Applies to mgx_solve_p and through it to mgx_solve / mgx_solve_device.
 *   The history entries of the iterations are the recurrence's residual norms; before the loop is left the true b - A p is computed, and where it
 *   is not below tol it replaces the recurrence's r, the retained pairs are dropped and the loop goes on.  On return grid(1)%r, *res and the last
 *   hist entry are the true residual's.  A vanishing or non-finite step leaves p as it was and ends the solve.  Costs 2 m + 2 extra level-1
 *   fields, allocated at the first solve with the option on and freed by mgx_clean (143 MB each at 512x512x64: 1.4 GB for m = 4).  Refused by
 *   solve_p together with "cycle_precision" = 32.  Three all-reduce calls per iteration on a process grid (one per pass).
 *   Read-only: "krylov_restarts" (times the last solve fell back to the true residual).
 * "krylov_precision" (64 default, or 32; any other value is refused; survives mgx_clean / mgx_init; acts only while "krylov" > 0, inert otherwise):
 *   32 = the preconditioner of the Krylov loop is the fp32 F-cycle of "cycle_precision" = 32 (A e = r / N from e = 0 on the fp32 copies, N = the
 *   residual norm the loop holds as the iteration starts).  The iterate, the recurrence, every inner product, the true residual and the stopping
 *   test stay fp64; GCR takes the inexact preconditioner as it is.  The loop adds no conversion pass in steady state: pass 3 leaves the next
 *   cycle's right-hand side in fp32 and pass 1 reads the cycle's fp32 result (mgx_krylov.hip).  "cycle_precision" stays 64 (the pair "krylov" > 0,
 *   "cycle_precision" = 32 is refused as before).  Refused at the first such solve like "cycle_precision" = 32 and in its words: a process
 *   grid larger than 1 x 1, relax_method = 'GS', option "rb_exact".
 *   Read-only: "krylov_mixed_iterations" (Krylov iterations run with an fp32 cycle since mgx_init); "mixed_iterations" does not count them.
 * "mixed_tail" (default 0, or 1; any other value is refused; survives mgx_clean / mgx_init; acts on the fp32 cycles of "cycle_precision" = 32 and
 *   "krylov_precision" = 32 only): the tail of a cycle -- the run of coarsest levels that are all small, a level being small with at most 32768
 *   cells and nz <= 32 (mgx_mixed_tail_first) -- runs inside one workgroup: one launch for a relax call on a small level, one for the part of a
 *   V-cycle from the first tail level down to the coarsest and back, one for the F-cycle's first leg, coarsest relax and the V-cycles that start
 *   inside the tail (k_tail32, mgx_mixed.hip).  The same device text as the per-launch kernels: the same bits as 0, which is one launch per colour
 *   pass and transfer on every level.  The levels above the tail keep their launches.  What changes is the launch count of mgx_counters: a
 *   tail launch counts as one, which is why the option is off until asked for.
 *   Read-only: "mixed_tail_launches" (launches of the tail kernel since mgx_init).
 * "mixed_ring" (default 0, or 1; any other value is refused; survives mgx_clean / mgx_init; no environment variable; may be set at any time;
 *   acts on the fp32 cycles of "cycle_precision" = 32 and "krylov_precision" = 32 and on mgx_mixed_op "relax" / "vcycle" only): 1 = the colour
 *   passes of the levels that are not small (more than 32768 cells, or nz > 32) and have nz = 16, 20, 24, 32, 40, 48 or 64
 *   (mgx_mixed_ring_levels) run the software-pipelined kernel k_relax32r (mgx_mixed.hip): the rows of the column and of its neighbours are
 *   requested two or three rows ahead into register rings, each neighbour row is read once, x and gam stay in registers.  The same operator
 *   and the same stored fp32 slots as the row-by-row kernel, summed in another order: other roundings, within the same 1e-5 of the fp64 pass,
 *   and the same iteration counts.  One launch per colour pass either way: mgx_counters does not move.  Every other level -- the small
 *   ones, so that "mixed_tail" = 0 and 1 stay the same bits under this option too, nz = 80, 96, 128 and every nz without an instance --
 *   keeps the row-by-row kernel.  0 = every launch and every bit as without the option.
 *   Read-only: "mixed_ring_passes" (colour passes served by the pipelined kernel since mgx_init).
 * "mixed_direct" (default 0, or 1; any other value is refused; survives mgx_clean / mgx_init; no environment variable; may be set at any time
 *   and steers later cycles only; acts on the fp32 cycles of "cycle_precision" = 32 and "krylov_precision" = 32 and on mgx_mixed_op "vcycle" /
 *   "coarsest" only): 1 = the coarsest solve of an fp32 cycle -- "ns_coarsest" sweeps from a zero correction, a fixed linear map of the level's
 *   right-hand side -- is one matrix-vector product e = B32 f, as the fp64 cycles have it under "coarsest_direct".  B32 is the fp64 operator
 *   (built from the unit vectors by the fp64 level's own relax kernel, in the parallel colour order the fp32 passes restate) rounded once to
 *   fp32; it is built at the first served solve and again when the matrices or "small_any_nz" change.  One launch (k_coarse_direct32,
 *   mgx_mixed.hip) instead of 4 "ns_coarsest" colour passes (2 or 4 "ns_coarsest" red-black), or one phase of the tail kernel under
 *   "mixed_tail" = 1: the same bits either way, the terms of a row being added in an order that depends on the number of cells alone.  Served
 *   (mgx_mixed_direct_cells): a coarsest level of nz = 2 or 4 (3 with "small_any_nz"), even nx and ny, at most 2048 cells, in a hierarchy of at
 *   least two levels, entered from a restriction, with "ns_coarsest" >= 1 and "tictoc" off; where the fp64 level has no one-workgroup relax
 *   kernel the sweeps run.  Not the bits of the sweeps: within the same 1e-5 of the fp64 solve, and the same iteration counts.  mgx_mixed_op
 *   "vcycle" entered at the coarsest level and "relax" keep the sweeps (they relax the correction they find).  0 = every launch and every bit
 *   as without the option.  The fp64 direct solve of "coarsest_direct" keeps its own operator and is not touched.
 *   Read-only: "mixed_direct_solves" (coarsest solves of fp32 cycles served by the product since mgx_init; a tail launch counts the solves it
 *   contains: as many as it has levels for an F-cycle tail, one for a V-cycle tail).
 * "small_any_nz" (default 0, or 1; any other value is refused; survives mgx_clean / mgx_init; no environment variable; may be set at any time:
 *   it steers the dispatch of later relax calls only): 1 = a relax call on a small level with nz = 3, 5, 6 or 7 -- the coarse ends of the
 *   nz = 24, 48, 96 hierarchies, and of nz = 20, 28, 40, 80 under "hold_odd_nz" -- runs in one workgroup and one launch, as the nz = 2 and 4
 *   levels do, instead of one launch per colour pass plus one per halo fill.  Served: a level whose four sides are physical (a fully gathered
 *   level included; not a level with neighbours or a periodic side) with even nx and ny and at most 1024 columns, relax_method 'FC' or 'RB'
 *   (cmatrix 'simple', the parallel pass of "rb_seq" = 0, the plane loop of "rb_exact", the sequential order by default: the walk at nz = 3,
 *   the plane loop at nz = 5).  nz = 3: four columns per lane (k_relax_wave, mgx_relax_coarse.hip); nz = 5, 6, 7: one thread per column with
 *   the coefficients in registers up to 256 columns (k_relax_reg), the colour loop inside one workgroup above (k_relax_small,
 *   mgx_relax.hip).  The same rows as the colour passes: four colours, 'simple', the parallel pass and "rb_exact" keep their bits; the
 *   sequential order by default stays within its 1e-12 of max|p| per call.  A closed, un-gathered coarsest level of nz = 3 and at most 2048
 *   cells (16 x 16 x 3) also takes the direct solve of "coarsest_direct", whose operator is rebuilt when this option changes.  Declined by
 *   measurement, i.e. the launches of 0: the sequential order by default at nz = 6, 7, at nz = 5 above 64 columns and
 *   at nz = 3 with ny > 128 (only the in-kernel plane loop could serve them, and it does not beat the colour passes with their walk);
 *   'simple' red-black at nz = 6, 7 above 256 columns.  Not served either: relax_method 'GS', a timed call ("tictoc"), the folded transfers of
 *   "fuse_tail", levels above 1024 columns, nz >= 9, the fp32 cycles.  0 = the dispatch without these instances, launch for launch; what changes with 1 is the
 *   launch count of mgx_counters, which is why it is off until asked for.
 *   Read-only: "small_any_nz_calls" (relax calls and direct coarsest solves served by these instances since mgx_init).
 * "periodic" (default 0; a bit mask, any value outside 0..3 is refused; survives mgx_clean): 1 = the domain wraps in the i direction (east-west,
 *   the plane index of the solver's layout), 2 = in the j direction (north-south), 3 = both.  Read by mgx_init: set it BEFORE mgx_init; while a
 *   solver is initialised a different value is refused (mgx_clean, set, mgx_init).  Served on one rank and on every process grid mgx_init
 *   takes; on a grid the hooks (mgx_set_comm, mgx_rccl_connect) must be installed BEFORE mgx_init, which refuses a periodic grid without them.  Along a periodic direction a level with ONE rank has the rank itself as neighbour (the local wrap: the un-decomposed direction of a
 *   strip of ranks, and every fully gathered level, where each rank holds the whole periodic domain); a level with several has the rank at the
 *   other end of the row or column, (pi +- incx) mod npx -- then one rank can be the neighbour on several sides (mgx_exchange_plan,
 *   mgx_level_table_periodic).  Either way (mgx_level_info) the side is an open
 *   side like a rank seam: no mirror halo, no zero flux in compute_rhs, and the velocity on it is corrected.  Every halo cell in a periodic
 *   direction of every field of every level (p, b, r; dx, dy, zeta, h; zr, zw with two halo columns; cA; the masks) is the image of the interior
 *   cell one period away; a closed direction is what it was; a corner between a periodic and a closed side is the closed side's image of the
 *   wrapped edge, a corner between two periodic sides wraps both ways.  Inputs: the halo entries of dx, dy, zeta, h, rmask ON a periodic side of the
 *   domain are ignored (replaced by the interior one period away -- the rank's own, or that of the rank at the other end); a rank seam inside
 *   the domain is what it was (the halo of rmask there is the caller's, cut from the global mask).  u, v, w come as a model hands them over after
 *   its own exchange -- halo columns across a periodic side hold the values from one period away, and the face on the wrap seam is held twice:
 *   u(nx+1) of the last rank of a row is u(1) of its first rank (on one rank, its own), likewise v(ny+1); the duplicated faces come back equal
 *   bit for bit if they went in so.
 *   Served: relax_method 'FC', 'RB' (the sequential order starts its walk at plane 1 and reads the wrapped image of plane nx as it was before
 *   the pass, the rule of a rank seam) and 'GS' (the hyperplane sweep of a level with neighbours: the wrapped images are those of the sweep
 *   before, filled once per sweep -- the rule of a rank seam too), "krylov", bmask, the per-call mask, "warm_start", the device entry points,
 *   "async".  Refused at the solve, on one rank and on a grid: "cycle_precision" = 32 and "krylov_precision" = 32 (the fp32 copies have mirror
 *   halos only); refused at the set: a change of the option under a live hierarchy.  The halo fill of a solver field is one launch behind
 *   every colour pass: k_halo_wrap where every neighbour is the rank itself; with the pushes, k_halo_exchange on a level that has other ranks too
 *   (a direction whose neighbour is the rank itself is a direct copy inside it: no slab, no flag); on the hooks that copy rides in the unpack
 *   launch.  Option "overlap" = 1 runs its one-stream pass on a periodic hierarchy (same bits).  Four colours give every rank, bit for bit, its
 *   block of the one-rank solution (tests/test_gpu_periodic_grid.py); the kernels that need a closed level (the
 *   persistent and one-workgroup relax, the restriction chain, the zeta chain, the direct coarsest solve) decline such a level, so a periodic
 *   hierarchy runs the launches of a level with neighbours (profiles/periodic_time.json).  mgx_transport() reports the wrap.
 * "hold_odd_nz" (default 0, or 1; any other value is refused; survives mgx_clean; no environment variable): 1 = once a level has an odd nz the
 *   coarser levels keep that nz and go on coarsening in x and y only, down to the horizontal bound of the hierarchy (mgx_level_table_hold), instead
 *   of the reference's nz / 2, which drops the top row of an odd level and diverges wherever such a level is not the coarsest (128 x 128 x 40:
 *   nz 40, 20, 10, 5, 2 becomes 40, 20, 10, 5, 5, 5).  Vertical sizes such as 20, 28, 40, 80 then converge like their even neighbours.  Read by
 *   mgx_init: set it BEFORE mgx_init; while a solver is initialised a different value is refused (mgx_clean, set, mgx_init).  A size whose nz
 *   stays even down to 2 has the same table, kernels, launch counts and bits with either value.  Between two levels of equal nz (a held pair)
 *   fine2coarse and coarse2fine are the reference's 2-D operators applied to every row (fine2coarse_2D, coarse2fine_2D_linear / _nearest,
 *   mg_intergrids.f90) in the reference's order of operations (mgx_hold.hip); the down leg of a cycle runs compute_residual and the restriction as
 *   two launches there, and the kernels that fold a transfer into another pass decline the pair.  An odd nx or ny on a level and an odd nz on level 1
 *   stay refused.  Served: relax_method 'FC', 'RB' in its modes and 'GS', "krylov" with fp64 cycles, bmask, "periodic", process grids, the device
 *   entry points.  Refused at the solve where the hierarchy has a held pair: "cycle_precision" = 32, "krylov_precision" = 32 and with them
 *   "mixed_tail" (the transfers of the fp32 copies halve nz).  mgx_mixed_tail_first keeps describing the hierarchy of hold_odd_nz = 0.
 * "hold_z_levels" (default 0, or m = 1..8; any other value is refused; survives mgx_clean; no environment variable): semi-coarsening at the
 *   fine end.  The first m coarsenings (levels 1 -> 2 ... m -> m + 1) keep nz and halve nx, ny; from level m + 1 on the hierarchy is built as
 *   without the option -- the reference's halving, or the rule of "hold_odd_nz" where that is set (mgx_level_table_semi).  For cells that are
 *   taller than wide (the seamount at 128 x 128 x 16: dx = 78 m against dz = 250 m), where the z-line smoother leaves the horizontally
 *   oscillatory error alone and full coarsening never repairs the aspect ratio: mgx_hold_z_hint names the m after which the cells are no
 *   longer taller than wide (DESIGN.md 7.1.1 has the iteration counts).  Read by mgx_init: set it BEFORE mgx_init; while a solver is
 *   initialised a different value is refused (mgx_clean, set, mgx_init).  0 = every table, kernel, launch count and bit as without the option.
 *   The held pairs are those of "hold_odd_nz" and are served as there: the reference's 2-D transfers row by row (mgx_hold.hip), the one-launch
 *   restriction chain ends above a held pair and may serve the halving pairs below the last one, the transfers folded into a relax ("fuse_tail")
 *   decline it.  New here: the down leg of a held pair with an even nz (residual + 2-D restriction) and the closing residual of a solve_p
 *   iteration ("fuse_closing") on a held pair of levels 1 and 2 are ONE kernel that never writes r, with the bits of the two launches
 *   (mgx_resrest_held.hip): matrix-free where the level has its slopes, on the stored slots otherwise (bmask, a matrix set through
 *   mgx_set_field); with "keep_r", "exact_halos", "hold_z_fuse" = 0 or MGX_NO_RESREST the two launches stay, as they do on a pair with an odd nz.  Served: relax_method 'FC', 'RB' in its modes and 'GS', "krylov" with fp64
 *   cycles, bmask and the per-call mask, "periodic", process grids, "hold_odd_nz", the device entry points (the 2-D zeta chain of
 *   mgx_update_zeta_device does not depend on nz), the _f32 state entries.  Refused at the solve, in the words of "hold_odd_nz": the fp32
 *   cycles.  A held level 2 has a quarter of level 1's cells instead of an eighth: a cycle costs more (profiles/hold_z_time.json).
 *   Read-only: "hold_z_fused" (down legs and closing residuals of held pairs served by the fused kernel since mgx_init).
 * "hold_z_fuse" (default 1, or 0; any other value is refused; survives mgx_clean; no environment variable; may be set at any time): A/B of the
 *   one-kernel down leg of a held pair.  0 = compute_residual and the 2-D restriction stay two launches on every held pair, and the closing
 *   residual of a solve_p iteration on a held pair of levels 1 and 2 is not fused either; the same bits (scripts/hold_z_time.py times both).
 * Read-only through mgx_get_option: "p2p_failed" (a peer-to-peer wait of THIS rank timed out since the ranks last agreed: see below),
 *   "overlapped_passes", "tall_stored_passes" (colour passes of nz = 80, 96, 128 levels served by the stored-coefficient tall-column kernel
 *   since mgx_init: bmask, mgx_set_field(cA) or MGX_NO_MF; 0 while the matrix-free form runs or under MGX_NO_TALL). */
int mgx_set_option(const char *name, int value);
/* Option "async" (default 0): the cycle / operator entry points (mgx_vcycle, mgx_vcycle2, mgx_fcycle, mgx_relax, mgx_fine2coarse,
 * mgx_coarse2fine) only ENQUEUE their kernels on the solver's stream and return -- what a GPU-resident model wants between its own
 * kernels.  mgx_synchronize() waits for the stream and reports what the device flagged meanwhile (a peer that never showed up, a
 * rejected launch); every entry point that returns data to the host (mgx_residual, mgx_solve_p, mgx_get_field ...) synchronises anyway. */
int mgx_synchronize(void);
/* read back an option, or an integer / logical member of /nhparam/ as mgx_init took it from nh_namelist ("bmask", "nsmall",
 * "solver_maxiter", "ns_coarsest", "ns_pre", "ns_post", "netcdf_output", "aggressive"): the reference's drivers read these module
 * variables of mg_namelist directly (e.g. `if (bmask)`, mg_testseamount.f90) */
int mgx_get_option(const char *name, int *value);
/* print_tictoc (mg_tictoc.f90:114-153): timer table (seconds, calls per level) to `path` (NULL = "fort.10") */
int mgx_print_tictoc(const char *path);
/* tic(lev, name) / toc(lev, name) (mg_tictoc.f90:21-111) for the CALLER's own sections -- the reference's drivers bracket their main
 * program with them (mg_testseamount.f90:37,220).  Host wall clock like the reference's system_clock; toc waits for the solver's stream
 * first, so that the section contains the GPU work enqueued inside it.  They share the table of mgx_print_tictoc with the library's own
 * timers (option "tictoc"); the table survives mgx_clean, as the reference's module variables survive nhydro_clean. */
int mgx_tic(int lev, const char *name);
int mgx_toc(int lev, const char *name);

/* ---- measurement helpers used by bench.py (timed with HIP events on the solver's stream) ---- */
/* run `reps` smoother sweeps on level `lev` (reps x relax(lev,1)); *ms = average milliseconds per sweep */
int mgx_time_relax(int lev, int reps, float *ms);
/* self-test of the arithmetic identity the level-1 colour pass relies on for its per-column divisors: a[i] / b[i] by
 * the hardware fp64 division sequence against the refined-reciprocal quotient; *nbad = pairs whose bits differ (0 for operands whose
 * quotient and operands sit in the normal range).  Host arrays; needs no mgx_init. */
int mgx_selftest_divc(const double *a, const double *b, int n, long long *nbad);
int mgx_time_residual(int lev, int reps, float *ms);
/* counters since mgx_init: out[0]=kernel launches, out[1]=halo fills, out[2]=exchanges, out[3]=allreduces */
int mgx_counters(long long *out);
/* test hook of the fp32 cycle of option "cycle_precision" = 32 (single rank): converts the level's fp64 fields into its fp32 copy, runs one
 * fp32 operator, converts the result back.  op = "relax" (n sweeps on p, b of level lev -> p), "residual" (p, b -> r), "fine2coarse"
 * (r of lev -> b of lev+1, p of lev+1 = 0), "coarse2fine" (p of lev += interpolation of p of lev+1), "resrest" (restriction of b - A p of lev
 * -> b of lev+1, p of lev+1 = 0: the down leg of a V-cycle), "vcycle" (Vcycle(lev) on the copies from p, b of level lev; p of every level
 * lev .. nlevs = the correction the cycle leaves there: every entry of the tail kernel of option "mixed_tail" from a rough state, where a solve
 * only ever enters with a zero correction), "coarsest" (lev = nlevs only: the coarsest solve of a cycle, b of the coarsest level -> p from a
 * zero correction -- the product where option "mixed_direct" is on and the level served, otherwise the "ns_coarsest" sweeps).  No Fortran
 * counterpart. */
int mgx_mixed_op(const char *op, int lev, int n);
/* test hook of the three passes of option "krylov" (mgx_krylov.hip; single rank, after mgx_matrices): runs ONE pass on level 1 through the
 * wrapper solve_p calls for it, on the buffers solve_p uses (its ring of direction pairs, partial sums and device scalars, grid(1)%p and %r,
 * which it overwrites), and adds no kernel of its own.  Fields are host arrays (nz, 0:ny+1, 0:nx+1) as in mgx_get_field, halos taken as given.
 * nd = retained pairs (0..8); pair n sits in ring slot slot[n] (distinct values of 0..nd; NULL = 0..nd-1), the pair in work in the free slot.
 *   op = "apply":  fields = z, q, q_1 .. q_nd.  q = A z is written; sout[0..nd-1] = (q, q_n).  z needs valid halos.
 *   op = "ortho":  fields = z, q, r, z_1, q_1, .. z_nd, q_nd; sin[0..7] = (q, q_n), sin[8..16] = (q_n, q_n) BY RING SLOT.  z, q are rewritten
 *                  (z -= sum beta_n z_n, q -= sum beta_n q_n, beta_n = sin[n] / sin[8 + slot[n]]); sout[0] = (q, q), sout[1] = (r, q).
 *   op = "update": fields = p, r, z, q; sin = {s, t}; the new pair's ring slot is nd.  p += (t / s) z, r -= (t / s) q are rewritten;
 *                  sout[0] = ||r||^2, or -1 when s, t allow no step (p, r untouched); sout[1] = what the pass filed under that slot (s).
 *   op = "apply32":  pass 1 of "krylov_precision" = 32.  fields = e, z, q, q_1 .. q_nd; sin[0] = 1 / sigma.  e holds doubles that fp32
 *                  represents exactly; the hook demotes them into the fp32 copy of level 1.  z = (double)e * sin[0] (whole array, halo cells
 *                  included) and q = A z are written; sout[0..nd-1] = (q, q_n).  Refused where "cycle_precision" = 32 is.
 *   op = "update32": pass 3 of "krylov_precision" = 32.  fields = p, r, z, q, f; sin = {s, t, sigma}.  As "update", and f (demoted into the fp32
 *                  copy on the way in, promoted exactly on the way out) receives (float)(sigma r) of the new r; no step: f untouched too.
 * Sums run over interior cells.  path (may be NULL) receives the launch taken: matrix-free operator (1) or stored slots (0), cmatrix='real',
 * the non-temporal variant, gx, gy of pass 1's block map.  No Fortran counterpart. */
int mgx_krylov_op(const char *op, int nd, double *const *fields, const int *slot, const double *sin, double *sout, int *path);

/* ---- peer-to-peer halo transport (replaces the MPI_Isend/MPI_Irecv/MPI_Waitall of fill_halo_3D[_relax],
 * mg_mpi_exchange.f90:504-718, for the p/b/r halos of the cycle) ----
 * Ranks of one node write their edges straight into the neighbours' receive buffers over xGMI (device memory shared
 * through hipIpc) and raise a flag there; the receiver waits on its local flag and unpacks -- one kernel per halo fill,
 * no host step, no callback.  Set-up is collective: every rank calls mgx_p2p_prepare (after mgx_init), the handle blobs
 * (mgx_p2p_handle_bytes() each) are all-gathered in rank order by the caller, every rank calls mgx_p2p_connect with
 * the concatenation.  mgx_set_option("p2p", 0|1) switches between this transport and the exchange callback (all
 * ranks together).  A neighbour that never shows up ends the wait after 5 s (option "p2p_timeout_ms" / MGX_P2P_TIMEOUT_MS); the rank
 * that waited does NOT fall back alone: it keeps exchanging and the ranks agree at the next global_sum (every solve_p iteration, every
 * mgx_residual norm), whose all-reduce carries a second value "a wait of mine timed out": if any rank says so, EVERY rank switches
 * to the hooks, rewinds its sequence numbers and returns the same error (the solve in progress is void; repeat it).  Test hook:
 * option "p2p_test_drop" = n makes the n-th halo exchange of this rank keep its flags down; "p2p_failed" (mgx_get_option) reads the
 * local marker. */
int mgx_p2p_handle_bytes(void);
int mgx_p2p_prepare(void *handles_out);
int mgx_p2p_connect(const void *all_handles, int nranks);
long long mgx_p2p_exchanges(void);

/* ---- more than one solver in a process (the reference has exactly one: module-global grid(:), mg_grids.f90:113-117) ----
 * Instance 0 exists from the start and is what every thread acts on.  mgx_instance_create returns the id of a new, empty
 * instance; mgx_instance_select(id) makes all later mgx_* calls OF THE CALLING THREAD act on it (thread-local selection:
 * one thread per instance may run concurrently; two threads must not drive the same instance at the same time).  Uses:
 * several nested domains coupled from one process; several ranks of one job as threads of one process (each with its own
 * stream, mgx_set_stream) where a box admits fewer processes than ranks -- they are connected with mgx_set_comm hooks or with
 * mgx_p2p_prepare + mgx_p2p_local_pointers + mgx_p2p_connect_pointers (same-process buffers need no hipIpc).
 * mgx_instance_destroy frees an instance (never 0); mgx_instance_current returns the calling thread's id. */
int mgx_instance_create(void);
int mgx_instance_select(int id);
int mgx_instance_current(void);
int mgx_instance_destroy(int id);
int mgx_p2p_local_pointers(void **slab, void **flags);
int mgx_p2p_connect_pointers(void *const *slabs, void *const *flags, int nranks);

const char *mgx_last_error(void);
const char *mgx_version(void);

#ifdef __cplusplus
}
#endif
#endif
