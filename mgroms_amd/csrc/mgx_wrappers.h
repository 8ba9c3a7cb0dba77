// The one declaration of every kernel wrapper of libmgx.so: the extern "C" entry points the HIP translation units and mgx_rccl.cpp
// define, and the two structs that cross that boundary by pointer.  Included (through mgx_internal.h) by the files that define the
// wrappers and by the files that call them, so a definition that drifts from its prototype is a conflicting declaration at compile time
// rather than a call with shifted arguments (extern "C" names carry no types: the linker cannot tell).
#pragma once
// (no includes: mgx_internal.h includes this file behind LevView, GeoView, Sides and LevView32)

// one generic halo / copy operation on a reference-layout array (mgx_setup.hip: k_rect)
struct RectOp { int op, nzz, nh, ny, j0, j1, i0, i1, mj, cj, mi, ci, mj2, cj2, mi2, ci2; };
// the model state of a call.  u, v, w point to doubles (f32 = 0) or to floats (f32 = 1: the mgx_*_f32 entries); the wrappers hand the kernels
// the typed view of it.  rmask: i-fastest copy of the level-1 mask (only read when bmask).  view = 1: u, v, w are the model's own padded arrays
// and `str` holds their strides (the *_view entries, include/mgx.h); view = 0: the densely packed arrays, whose strides the wrappers work out
// from the level's shape (str is not read).  u, v, w name the first logical element either way: u(1,0,1), v(0,1,1), w(0,0,0).
struct ModelView { void *u, *v, *w; double *rmask; int bmask, f32; int view; mgx_state_strides str; };
// the kernels' state: element strides from row j to j + 1 (sj) and from level k to k + 1 (sk) of each array; the i stride is 1
template <typename T> struct ModelViewT { T *u, *v, *w; double *rmask; int bmask; long long usj, usk, vsj, vsk, wsj, wsk; };
struct ExMap;   // mgx_export.h: the geometry of one CSR export

extern "C" {

// what a colour pass reports: the return value of mgxk_relax_colour, mgxk_relax_ks and mgxk_relax_tall (0 from the last two: nothing ran)
enum {
  PASS_MIRRORS = 1,      // the kernel stored the physical images of p itself: no k_halo_phys behind it
  PASS_D0 = 2,           // it wrote L->d0w, the walk's d0 of sequential-order red-black
  PASS_TALL_STORED = 4,  // it was the stored-coefficient tall-column pass (counter "tall_stored_passes")
};

// what serves a direction of a halo fill: present[d] of mgxk_halo_pack_all and mgxk_halo_p2p
enum {
  HALO_NONE = 0,    // no neighbour, nothing due
  HALO_PEER = 1,    // another rank: buffers (and, with the pushes, flags)
  HALO_SELF = 2,    // the rank itself (option "periodic", one rank along the direction): the halo is the interior the opposite side packs
  HALO_MIRROR = 3,  // a closed side whose image is still due (mgxk_halo_p2p on a mixed level only): the halo is the interior this side packs
};

// ---- mgx_relax.hip ----
int mgxk_relax_gs_sweep(hipStream_t st, const LevView *L, int real);
int mgxk_relax_small(hipStream_t st, const LevView *L, int nsweeps, int method, int real, Sides ph, int mode, int any);
int mgxk_relax_colour(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph);
int mgxk_has_reg_kernel(const LevView *L);
void mgxk_snapshot_k1(hipStream_t st, const LevView *L);

// ---- mgx_rbseq.hip ----
void mgxk_rbseq_setup(hipStream_t st, const LevView *L);
int mgxk_rbseq_scan(hipStream_t st, const LevView *L, int rb, int have_d0);
int mgxk_rbseq_wants_d0(const LevView *L);
int mgxk_rbseq_scan_apply(hipStream_t st, const LevView *L, int rb, Sides ph, int snapw, int have_d0, unsigned int *words, unsigned int seq,
                          int *err, int test_stall, long long min_cells);
int mgxk_rbseq_walk_apply(hipStream_t st, const LevView *L, int rb, Sides ph, int snapw);
void mgxk_rbseq_rho(hipStream_t st, const LevView *L, double *out);
void mgxk_rbseq_gdecay(hipStream_t st, const LevView *L, double *out);
int mgxk_rbseq_window_rows(const double *decay, int nz);
void mgxk_rbseq_d0(hipStream_t st, const LevView *L, int rb);
int mgxk_rbseq_window_planes(double rho);
int mgxk_rbseq_window(hipStream_t st, const LevView *L, int rb, Sides ph, int snapw, int m, int kcut);
int mgxk_set_rbseq_timeout(double ms);
void mgxk_rbseq_apply(hipStream_t st, const LevView *L, int rb, Sides ph, int snapw);

// ---- mgx_relax_tall.hip ----
int mgxk_relax_tall(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph);

// ---- mgx_relax_ks.hip ----
#ifdef MGX_KS_STAMP  // probe hook (scripts/probe): the per-plane time stamps of the persistent relax kernel
int mgxk_ks_stamps(long long *out);
#endif
int mgxk_relax_ks(hipStream_t st, const LevView *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, Sides ph);
int mgxk_relax_ks_pair(hipStream_t st, const LevView *L, int i0, int nplanes, int real, Sides ph);
int mgxk_set_ksp_timeout(double ms);
int mgxk_relax_ks_persist(hipStream_t st, const LevView *L, int nsweeps, int real, Sides ph, unsigned int *done, unsigned int base, int *err,
                          int stall);

// ---- mgx_relax_coarse.hip ----
int mgxk_relax_wave(hipStream_t st, const LevView *L, int nsweeps, int method, int real, Sides ph, int mode, int any);
int mgxk_coarse_direct_cells(const LevView *L, int any);
int mgxk_coarse_direct_build(hipStream_t st, const LevView *L, int nsweeps, int method, int real, Sides ph, int mode, double *pb, long long stride,
                             double *M, int any);
int mgxk_coarse_direct_apply(hipStream_t st, const LevView *L, const double *M, double *part, unsigned int *cnt, Sides ph, int any);
int mgxk_coarse_direct_slabs(int n);
int mgxk_relax_wave_fused(hipStream_t st, const LevView *L, const LevView *C, int nsweeps, int method, int real, Sides ph, int flags, int mode);

// ---- mgx_resrest.hip ----
int mgxk_residual_restrict_grid(const LevView *F, const LevView *C);
int mgxk_residual_restrict_ex(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero, double *partial,
                              double *dup);
int mgxk_residual_restrict(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero);

// ---- mgx_resrest_held.hip ----
int mgxk_residual_restrict_held_grid(const LevView *F, const LevView *C);
int mgxk_residual_restrict_held(hipStream_t st, const LevView *F, const LevView *C, double *dst, int real, Sides ph, double *zero, double *partial,
                                double *dup);

// ---- mgx_residual.hip ----
int mgxk_residual_nblocks(const LevView *L);
void mgxk_residual(hipStream_t st, const LevView *L, double *partial, double *out, int real, int want_norm, Sides ph);
void mgxk_reduce(hipStream_t st, const double *partial, int n, double *out);
void mgxk_sumsq(hipStream_t st, const LevView *L, const double *a, double *partial, double *out);
void mgxk_dot(hipStream_t st, const LevView *L, const double *a, const double *b, double *partial, double *out);

// ---- mgx_transfer.hip ----
int mgxk_restrict_chain_served(const LevView *const *levels, int dep);
void mgxk_restrict_chain(hipStream_t st, const LevView *const *levels, int dep, Sides ph);
void mgxk_fine2coarse(hipStream_t st, const LevView *F, const LevView *C, double *dst, Sides ph, double *dup, double *zero);
void mgxk_coarse2fine(hipStream_t st, const LevView *F, const LevView *C, const double *src, int linear, Sides ph, int keep_r, int skip1);

// ---- mgx_halo.hip ----
void mgxk_halo_phys(hipStream_t st, const LevView *L, double *a, Sides ph);
void mgxk_halo_wrap(hipStream_t st, const LevView *L, double *a, int im, int jm);
void mgxk_halo_mixed_corners(hipStream_t st, const LevView *L, double *a, int mSW, int mSE, int mNE, int mNW);
void mgxk_halo_pack_all(hipStream_t st, const LevView *L, double *a, double *const *bufs, const int *present, int unpack);
void mgxk_halo_p2p(hipStream_t st, const LevView *L, double *a, double *const *rbuf, double *const *lbuf, unsigned long long *const *rflag,
                   unsigned long long *const *lflag, const int *present, unsigned long long seq, unsigned int *counter, int *err, const int *mixed,
                   int drop);
int mgxk_set_p2p_timeout(double ms);
void mgxk_err_to_double(hipStream_t st, const int *err, int extra, double *out);
void mgxk_gather_place(hipStream_t st, const LevView *C, double *dstjs, const double *blk, int nxc, int nyc, int l, int m);
void mgxk_block_to_ref(hipStream_t st, const LevView *Cs, const double *js, double *blk);
void mgxk_gather_push(hipStream_t st, const LevView *Cs, const double *js, double *const *dst, unsigned long long *const *flags, int ng, int me,
                      unsigned long long seq, unsigned int *counter, int *err);
void mgxk_gather_place_wait(hipStream_t st, const LevView *C, double *dstjs, const double *blk, int nxc, int nyc, int l, int m,
                            unsigned long long *flag, unsigned long long seq, int *err);
void mgxk_split(hipStream_t st, const LevView *C, const LevView *Cs, const double *pc, double *dst, int l, int m);

// ---- mgx_layout.hip ----
void mgxk_divc_selftest(hipStream_t st, const double *a, const double *b, int n, unsigned long long *bad);
void mgxk_convert(hipStream_t st, const LevView *L, double *js, double *ref, int nslot, int slot, int dir);
void mgxk_convert8(hipStream_t st, const LevView *L, const double *ref);
void mgxk_convert2(hipStream_t st, const LevView *L, double *out0, double *out1, const double *ref);

// ---- mgx_hold.hip ----
void mgxk_fine2coarse_held(hipStream_t st, const LevView *F, const LevView *C, double *dst, Sides ph, double *dup, double *zero);
void mgxk_coarse2fine_held(hipStream_t st, const LevView *F, const LevView *C, const double *src, int linear, Sides ph, int keep_r, int skip1);

// ---- mgx_setup.hip ----
void mgxs_coarsen2d(hipStream_t st, const double *src, double *dst, int nyf, int nyc, int nxc, double fac);
void mgxs_zeta_view(hipStream_t st, const double *src, long long sj, double *dst, int nx, int ny);
void mgxs_rect(hipStream_t st, double *a, double *buf, const RectOp *R);
void mgxs_halo_ref_closed(hipStream_t st, double *a, int nzz, int nh, int ny, int nx);
int mgxs_zeta_chain_depth(void);
void mgxs_zeta_chain(hipStream_t st, double *const *lev, int ny, int nx, int nd);
void mgxs_ze2_js(hipStream_t st, const GeoView *G, const LevView *L);
void mgxs_zr_zw(hipStream_t st, const GeoView *G, double hlim, double theta_b, double theta_s);
void mgxs_define_matrix(hipStream_t st, const GeoView *G, int lev1, int phase);
void mgxs_slopes_ref(hipStream_t st, const GeoView *G);
void mgxs_zw_js(hipStream_t st, const GeoView *G, const LevView *L, double hlim, double theta_b, double theta_s);
void mgxs_pivots(hipStream_t st, const LevView *L);

// ---- mgx_depths.hip (the launches: mgx_choice_depths.h) ----
void mgxd_coarsen(hipStream_t st, const GeoView *F, int nxc, int nyc, int nzc, double *zrc, double *zwc, int block);
void mgxd_in(hipStream_t st, const double *zr, const double *zw, const mgx_depth_strides *s, const GeoView *G);
void mgxd_copy(hipStream_t st, const double *zr, const double *zw, const GeoView *G);
void mgxd_hz(hipStream_t st, const GeoView *G);
void mgxd_choice(int nx, int ny, int nz, int *out);

// ---- mgx_model.hip ----
void mgxm_ref2model(hipStream_t st, const double *src, double *dst, int rows, int nh, int nx, int ny);
void mgxm_ref2model_2d(hipStream_t st, const double *src, double *dst, int nx, int ny);
void mgxm_js_model(hipStream_t st, const LevView *L, double *js, double *md, int dir);
void mgxm_rhs_uf(hipStream_t st, const GeoView *G, const ModelView *M, double *fx);
void mgxm_rhs_vf(hipStream_t st, const GeoView *G, const ModelView *M, double *fx);
void mgxm_rhs_wf(hipStream_t st, const GeoView *G, const ModelView *M, double *fz);
void mgxm_flux_zero_face(hipStream_t st, const GeoView *G, double *f, int face, int pl);
void mgxm_flux_face_copy(hipStream_t st, const GeoView *G, double *f, double *buf, int face, int pl, int unpack);
void mgxm_rhs_accum(hipStream_t st, const GeoView *G, double *bm, const double *fu, const double *fv, const double *fw);
void mgxm_correct_uvw(hipStream_t st, const GeoView *G, const double *pm, const ModelView *M);

// ---- mgx_mixed.hip ----
int mgxx_relax_pass(hipStream_t st, const LevView32 *L, int i0, int istep, int nplanes, int jodd_fixed, int rb, int real, int snap, int ring);
void mgxx_ring_choice(int nx, int ny, int nz, int nplanes, int *out);
void mgxx_snapshot(hipStream_t st, const LevView32 *L);
void mgxx_residual(hipStream_t st, const LevView32 *L, int real);
void mgxx_resrest(hipStream_t st, const LevView32 *F, const LevView32 *C, int real);
void mgxx_restrict(hipStream_t st, const LevView32 *F, const LevView32 *C, const float *src);
void mgxx_coarse2fine(hipStream_t st, const LevView32 *F, const LevView32 *C, int linear);
enum { TAIL_RELAX = 0, TAIL_VCYCLE = 1, TAIL_FCYCLE = 2 };   // what one launch of the tail kernel runs: mode of mgxx_tail
int mgxx_tail(hipStream_t st, const LevView32 *const *levs, int nl, int mode, int lead, int n, int ns_pre, int ns_post, int ns_coarsest, int rb,
              int real, int linear, const float *dM, int dn);
int mgxx_tail_max_levels(void);
int mgxx_direct32_cells(int nx, int ny, int nz, int nlevs, int any);
void mgxx_direct32_round(hipStream_t st, const double *M64, float *M, int n);
int mgxx_coarse_direct32(hipStream_t st, const LevView32 *L, const float *M, int nlevs, int any);
void mgxx_to32(hipStream_t st, const LevView *D, const LevView32 *S, const double *src, float *dst, double scale);
void mgxx_to64(hipStream_t st, const LevView *D, const LevView32 *S, const float *src, double *dst, double scale, int add);

// ---- mgx_krylov.hip ----
long long mgxq_partials(const LevView *L);
void mgxq_path(const LevView *L, int *out);
void mgxq_apply(hipStream_t st, const LevView *L, double *qout, const double *const *qi, int nd, double *partial, double *sc, int real);
void mgxq_apply32(hipStream_t st, const LevView *L, const LevView32 *S, double isg, double *zout, double *qout, const double *const *qi, int nd, double *partial,
                  double *sc, int real);
void mgxq_ortho(hipStream_t st, const LevView *L, double *z, double *q, const double *r, const double *const *zi, const double *const *qi,
                const int *slot, int nd, const double *sc, const double *qq, double *partial, double *out);
void mgxq_update(hipStream_t st, const LevView *L, double *p, double *r, const double *z, const double *q, const double *st2v, double *qq_new,
                 double *partial, double *out);
void mgxq_update32(hipStream_t st, const LevView *L, const LevView32 *S, double *p, double *r, const double *z, const double *q, double sigma, const double *st2v,
                   double *qq_new, double *partial, double *out);

// ---- mgx_export.hip (ExMap: mgx_export.h, the geometry of one export) ----
void mgxe_probe_fill(hipStream_t st, const LevView *L, double *a, const ExMap *m, int colour);
void mgxe_csr_mark(hipStream_t st, const LevView *L, const double *a, const ExMap *m, int colour, unsigned long long *mask);
int mgxe_csr_sums_len(long long n);
void mgxe_csr_count(hipStream_t st, const unsigned long long *mask, long long n, long long *sums);
void mgxe_csr_rowptr(hipStream_t st, const unsigned long long *mask, long long n, const long long *sums, int *rowptr);
void mgxe_csr_scatter(hipStream_t st, const LevView *L, const double *a, const ExMap *m, int colour, const unsigned long long *mask, const int *rowptr,
                      int *col, double *val, double sign);

// ---- mgx_rccl.cpp ----
const char *mgxr_last_error(void);
const char *mgxr_library(void);
int mgxr_connected(void);
int mgxr_nranks(void);
int mgxr_get_unique_id(void *out);
int mgxr_connect(const void *idbytes, int nranks, int rank);
void mgxr_disconnect(void);
int mgxr_exchange(hipStream_t st, int n, const int *peer, double *const *sendbuf, double *const *recvbuf, const int *count);
int mgxr_allreduce(hipStream_t st, double *buf, int n);
int mgxr_allgather(hipStream_t st, const int *group, int ng, const double *sendbuf, double *recvbuf, int count);

// ---- mgx_api.cpp ----
#ifdef MGX_RBSEQ_TRACE  // probe hook (scripts/probe): the trace words behind a level's progress flags of the fused red-black walk
int mgx_debug_rbs(int lev, unsigned long long *out8);
#endif
}  // extern "C"
