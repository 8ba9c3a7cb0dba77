// Force-included (-include) in front of a unit compiled host-only: every kernel launch, hipGetLastError and hipFuncSetAttribute of the
// unit goes to the recorder of record_main.cpp instead of the HIP runtime.  No source file is edited.
#pragma once
#include <hip/hip_runtime.h>
#include "mgx_internal.h"

void rec_launch(const void *kernel, dim3 grid, dim3 block, size_t lds);
void rec_arg(long long v);
void rec_arg(const LevView &L);
void rec_arg(const LevView32 &L);
void rec_arg(const Sides &s);
void rec_arg(const void *p);
void rec_end();
hipError_t rec_last_error();
hipError_t rec_set_attribute(const void *kernel, hipFuncAttribute attr, int value);

inline void rec_arg(int v) { rec_arg((long long)v); }
inline void rec_arg(unsigned int v) { rec_arg((long long)v); }
inline void rec_arg(bool v) { rec_arg((long long)v); }
// the hand-off block of the fused walk (RbFuse, a struct of mgx_rbseq.hip that this header cannot name): recognised by its members
void rec_fuse(const Sides &ph, const int (&v)[6], long long min_cells, const void *flag, unsigned int seq, const void *err);
template <class T>
inline auto rec_arg(const T &f) -> decltype((void)f.nworkers) {
  const int v[6] = {f.KR, f.nt, f.nchunk, f.nkz, f.nworkers, f.test_stall};
  rec_fuse(f.ph, v, f.min_cells, f.flag, f.seq, f.err);
}
// the other structs that a kernel of the units takes by value, by their members too: LevChain (mgx_transfer.hip), HaloBufs, HaloXchg, HaloP2P
// -- the plan of the peer-to-peer exchange in full --, GatherP2P (mgx_halo.hip), Slots8 (mgx_layout.hip), KrDirs (mgx_krylov.hip) and the typed
// model state (mgx_wrappers.h); rec_text appends to the launch line
void rec_text(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void rec_arg(const GeoView &G);
inline void rec_arg(double v) { rec_text("%.17g ", v); }
inline void rec_arg(unsigned long v) { rec_arg((long long)v); }
inline void rec_arg(unsigned long long v) { rec_arg((long long)v); }
template <class P> inline int rec_mask(P *const *p, int n) { int m = 0; for (int q = 0; q < n; q++) m |= (p[q] != nullptr) << q; return m; }
template <class T>
inline auto rec_arg(const T &c) -> decltype((void)c.v[4].plane) { rec_text("Chain( "); for (const LevView &L : c.v) rec_arg(L); rec_text(") "); }
template <class T>
inline auto rec_arg(const T &h) -> decltype((void)h.b[7], (void)h.present[7]) {
  rec_text("HB(b=%02x,present=", rec_mask(h.b, 8)); for (int d = 0; d < 8; d++) rec_text("%d", h.present[d]); rec_text(") ");
}
template <class T>
inline auto rec_arg(const T &h) -> decltype((void)h.rflag[7]) {
  rec_text("HX(rbuf=%02x,lbuf=%02x,rflag=%02x,lflag=%02x,present=", rec_mask(h.rbuf, 8), rec_mask(h.lbuf, 8), rec_mask(h.rflag, 8), rec_mask(h.lflag, 8));
  for (int d = 0; d < 8; d++) rec_text("%d", h.present[d]);
  rec_text(") ");
}
template <class T>
inline auto rec_arg(const T &p) -> decltype((void)p.blk0[8]) {
  rec_text("PP(drop=%d,flag=%02x,seq=%llu,counter=%d,err=%d,m=%d%d%d%d,ipt=%d,nreal=%d,blk0=", p.drop, rec_mask(p.flag, 8), p.seq, p.counter != nullptr, p.err != nullptr,
           p.mSW, p.mSE, p.mNE, p.mNW, p.ipt, p.nreal);
  for (int d = 0; d < 9; d++) rec_text("%d%s", p.blk0[d], d < 8 ? "," : ") ");
}
template <class T>
inline auto rec_arg(const T &g) -> decltype((void)g.ng) {
  rec_text("GP(dst=%x,flag=%x,ng=%d,me=%d,seq=%llu,counter=%d,err=%d) ", rec_mask(g.dst, 4), rec_mask(g.flag, 4), g.ng, g.me, g.seq, g.counter != nullptr, g.err != nullptr);
}
template <class T>
inline auto rec_arg(const T &o) -> decltype((void)o.s[7]) { rec_text("Slots(%02x) ", rec_mask(o.s, 8)); }
template <class T>
inline auto rec_arg(const T &d) -> decltype((void)d.slot[7]) {
  rec_text("KrDirs(n=%d,q=%02x,z=%02x,slot=", d.n, rec_mask(d.q, 8), rec_mask(d.z, 8)); for (int n = 0; n < 8; n++) rec_text("%d%s", d.slot[n], n < 7 ? "," : ") ");
}
template <class T>
inline void rec_arg(const ModelViewT<T> &m) { rec_text("M%zu(u=%d,v=%d,w=%d,rmask=%d,bmask=%d) ", 8 * sizeof(T), m.u != nullptr, m.v != nullptr, m.w != nullptr, m.rmask != nullptr, m.bmask); }
template <typename K, typename... A>
inline void rec_record(K *kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, A... a) {
  rec_launch((const void *)kernel, grid, block, lds);
  (rec_arg(a), ...);
  rec_end();
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, ...) rec_record(kernel, __VA_ARGS__)
#define hipGetLastError rec_last_error
#define hipFuncSetAttribute rec_set_attribute
