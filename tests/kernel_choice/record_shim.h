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
